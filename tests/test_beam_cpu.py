"""Beam search without a GPU: the transformers 4.34 restatement (tests/beam_ref.py) against recorded HF output and hand-built
scorer cases, the keyword checks of resolve_beam_kwargs, and the C ABI's parameter block."""
import ctypes as C
import copy
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from music2midi_amd import native, synth
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config
from music2midi_amd.generation import BeamConfig, resolve_beam_kwargs
from oracle.t5 import T5Oracle

from beam_ref import _Hyps, beam_search, oracle_step, pick_best

GOLDEN = Path(__file__).resolve().parent / "golden" / "beam.npz"
LN = math.log


def _tiny_oracle():
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["model"]["t5"].update(d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2)
    geom = T5Geometry(load_config(cfg).model.t5)
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    synth.force_eos_head(sd, geom)
    return T5Oracle(geom, sd), geom


def _upto_eos(row, eos):
    r = [int(v) for v in row]
    return r[: r.index(eos) + 1] if eos in r else r


def test_restatement_reproduces_recorded_hf_beam_search():
    data = np.load(GOLDEN)
    B, S, L = (int(v) for v in data["meta"])
    orc, g = _tiny_oracle()
    x = torch.from_numpy(synth.normal(7, "embeds", (B, S, g.d_model), 3.0))
    enc = orc.encode(x)
    keys = sorted(k[: -len("_ids")] for k in data.files if k.endswith("_ids"))
    assert len(keys) == 36
    for key in keys:
        nb = int(key.split("_")[0][2:])
        n = int(key.split("_")[1][1:])
        lp = float(key.split("_")[2][2:])
        es = {"esFalse": False, "esTrue": True, "esnever": "never"}[key.split("_")[3]]
        want_ids, want_sc = data[key + "_ids"].astype(np.int64), data[key + "_scores"]
        ids, sc, _ = _run(orc, enc, B, nb, L, lp, es, n, g)
        assert ids.shape[0] == want_ids.shape[0], key
        want_sc = want_sc.astype(np.float64)
        for i in range(ids.shape[0]):
            assert _upto_eos(ids[i], g.eos_token_id) == _upto_eos(want_ids[i], g.eos_token_id), (key, i)
            if g.eos_token_id not in want_ids[i].tolist():
                # the one delta: a beam still running at max_length is scored over max_length tokens in 4.34 (hyp.shape[-1],
                # start token included), over max_length - 1 (generated_len) in the recording release
                want_sc[i] *= (L - 1) ** lp / L ** lp
        np.testing.assert_allclose(sc.numpy(), want_sc, rtol=1e-5, atol=1e-6, err_msg=key)


def _run(orc, enc, B, nb, L, lp, es, n, g):
    step = oracle_step(orc, enc, nb, L)
    return beam_search(step, B, nb, g.vocab_size, L, lp, es, n, eos=g.eos_token_id, pad=g.pad_token_id,
                       start=g.decoder_start_token_id)


# ---------------------------------------------------------------------------------------------- hand-built scorer cases
# V = 4: pad 0, EOS 1, tokens 2 and 3; the step returns log-probabilities (log_softmax keeps them up to rounding)
def _table_step(tables, calls):
    def step(tokens, t, beam_idx):
        calls.append(t)
        p = torch.tensor(tables[min(t, len(tables) - 1)], dtype=torch.float64)
        return torch.log(p).float().expand(tokens.shape[0], -1).clone()
    return step


def test_eos_at_rank_nb_or_later_is_ignored_and_negative_length_penalty():
    # t = 0: EOS is the third candidate of beam 0 (rank 2 >= nb = 2): no hypothesis.  With length_penalty = -1 a hypothesis
    # [start] of score log 0.2 would beat both final beams (sum x len), so its absence shows in the output.
    calls = []
    step = _table_step([[0.05, 0.2, 0.4, 0.35], [0.01, 0.01, 0.01, 0.97]], calls)
    ids, sc, _ = beam_search(step, 1, 2, 4, 3, length_penalty=-1.0, num_return_sequences=2)
    assert ids.tolist() == [[0, 2, 3], [0, 3, 3]]               # width = max_length: no EOS appended
    want = [(LN(0.4) + LN(0.97)) * 3, (LN(0.35) + LN(0.97)) * 3]
    np.testing.assert_allclose(sc.numpy(), want, rtol=1e-6)
    assert calls == [0, 1]


@pytest.mark.parametrize("early,steps", [(True, 2), (False, 2), ("never", 6)])
def test_early_stopping_points(early, steps):
    # t = 0: EOS is the best candidate (hypothesis [0]); t = 1: beam 0's EOS again (hypothesis [0, 2]) -> nb = 2 hypotheses.
    # True stops at once; False compares the worst hypothesis log(0.3 * 0.5) / 2 with the best candidate / cur_len = the
    # same value -> done; "never" (length_penalty > 0) divides by max_length = 7 instead -> runs to the end.
    calls = []
    step = _table_step([[0.05, 0.5, 0.3, 0.15]], calls)
    ids, sc, _ = beam_search(step, 1, 2, 4, 7, length_penalty=1.0, early_stopping=early, num_return_sequences=2)
    assert len(calls) == steps
    if early is not True and early != "never":
        assert ids.tolist() == [[0, 1, 0], [0, 2, 1]]             # padded after EOS, EOS appended to the shorter hypothesis
        np.testing.assert_allclose(sc.numpy(), [LN(0.5), (LN(0.3) + LN(0.5)) / 2], rtol=1e-6)


def test_is_done_rules():
    for early, lp, best, cur_len, want in [
            (True, 1.0, -100.0, 2, True),
            (False, 1.0, -2.0, 2, True),          # worst -1.0 >= -2 / 2
            (False, 1.0, -1.9, 2, False),         # worst -1.0 < -0.95
            ("never", 1.0, -2.0, 2, False),       # bound -2 / max_length(10) = -0.2
            ("never", 1.0, -20.0, 2, True),       # -20 / 10 = -2 <= worst
            ("never", -0.5, -2.0, 4, True)]:      # length_penalty <= 0: cur_len: -2 * 2 = -4 <= worst
        h = _Hyps(2, lp, early, 10, [])
        h.add([0, 5], -0.5 * (2 ** lp))           # score -0.5
        assert not h.is_done(best, cur_len)       # fewer than nb hypotheses: never done
        h.add([0, 6], -1.0 * (2 ** lp))           # score -1.0: the worst
        assert h.worst == -1.0
        assert h.is_done(best, cur_len) is want, (early, lp, best, cur_len)


def test_hypotheses_keep_the_best_and_track_the_worst():
    h = _Hyps(2, 0.0, False, 10, [])
    h.add([0], -3.0)
    h.add([0, 2], -1.0)
    assert h.worst == -3.0
    h.add([0, 3], -4.0)                           # not better than the worst: dropped
    assert [s for s, _ in h.beams] == [-3.0, -1.0]
    h.add([0, 4], -2.0)                           # replaces -3.0; the worst is now -2.0
    assert [s for s, _ in h.beams] == [-1.0, -2.0] and h.worst == -2.0


def test_pop_prefers_the_later_hypothesis_among_equal_scores():
    beams = [(-1.0, ["a"]), (-2.0, ["b"]), (-1.0, ["c"])]
    assert [h for _, h in pick_best(beams, 3)] == [["c"], ["a"], ["b"]]


# ---------------------------------------------------------------------------------------------- keywords and the ABI
@pytest.mark.parametrize("kw,match", [
    (dict(num_beams=1), "greedy"), (dict(num_beams=33), "32"), (dict(num_beams=0), "positive"),
    (dict(num_beams=4, num_return_sequences=5), "has to be smaller or equal to `num_beams`"),
    (dict(num_beams=4, num_return_sequences=0), "positive"),
    (dict(num_beams=4, early_stopping="always"), "early_stopping"), (dict(num_beams=4, early_stopping=1.5), "early_stopping"),
    (dict(num_beams=4, length_penalty=math.inf), "length_penalty"), (dict(num_beams=4, length_penalty=math.nan), "length_penalty"),
    (dict(num_beams=2.5), "positive")])
def test_resolve_beam_kwargs_errors(kw, match):
    with pytest.raises(ValueError, match=match):
        resolve_beam_kwargs(**kw)


def test_resolve_beam_kwargs_defaults_and_codes():
    cfg = resolve_beam_kwargs(4)
    assert cfg == BeamConfig(num_beams=4, max_length=20, length_penalty=1.0, early_stopping=False, num_return_sequences=1)
    assert [resolve_beam_kwargs(2, early_stopping=e).early_stopping_code for e in (False, True, "never")] == [0, 1, 2]


def test_beam_params_layout_and_symbol():
    assert C.sizeof(native.BeamParams) == 16
    assert [(n, getattr(native.BeamParams, n).offset) for n, _ in native.BeamParams._fields_] == [
        ("num_beams", 0), ("length_penalty", 4), ("early_stopping", 8), ("num_return_sequences", 12)]
    res, args = native._SIGNATURES["m2m_generate_beam"]
    assert res is C.c_int and len(args) == 7
    header = (Path(__file__).resolve().parents[1] / "include" / "music2midi_amd.h").read_text()
    assert "int m2m_generate_beam(m2m_session* s, int max_length, const m2m_beam_params* p" in header
    if native.library_path().exists():
        assert hasattr(native.load(), "m2m_generate_beam")
