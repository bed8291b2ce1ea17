"""The decoder's layer-0 input row is emb[tok] and nothing else, so the layer-0 self-attention's q (fp32) and k, v (rounded to the
storage type) of a head are functions of the token id alone.  m2m_model_create writes them once into three tables of the model
(t5.h m2m_model::q0_tab / k0_tab / v0_tab, decode.hip dec_token_tables_kernel: the step kernel's own norm and da_project), and the
one-clip layer-0 self-attention of the headless greedy step takes them from there (M2M_DEC_TOKEN_TABLES, latched per session: 0
projects and streams the cache, 1 takes this step's q, k, v from the tables, 2 also reads the cached K/V rows from the tables,
addressed by the row's token history).

The greedy ids of every leg are torch.equal with the form switched off, a new model per leg: a table entry has the bits the step
would have produced.  The off leg is held to the oracle by the bars of tests/test_dec_row_stage_gpu.py.  Lengths enter the main
loop of the K/V stream (it starts past (2 PF - 1) KPB keys: 384 in bf16, 192 in fp32); the oracle comparison stops at 140 tokens
to bound the CPU time.

What the ids comparison rests on: _has_tables() asserts that the model really holds the tables (its blob is larger by exactly
H x V x 64 x (4 + 2 es) bytes than the tensors without them), and with tables and the switch on, decode_launch_attn takes the form
for every headless one-clip layer-0 launch or refuses the launch (launch_dec_attn's M2M_REQUIRE); the gate test shows the other
side (no tables, blob without them).

NOT a check of the tables: the teacher-forced step logits.  The teacher-forced step does not take the form (DESIGN 4.3, round 9:
it reads its row from the fixed-point stream, whose image of emb[tok] is not emb[tok] where an element is no multiple of 2^-30,
so its q, k, v are not the tables').  Its logits are compared across the legs for one thing only: that the projecting step, run
on a session whose greedy call took the table form just before, reads a layer-0 cache and a session state that the form left as
the parent's kernels leave them."""
import numpy as np
import pytest
import torch

from music2midi_amd import native, synth
from music2midi_amd.checkpoint import load_t5_state
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config
from music2midi_amd.transformer import T5Transformer

from test_geometry_axes_gpu import geom_config

pytestmark = pytest.mark.gpu

S = 8
LONG = {"bf16": 420, "fp32": 210}        # max_length of the on / off comparison
L_ORACLE = 140
LEGS = ("0", "1", "2")
SWITCH = "M2M_DEC_TOKEN_TABLES"


def _weights(cfg, eos_scale=None):
    geom = T5Geometry(load_config(cfg).model.t5)
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    if eos_scale is not None:
        synth.force_eos_head(sd, geom, active=340, eos_scale=eos_scale)
    return geom, sd


def _model(monkeypatch, cfg, sd, precision, leg, **env):
    """a new model, hence a new session: the switches are latched when the session is created"""
    monkeypatch.setenv(SWITCH, leg)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = T5Transformer(cfg, precision=precision)
    load_t5_state(m, sd, strict=False)
    return m.cuda().eval()


def _blob_without_tables(geom, es):
    """bytes of every packed tensor but the token tables: the blob's declarations, each rounded up to 256 bytes
    (t5_api.hip m2m_model_create, carver.h)"""
    d, dff, inner, V = geom.d_model, geom.d_ff, geom.num_heads * geom.d_kv, geom.vocab_size
    off = 0

    def take(nbytes):
        nonlocal off
        off = (off + nbytes + 255) // 256 * 256

    for _ in range(geom.num_layers):
        for n in (d * 4, 3 * inner * d * es, d * inner * es, d * 4, 2 * dff * d * es, d * dff * es):
            take(n)
    for _ in range(geom.num_decoder_layers):
        for n in (d * 4, 3 * inner * d * es, d * inner * es, d * 4, inner * d * es, d * inner * es, d * 4, 2 * dff * d * es,
                  d * dff * es, 3 * dff * d * es, d * inner * es, d * inner * es):
            take(n)
    for n in (d * 4, d * 4, V * d * 4, (V + 15) // 16 * 16 * d * es, geom.num_decoder_layers * 2 * inner * d * es):
        take(n)
    return off


def _has_tables(m, geom, precision):
    """(bytes of the model's blob, bytes of the same tensors without the three tables, bytes of the tables)"""
    es = 2 if precision == "bf16" else 4
    nbytes = int(native.load().m2m_model_param_bytes(m._get_model()))
    elems = geom.num_heads * geom.vocab_size * 64
    tables = sum((elems * b + 255) // 256 * 256 for b in (4, es, es))
    return nbytes, _blob_without_tables(geom, es), tables


def _inputs(geom, B, L, seed=47):
    x = torch.from_numpy(synth.normal(seed, "embeds", (B, S, geom.d_model), 3.0))
    labels = torch.from_numpy((synth.uniform01(9, "labels", B * L) * 330).astype(np.int64).reshape(B, L)) + 3
    dec_in = torch.full_like(labels, geom.decoder_start_token_id)
    dec_in[:, 1:] = labels[:, :-1]
    return x, dec_in


def _hold_to_oracle(geom, sd, precision, x, out, what):
    """the bars of tests/test_dec_row_stage_gpu.py on the first L_ORACLE tokens (without EOS a shorter call's ids are a prefix)"""
    from oracle.t5 import T5Oracle
    ref_ids, margins = T5Oracle(geom, sd, emulate=precision).generate(x, L_ORACLE, return_margins=True)
    n = min(out.shape[1], ref_ids.shape[1])
    assert n == L_ORACLE
    if precision == "fp32":
        assert torch.equal(out[:, :n], ref_ids), f"{what}: fp32 ids differ from the oracle's"
        return
    for b in range(x.shape[0]):
        for t in range(1, n):
            if out[b, t] != ref_ids[b, t]:
                assert margins[b, t - 1] < 0.5, f"{what}: row {b} step {t}: diverged at margin {margins[b, t - 1]:.3f}"
                break


def _legs_equal(monkeypatch, cfg, geom, sd, precision, B, what, session_rows=0, oracle=True):
    L = LONG[precision]
    x, dec_in = _inputs(geom, B, L)
    ids, logits, sizes = {}, {}, set()
    for leg in LEGS:
        m = _model(monkeypatch, cfg, sd, precision, leg)
        nbytes, plain, tables = _has_tables(m, geom, precision)
        assert nbytes == plain + tables, f"{what}: blob {nbytes} bytes, tensors {plain} + tables {tables}: the model holds no tables"
        sizes.add(nbytes)
        if session_rows:
            m._get_session(session_rows, S, L)                 # a session sized above the batch it decodes
        monkeypatch.delenv("M2M_FORWARD", raising=False)
        ids[leg] = m.generate_from_embeds(x.cuda(), max_length=L).cpu()
        monkeypatch.setenv("M2M_FORWARD", "step")              # the same step kernels, teacher-forced
        logits[leg] = m.logits_from_embeds(x.cuda(), dec_in.cuda()).cpu()
        monkeypatch.delenv("M2M_FORWARD", raising=False)
        del m
    assert ids["0"].shape == (B, L)
    for leg in LEGS[1:]:
        assert torch.equal(ids[leg], ids["0"]), f"{what}: ids differ with {SWITCH}={leg}"
        # (not a check of the tables - see the module docstring: the projecting step on a session the table form ran on)
        assert torch.equal(logits[leg], logits["0"]), f"{what}: step logits differ with {SWITCH}={leg}"
    assert len(sizes) == 1                                      # the tables are the model's, whatever the session's switch
    if oracle:
        _hold_to_oracle(geom, sd, precision, x, ids["0"], what)


@pytest.fixture(scope="module")
def default_weights():
    return _weights(DEFAULT_CONFIG)


# B = 1, a partial chain (7), a session larger than its batch (7 and 17 rows in a 33-row session) and two chains (33)
@pytest.mark.parametrize("B,session_rows", [(1, 0), (7, 33), (17, 33), (33, 0)])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_table_legs_equal_the_projecting_step(monkeypatch, default_weights, precision, B, session_rows):
    geom, sd = default_weights
    _legs_equal(monkeypatch, DEFAULT_CONFIG, geom, sd, precision, B, f"default geometry B={B}", session_rows)


# geometries where a wrong table index shows: every d_model beside the default's 384, four heads, a vocabulary that is no multiple of 16
MAPS = {
    "d128": dict(d_model=128),
    "d256": dict(d_model=256),
    "d512": dict(d_model=512),
    "four_heads": dict(d_model=256, d_ff=128, num_heads=4),
    "vocab397": dict(vocab_size=397),
}


@pytest.mark.parametrize("case", sorted(MAPS))
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_table_index_map_at_the_small_geometries(monkeypatch, precision, case):
    cfg = geom_config(**MAPS[case])
    geom, sd = _weights(cfg)
    _legs_equal(monkeypatch, cfg, geom, sd, precision, 9, case)


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_size_gate_t5_vocabulary_has_no_tables(monkeypatch, precision):
    """the default T5 vocabulary: the tables would take 2 heads x 32 128 x 64 x (4 + 2 es) bytes, beyond the 16 MB cap - the model
    has none and the switch changes nothing"""
    cfg = geom_config(vocab_size=32128, d_model=128)
    geom, sd = _weights(cfg)
    x, _ = _inputs(geom, 2, 12)
    out = {}
    for leg in ("0", "2"):
        m = _model(monkeypatch, cfg, sd, precision, leg)
        out[leg] = m.generate_from_embeds(x.cuda(), max_length=12).cpu()
        nbytes, plain, tables = _has_tables(m, geom, precision)
        assert tables > 16 << 20 and nbytes == plain, (nbytes, plain, tables)      # beyond the cap: the blob is the tensors alone
        del m
    assert out["0"].shape == (2, 12) and torch.equal(out["0"], out["2"])


def _eos_columns(ids, eos):
    hit = ids == eos
    return [int(hit[r].float().argmax()) if bool(hit[r].any()) else -1 for r in range(ids.shape[0])]


@pytest.mark.parametrize("precision,B", [("fp32", 9), ("bf16", 32)])
def test_rows_that_end(monkeypatch, precision, B):
    """rows stop at different steps: with live-row re-packing (token rows do not move, tok_row is the indirection), without it and
    with finished rows streaming on - ids equal in all; then a full batch on the same session.  Finished rows are compared by
    their ids only."""
    geom, sd = _weights(DEFAULT_CONFIG, eos_scale=1.6)
    x = torch.from_numpy(synth.normal(21, "embeds", (B, 61, geom.d_model), 3.0))
    x2 = torch.from_numpy(synth.normal(22, "embeds", (B, 61, geom.d_model), 3.0))
    runs = {"repack": {"M2M_COMPACT": "1", "M2M_FINISHED_SKIP": "1"}, "no_repack": {"M2M_COMPACT": "0", "M2M_FINISHED_SKIP": "1"},
            "no_skip": {"M2M_COMPACT": "1", "M2M_FINISHED_SKIP": "0"}}
    want = want2 = None
    for name, env in runs.items():
        for leg in LEGS:
            m = _model(monkeypatch, DEFAULT_CONFIG, sd, precision, leg, **env)
            out = m.generate_from_embeds(x.cuda(), max_length=400).cpu()
            stats = m.repack_stats()
            out2 = m.generate_from_embeds(x2.cuda(), max_length=400).cpu()     # the same session, every slot live again
            del m
            if want is None:
                want, want2 = out, out2
                assert len(set(_eos_columns(out, geom.eos_token_id))) > 2            # rows end at different steps
            if name == "repack":
                assert stats[0] >= 1 and stats[1] >= 1, stats                        # rows really moved
            assert out.shape == want.shape and torch.equal(out, want), (name, leg)
            assert out2.shape == want2.shape and torch.equal(out2, want2), (name, leg)


def test_other_head_forms_read_the_cache_the_table_form_appends(monkeypatch, default_weights):
    """sampled, processed, scored, beam and two clips per workgroup on a session with tables, each behind a greedy call of the
    table form on the same session: equal to the leg without"""
    geom, sd = default_weights
    x, _ = _inputs(geom, 5, 40)
    got = {}
    for leg in ("0", "2"):
        m = _model(monkeypatch, DEFAULT_CONFIG, sd, "fp32", leg)
        r = {"greedy": m.generate_from_embeds(x.cuda(), max_length=40).cpu()}
        torch.manual_seed(5)
        r["sampled"] = m.generate_from_embeds(x.cuda(), max_length=40, do_sample=True, top_k=8).cpu()
        r["processed"] = m.generate_from_embeds(x.cuda(), max_length=40, repetition_penalty=1.3).cpu()
        sc = m.generate_from_embeds(x.cuda(), max_length=40, return_dict_in_generate=True, output_scores=True)
        r["scored"], r["scores"] = sc.sequences.cpu(), torch.stack(sc.scores).cpu()
        r["beam"] = m.beam_search_from_embeds(x.cuda(), 2, max_length=40).cpu()
        r["greedy_again"] = m.generate_from_embeds(x.cuda(), max_length=40).cpu()
        del m
        m = _model(monkeypatch, DEFAULT_CONFIG, sd, "fp32", leg, M2M_DA_CLIPS="2")
        r["two_clips"] = m.generate_from_embeds(x.cuda(), max_length=40).cpu()
        del m
        got[leg] = r
    for k, v in got["0"].items():
        assert torch.equal(got["2"][k], v), k
    assert torch.equal(got["2"]["greedy_again"], got["2"]["greedy"]) and torch.equal(got["2"]["two_clips"], got["2"]["greedy"])


def test_switch_outside_its_range_refuses_the_session(monkeypatch, default_weights):
    geom, sd = default_weights
    m = _model(monkeypatch, DEFAULT_CONFIG, sd, "fp32", "3")
    x, _ = _inputs(geom, 1, 4)
    with pytest.raises(native.NativeError, match=SWITCH):
        m.generate_from_embeds(x.cuda(), max_length=4)
