"""GPU parity of the large-chain decode forms at the headline length S = 864: the multi-clip attention (dec_attn_mc_kernel, C = 2 / 4
clips of one head per workgroup, their K/V streams back to back, a clip's last prefetch rounds handed to the next clip that still
walks) and the multi-slice feed-forward (dec_ff_multi_kernel).  Per row both do the first kernels' arithmetic operation for operation,
so every comparison here is exact (ids against HuggingFace's, or torch.equal against the C = 1 path) except the existing bf16 bars.

The forms named in the docstrings follow today's policy (csrc/decode.hip decode_attn_clips / decode_ff_slices, csrc/t5_api.hip
plan_groups): C = 2 from 32 clips per chain, C = 4 from 48; 2 hidden slices from 32, 4 from 56; two chains from 24 clips; the forced
step mode decodes the whole batch as one chain.  A policy change has to edit them."""
import numpy as np
import pytest
import torch

from music2midi_amd import synth
from music2midi_amd.checkpoint import load_t5_state
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry
from music2midi_amd.transformer import T5Transformer

from test_golden_gpu import _bf16_divergence, _bf16_noise_margin
from test_t5_gpu import build, embeds

pytestmark = pytest.mark.gpu

GEOM = T5Geometry(DEFAULT_CONFIG["model"]["t5"])

# (B, M2M_GROUP_ROWS) tiles of the two golden clips; None = the default two chains
TILES = [(64, None), (66, None), (96, None), (98, None), (126, None), (128, "128")]


def _ends(ids, eos_id):
    """First EOS position per row (the output length when a row never ends)."""
    return [int(np.nonzero(r == eos_id)[0][0]) if (r == eos_id).any() else ids.shape[1] for r in ids]


def _tiled_runs(monkeypatch, model, x2):
    out = {}
    for B, rows in TILES:
        if rows is None:
            monkeypatch.delenv("M2M_GROUP_ROWS", raising=False)
        else:
            monkeypatch.setenv("M2M_GROUP_ROWS", rows)
        out[B] = model.generate_from_embeds(x2.repeat(B // 2, 1, 1).contiguous(), max_length=1024).cpu().numpy()
    monkeypatch.delenv("M2M_GROUP_ROWS", raising=False)
    return out


def test_fp32_greedy_golden_tiles_reach_every_large_chain_form(monkeypatch, golden_dir):
    """fp32 greedy ids of the golden `full_s864` clips tiled into large batches: every row must be HuggingFace's over all 1 024 tokens.
    Forms reached (two default chains unless noted): B = 64: 2 x 32 clips, C = 2, no tail, 2 FF slices; B = 66: 2 x 33, C = 2, a 1-clip
    tail workgroup, 2 slices; B = 96: 2 x 48, C = 4, no tail, 2 slices; B = 98: 2 x 49, C = 4, 1-clip tail, 2 slices; B = 126: 2 x 63,
    C = 4, 3-clip tail, 4 slices; B = 128 with M2M_GROUP_ROWS=128: one chain, C = 4, 32 workgroups per head, 4 slices.  At these sizes
    only 0 - 2 of the 6 layers' cross K/V fit the 180 MB resident budget: non-temporal and resident layers are mixed.  Clip 0 of the
    pair emits EOS at step 187 and clip 1 never does, so for the remaining 836 steps every other clip of a workgroup is finished: the
    walking clips' streams are handed over across a finished one (C = 4), and a workgroup's first walking clip is not its first clip."""
    z = np.load(golden_dir / "t5.npz")
    want = z["full_s864/ids"].astype(np.int64)
    assert want.shape == (2, 1024)
    model, _, g = build(DEFAULT_CONFIG, "fp32")
    x2 = embeds(2, 864, g.d_model).cuda()
    for B, ids in _tiled_runs(monkeypatch, model, x2).items():
        assert ids.shape == (B, 1024), (B, ids.shape)
        for r in range(B):
            if not np.array_equal(ids[r], want[r % 2]):
                t = int(np.nonzero(ids[r] != want[r % 2])[0][0])
                pytest.fail(f"B = {B}: row {r} leaves HF's ids at step {t} (oracle margin {z['full_s864/margins'][r % 2, t - 1]:.5f})")


def test_bf16_greedy_golden_tiles_are_batch_invariant_and_track_the_emulation(monkeypatch, golden_dir):
    """bf16 greedy ids of the `full_s864` clips in the same tiles as the fp32 test (C = 2 at B = 64 / 66, C = 4 at 96 / 98 / 126 / 128;
    tails of 1, 1 and 3 clips at B = 66 / 98 / 126; one chain of 128 with M2M_GROUP_ROWS=128).  Every copy bit-identical to copy 0;
    copy 0 bit-identical to a B = 2 run of the same clips (one chain, C = 1, one FF slice, temporal K/V loads: the same per-row
    arithmetic); copy 0 within the bf16 noise margin of the bf16-emulating oracle (tests/golden/t5_forced.npz full_s864_bf16)."""
    z = np.load(golden_dir / "t5_forced.npz")
    model, _, g = build(DEFAULT_CONFIG, "bf16")
    x2 = embeds(2, 864, g.d_model).cuda()
    small = model.generate_from_embeds(x2, max_length=1024).cpu().numpy()
    for B, ids in _tiled_runs(monkeypatch, model, x2).items():
        assert ids.shape[0] == B
        for c in range(1, B // 2):
            assert np.array_equal(ids[2 * c: 2 * c + 2], ids[:2]), f"B = {B}: copy {c} decodes differently from copy 0"
        assert ids.shape == (B, small.shape[1]) and np.array_equal(ids[:2], small), f"B = {B}: copy 0 differs from the B = 2 run"
    want = z["full_s864_bf16/ids"].astype(np.int64)
    got = np.pad(small, ((0, 0), (0, 1024 - small.shape[1])), constant_values=g.pad_token_id)
    rows = _bf16_divergence(got, want, z["full_s864_bf16/margins"], "full_s864_bf16 tiles", _bf16_noise_margin(golden_dir, "full_s864_bf16"))
    assert all(t < 0 or t >= 4 for _, t, _ in rows)


@pytest.mark.parametrize("copies", [24, 49])
@pytest.mark.parametrize("case,precision", [("full_s864_fp32", "fp32"), ("full_s864_bf16", "bf16")])
def test_forced_check_at_four_clips_per_workgroup(golden_dir, case, precision, copies):
    """The every-position forced check (tests/forced_check.py) of the S = 864 case through the KV-cached decode kernels on one chain of
    2 x copies clips: copies = 24 -> B = 48: C = 4, no tail, 2 FF slices; copies = 49 -> B = 98: C = 4, a 2-clip tail workgroup,
    4 FF slices.  (The headline check at B = 32 reaches C = 2 only.)"""
    from forced_check import case_inputs, forced_check
    sd, x = case_inputs(case, GEOM, "cuda")
    m = T5Transformer(DEFAULT_CONFIG, precision=precision)
    load_t5_state(m, sd, strict=False)
    m = m.cuda().eval()
    rec = forced_check(m, x, case, precision, copies=copies, mode="step", z=np.load(golden_dir / "t5_forced.npz"))
    print(f"[forced {case} step, B = {2 * copies}] {rec}")
    assert rec["positions"] == 2 * 1023
    assert rec["argmax_asserted_positions"] >= 0.8 * rec["positions"]


def test_bf16_against_the_fp32_reference_at_four_clips_per_workgroup(golden_dir):
    """forced_bf16_vs_fp32 (fixed absolute bars against the fp32 oracle) on one chain of 98 clips: C = 4, a 2-clip tail, 4 FF slices."""
    from forced_check import case_inputs, forced_bf16_vs_fp32
    sd, x = case_inputs("full_s864_fp32", GEOM, "cuda")
    m = T5Transformer(DEFAULT_CONFIG, precision="bf16")
    load_t5_state(m, sd, strict=False)
    m = m.cuda().eval()
    rec = forced_bf16_vs_fp32(m, x, "full_s864_fp32", copies=49, z=np.load(golden_dir / "t5_forced.npz"))
    print(f"[bf16 vs fp32 oracle, full_s864_fp32, B = 98] {rec}")
    assert rec["positions"] == 2 * 1023 and rec["argmax_asserted_positions"] >= 0.5 * rec["positions"]


# ------------------------------------------------------------------ ragged EOS at S = 864 on large chains
EOS_SEED, EOS_SCALE = 7, 1.3
RAGGED_B, RAGGED_LD = 98, 320
# (M2M_DA_CLIPS, M2M_DEC_FF_ROWS, M2M_DEC_FF_SLICES, M2M_COMPACT, M2M_MC_CIF)
RAGGED_BASE = ("1", "8", "1", "1", None)
RAGGED_LEGS = [RAGGED_BASE, ("0", "0", "0", "1", None), ("2", "8", "2", "1", None), ("4", "16", "4", "1", None),
               ("4", "8", "1", "0", None), ("4", "8", "4", "1", "2")]


def _hand_over_holes(ends, nb_chain, C, gap):
    """(e, i, l) clip triples of one C-clip workgroup (fixed slots, two chains of nb_chain) where clip i ends >= gap steps before both
    the earlier clip e and the later clip l: for that long, e's stream hands its last rounds over clip i to l."""
    out = []
    for c0 in range(0, len(ends), nb_chain):
        for b0 in range(c0, c0 + nb_chain, C):
            grp = list(range(b0, min(b0 + C, c0 + nb_chain)))
            for k, i in enumerate(grp):
                for e in grp[:k]:
                    for l in grp[k + 1:]:
                        if ends[i] + gap <= min(ends[e], ends[l]):
                            out.append((e, i, l))
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ragged_eos_on_large_chains_every_form_is_bit_identical(monkeypatch, precision):
    """98 clips at S = 864 whose rows end raggedly (synth.force_eos_head, active = 340), decoded greedily to 1 024 tokens with the
    finished-row skip on.  eos_scale 1.3 was picked from the oracle's EOS spread at 1.3 - 2.0 (the S <= 864 tests' 1.6 leaves 3 holes):
    on MI355X, fp32 (= the oracle, rows 0 - 15 and 28 - 31 checked on the CPU) ends 75 rows at 28 distinct steps, 17 of them in
    127 .. 889 (the latest 938), 47 at step 4, 23 rows run to 1 024 tokens, 9 hand-over holes; bf16 ends 80 rows at 31 distinct steps,
    20 in 123 .. 891, 10 holes.  Default form: two
    chains of 49 = C = 4 with a 1-clip tail workgroup, 2 FF slices; cross streams of 7 (bf16, padded to 8) / 14 (fp32) rounds, longer
    than the 2-round prefetch window, so a clip re-requests inside its stream and hands over across finished clips.  Legs, each a
    session of its own (M2M_DA_CLIPS, M2M_DEC_FF_ROWS, M2M_DEC_FF_SLICES): 1,8,1 (the first kernels, the base) / 0,0,0 (policy) /
    2,8,2 / 4,16,4 with live-row re-packing; 4,8,1 with M2M_COMPACT=0 (fixed slots: the holes below are known); 4,8,4 with
    M2M_MC_CIF=2 (two clips in flight).  Greedy ids and teacher-forced step logits along the base ids (Ld = 320: the self stream
    re-requests too) must be torch.equal across legs; fp32 ids equal the oracle's on the rows of a hand-over hole and the tail clips."""
    geom = GEOM
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    synth.force_eos_head(sd, geom, active=340, eos_scale=EOS_SCALE)
    x = embeds(RAGGED_B, 864, geom.d_model, seed=EOS_SEED)
    xd = x.cuda()
    ids, logits, stats = {}, {}, {}
    for leg in RAGGED_LEGS:
        for k, v in zip(("M2M_DA_CLIPS", "M2M_DEC_FF_ROWS", "M2M_DEC_FF_SLICES", "M2M_COMPACT", "M2M_MC_CIF"), leg):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
        monkeypatch.delenv("M2M_FORWARD", raising=False)
        m = T5Transformer(DEFAULT_CONFIG, precision=precision)       # the switches are latched when its session is created
        load_t5_state(m, sd, strict=False)
        m = m.cuda().eval()
        ids[leg] = m.generate_from_embeds(xd, max_length=1024).cpu()
        stats[leg] = m.repack_stats()
        monkeypatch.setenv("M2M_FORWARD", "step")
        logits[leg] = m.logits_from_embeds(xd, ids[RAGGED_BASE][:, :RAGGED_LD].cuda()).cpu()
        monkeypatch.delenv("M2M_FORWARD", raising=False)
        del m
    base = ids[RAGGED_BASE]
    ends = _ends(base.numpy(), geom.eos_token_id)
    holes = _hand_over_holes(ends, RAGGED_B // 2, 4, 256)
    print(f"ragged EOS {precision} B = {RAGGED_B} S = 864: output length {base.shape[1]}, EOS positions {sorted(ends)}, "
          f"re-packings {stats}, hand-over holes (earlier, finished, later clip) {holes[:8]}")
    assert base.shape[1] >= RAGGED_LD
    for leg in RAGGED_LEGS:
        assert torch.equal(ids[leg], base), f"ids differ in leg {leg}"
        assert torch.equal(logits[leg], logits[RAGGED_BASE]), f"step logits differ in leg {leg}"
        if leg[3] == "1":
            assert stats[leg][0] >= 1, f"leg {leg} did not re-pack"
        else:
            assert stats[leg] == (0, 0)
    # the case must bite: ragged ends over the whole length, and a long hole between walking clips of one C = 4 workgroup
    assert len({e for e in ends if 100 <= e <= 900}) >= 10 and min(ends) <= 10 and max(e for e in ends if e < base.shape[1]) >= 800, sorted(ends)
    assert holes
    if precision == "fp32":
        from oracle.t5 import T5Oracle
        rows = sorted(set(holes[0]) | {RAGGED_B // 2 - 1, RAGGED_B - 1})     # a hole's three clips and the two 1-clip tails
        want = T5Oracle(geom, sd).generate(x[rows], 1024)
        n = want.shape[1]
        assert torch.equal(base[rows, :n], want) and (base[rows, n:] == geom.pad_token_id).all(), rows
