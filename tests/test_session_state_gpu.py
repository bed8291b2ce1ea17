"""Session state of the C ABI around live-row re-packing (VERDICT r5 weak #3 / ADVICE r5), THROUGH ctypes.

HF's forward and generate share one encoder pass (ref: music2midi/transformer.py:28-45), and include/music2midi_amd.h allows
m2m_encode -> any number of m2m_generate_greedy / m2m_decode_forced / m2m_bench_kernel calls.  Re-packing the live rows moves
clips over finished ones, so a greedy decode that moved rows CONSUMES the encode: the next call must say so (M2M_ERR_STATE,
"re-encode") instead of decoding permuted clips, and after a new m2m_encode everything must equal the oracle again.
"""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from music2midi_amd import native, synth
from music2midi_amd.checkpoint import load_t5_state
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config
from music2midi_amd.transformer import T5Transformer

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
M2M_ERR_STATE = -4


def _model(precision, eos):
    geom = T5Geometry(load_config(DEFAULT_CONFIG).model.t5)
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    if eos:
        synth.force_eos_head(sd, geom, active=340, eos_scale=1.6)
    m = T5Transformer(DEFAULT_CONFIG, precision=precision)
    load_t5_state(m, sd, strict=False)
    return m.cuda().eval(), geom, sd


def _oracle_logits(orc, x, dec_in):
    """teacher-forced logits of the oracle for explicit decoder inputs (column 0 = the start token): its forward() takes labels and
    shifts them right, so hand it the inputs shifted left (the last label only enters the loss)"""
    labels = torch.cat([dec_in[:, 1:], torch.zeros_like(dec_in[:, :1])], dim=1)
    return orc.forward(x, labels)[1]


def _generate(lib, sess, B, L, dev):
    tokens = torch.empty((B, L), dtype=torch.long, device=dev)
    n = C.c_int(0)
    rc = lib.m2m_generate_greedy(sess, L, tokens.data_ptr(), C.byref(n), native.stream_handle(dev))
    return rc, tokens[:, : max(n.value, 1)].cpu()


def _forced(lib, sess, ids, V, dev):
    B, Ld = ids.shape
    logits = torch.empty((B, Ld, V), dtype=torch.float32, device=dev)
    ids_dev = ids.to(dev).contiguous()
    rc = lib.m2m_decode_forced(sess, ids_dev.data_ptr(), Ld, logits.data_ptr(), native.stream_handle(dev))
    torch.cuda.synchronize(dev)
    return rc, logits.cpu()


def _stats(lib, sess):
    a, b = C.c_int(0), C.c_int(0)
    assert lib.m2m_session_repack_stats(sess, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


@pytest.mark.parametrize("mode", ["batched", "step"])
def test_generate_that_moved_rows_consumes_the_encode(monkeypatch, mode):
    from oracle.t5 import T5Oracle
    monkeypatch.setenv("M2M_FORWARD", mode)
    monkeypatch.setenv("M2M_COMPACT", "1")
    B, S, L, Ld = 9, 61, 400, 48
    m, geom, sd = _model("fp32", eos=True)
    x = torch.from_numpy(synth.normal(21, "embeds", (B, S, geom.d_model), 3.0))
    orc = T5Oracle(geom, sd)
    want_ids = orc.generate(x, L)
    dec_in = want_ids[:, :Ld].contiguous()
    assert want_ids.shape[1] >= Ld
    want_logits = _oracle_logits(orc, x, dec_in)
    lib = native.load()
    dev = m.transformer.device
    xd = x.to(dev).contiguous()
    with torch.cuda.device(dev):
        sess, _ = m._encode(xd, L)
        rc, ids = _generate(lib, sess, B, L, dev)
        assert rc == 0 and torch.equal(ids, want_ids)
        repacks, moved = _stats(lib, sess)
        print(f"state hole ({mode}): {repacks} re-packings, {moved} rows moved")
        assert moved > 0, "the fixture must really move rows"
        # every call that needs the encode now refuses, naming the reason
        rc, _ = _forced(lib, sess, dec_in, geom.vocab_size, dev)
        assert rc == M2M_ERR_STATE and b"re-encode" in lib.m2m_last_error()
        rc, _ = _generate(lib, sess, B, L, dev)
        assert rc == M2M_ERR_STATE and b"re-encode" in lib.m2m_last_error()
        us, nb = C.c_float(0), C.c_int64(0)
        rc = lib.m2m_bench_kernel(sess, native.KERNEL_DEC_CROSS_ATTN, 8, 2, C.byref(us), C.byref(nb), native.stream_handle(dev))
        assert rc == M2M_ERR_STATE and b"re-encode" in lib.m2m_last_error()
        # a new encode restores the contract: forced logits == oracle, then a second generate on the SAME encode == oracle
        # is refused only if the first one moved rows again
        sess, _ = m._encode(xd, L)
        rc, logits = _forced(lib, sess, dec_in, geom.vocab_size, dev)
        assert rc == 0
        err = (logits - want_logits).abs().max().item()
        print(f"forced logits after re-encode: max|diff| {err:.2e}")
        assert err < 2e-3
        rc, ids2 = _generate(lib, sess, B, L, dev)       # forced -> generate on one encode: legal, the forced pass moves nothing
        assert rc == 0 and torch.equal(ids2, want_ids)


def test_encode_is_shared_when_no_row_moves(monkeypatch):
    """Without EOS nothing is re-packed: generate -> forced -> generate on ONE encode, as the header allows."""
    from oracle.t5 import T5Oracle
    monkeypatch.setenv("M2M_FORWARD", "step")
    B, S, L = 5, 40, 40
    m, geom, sd = _model("fp32", eos=False)
    x = torch.from_numpy(synth.normal(5, "embeds", (B, S, geom.d_model), 3.0))
    orc = T5Oracle(geom, sd)
    want_ids = orc.generate(x, L)
    want_logits = _oracle_logits(orc, x, want_ids)
    lib = native.load()
    dev = m.transformer.device
    with torch.cuda.device(dev):
        sess, _ = m._encode(x.to(dev).contiguous(), L)
        rc, ids = _generate(lib, sess, B, L, dev)
        assert rc == 0 and torch.equal(ids, want_ids) and _stats(lib, sess)[1] == 0
        rc, logits = _forced(lib, sess, want_ids, geom.vocab_size, dev)
        assert rc == 0 and (logits - want_logits).abs().max().item() < 2e-3
        rc, ids2 = _generate(lib, sess, B, L, dev)
        assert rc == 0 and torch.equal(ids2, want_ids)


_CHILD = r"""
import sys, torch
torch.set_num_threads(min(16, torch.get_num_threads()))     # the oracle's matmuls are tiny: 256 visible cores only cost fan-out (tests/conftest.py)
sys.path.insert(0, %r)
from music2midi_amd import synth
from music2midi_amd.checkpoint import load_t5_state
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry, load_config
from music2midi_amd.transformer import T5Transformer
from oracle.t5 import T5Oracle
import os
geom = T5Geometry(load_config(DEFAULT_CONFIG).model.t5)
sd = synth.t5_state_dict(geom, seed=0); synth.perturb_layer_norms(sd, 0); synth.force_eos_head(sd, geom, active=340, eos_scale=1.6)
m = T5Transformer(DEFAULT_CONFIG, precision="fp32"); load_t5_state(m, sd, strict=False); m = m.cuda().eval()
big, B, S, L = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
if big > B:
    m._get_session(big, S, L)            # a session sized ABOVE the encoded batch: self-cache strides come from max_batch
x = torch.from_numpy(synth.normal(21, "embeds", (B, S, geom.d_model), 3.0))
os.environ["M2M_COMPACT"] = "1"
on = m.generate_from_embeds(x.cuda(), max_length=L).cpu()
stats = m.repack_stats()
os.environ["M2M_COMPACT"] = "0"
off = m.generate_from_embeds(x.cuda(), max_length=L).cpu()
ref = T5Oracle(geom, sd).generate(x, L)
print("STATS", stats[0], stats[1], int(torch.equal(on, off)), int(torch.equal(on, ref)))
""" % str(ROOT)


@pytest.mark.parametrize("big,B,S,L,headless", [(33, 9, 61, 140, "1"), (9, 9, 61, 140, "0"), (40, 17, 30, 140, "0")])
def test_repacking_on_a_larger_session_and_with_the_head_kernel(big, B, S, L, headless):
    """decode_move_rows takes the self-cache layer stride from max_batch and the cross plane stride from the encoded B —
    covered here with a session created larger than the batch it decodes (encode B = 9 on a 33-clip session), and the re-packing
    path with dec_head_kernel kept in the loop (M2M_HEADLESS=0 is latched when a session is created; set for a child process), where the moved residual
    row is what the next step reads."""
    env = dict(os.environ, M2M_HEADLESS=headless)
    env.pop("M2M_COMPACT", None)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(big), str(B), str(S), str(L)], env=env, capture_output=True, text=True, timeout=900)
    line = [l for l in r.stdout.splitlines() if l.startswith("STATS")]
    assert r.returncode == 0 and line, r.stdout[-2000:] + r.stderr[-3000:]
    repacks, moved, same, ref = (int(v) for v in line[-1].split()[1:])
    print(f"session {big} >= batch {B}, M2M_HEADLESS={headless}: {repacks} re-packings, {moved} rows moved")
    assert repacks >= 1 and moved >= 1 and same == 1 and ref == 1


_RANGED = ("M2M_DA_CLIPS", "M2M_DEC_FF_ROWS", "M2M_DEC_FF_SLICES", "M2M_MC_CIF")


@pytest.fixture(scope="module")
def small_greedy():
    """inputs [2, 8, d] and their greedy ids (max_length 8) from a model built with none of the ranged switches set"""
    saved = {k: os.environ.pop(k) for k in _RANGED if k in os.environ}
    try:
        m, geom, _ = _model("fp32", eos=False)
        x = torch.from_numpy(synth.normal(5, "embeds", (2, 8, geom.d_model), 3.0)).cuda()
        return x, m.generate_from_embeds(x, max_length=8).cpu()
    finally:
        os.environ.update(saved)


@pytest.mark.parametrize("switch,value", [("M2M_DA_CLIPS", "3"), ("M2M_DEC_FF_ROWS", "4"), ("M2M_DEC_FF_SLICES", "3"), ("M2M_MC_CIF", "5")])
def test_a_switch_outside_its_range_refuses_the_session(monkeypatch, small_greedy, switch, value):
    """m2m_session_create latches the decode switches and refuses a value outside a switch's range by name; nothing of the refused
    session is left behind: with the variable removed the same model creates its session and decodes as one that never saw it."""
    x, want = small_greedy
    for k in _RANGED:
        monkeypatch.delenv(k, raising=False)
    m, _, _ = _model("fp32", eos=False)
    monkeypatch.setenv(switch, value)
    with pytest.raises(native.NativeError) as err:
        m.generate_from_embeds(x, max_length=8)
    assert "m2m_session_create" in str(err.value) and f"{switch}={value}" in str(err.value), str(err.value)
    monkeypatch.delenv(switch)
    assert torch.equal(m.generate_from_embeds(x, max_length=8).cpu(), want)
