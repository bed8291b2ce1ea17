"""GPU: the log-mel frontend (csrc/frontend.hip) across the geometry the config allows, held to the CPU oracle.

The case table (tests/frontend_cases.py) varies sample rate, f_min, n_mels, hop and T so that both instantiations of the second
form meet partial filter groups, the first form runs at FR 16 / 12 / 8 / 4, the v2 LDS gate is crossed at hop 272, and 48-bin and
empty filters occur.  Every case asserts the form m2m_frontend_plan reports and is held to the oracle with tests/logmel_check.py's
unchanged bars.  Then exact invariances (batch width, chunks per workgroup, FR, output placement), the launch limits, > 2^31
indices, a filterbank loaded from a state dict (the taps-in-memory instantiation), the refusals, and NaN / Inf propagation.
"""

import numpy as np
import pytest
import torch

import frontend_cases as fc
from logmel_check import FLOOR, check_logmel
from music2midi_amd import native, synth
from music2midi_amd.input import LogMelSpectrogram, ModelInputs

pytestmark = pytest.mark.gpu


def _oracle(sr, hop, f_min, n_mels):
    from oracle.logmel import LogMelOracle
    return LogMelOracle(sr, 2048, hop, f_min, n_mels)


def _wave(kind, B, T, first=0, orc=None):
    """synth clips; "quiet" is noise scaled so that the median float64 mel power is 1e-6 (the clamp splits the bins)."""
    if kind != "quiet":
        return torch.from_numpy(synth.waveform_batch(first, B, T, kind))
    w = torch.from_numpy(synth.waveform_batch(first, B, T, "noise"))
    mel = torch.matmul(orc.power_spectrogram(w, torch.float64).transpose(-1, -2), orc.fb.double())
    return (w.double() * (1e-6 / mel.median()).sqrt()).float()


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _plan_matches(fe, B, T, **want):
    p = fe.plan(B, T)
    for k, v in want.items():
        assert p[k] == v, (k, p)
    return p


# ---------------------------------------------------------------------------------------------------- the case table
def _run_case(c):
    """-> (device log-mel, waveform, oracle) of a table case, after asserting the plan the device makes for it."""
    fe = LogMelSpectrogram(c.sr, 2048, c.hop, c.f_min, c.n_mels)
    p = fe.plan(c.B, c.T)
    assert p == dict(fc.case_plan(c, n_cu=_n_cu()), lds_bytes=p["lds_bytes"]), p
    assert (p["form"], p["frames_per_chunk"]) == (c.form, c.fr)
    orc = _oracle(c.sr, c.hop, c.f_min, c.n_mels)
    wav = _wave(c.kind, c.B, c.T, first=c.first if c.first >= 0 else c.n_mels, orc=orc)
    out = fe(wav.cuda()).cpu()
    assert out.shape == (c.B, 1 + c.T // c.hop, c.n_mels)
    return out, wav, orc


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.id)
def test_geometry_case_matches_oracle(case):
    c = case
    out, wav, orc = _run_case(c)
    check_logmel(out, wav, orc, c.id)
    _, width = fc.taps(fc.filterbank(c.sr, c.f_min, c.n_mels))
    empty = torch.from_numpy(np.nonzero(width == 0)[0])
    if len(empty):     # an empty filter is log(float32(1e-6)) on every frame, as the oracle's dense matmul gives
        assert torch.all(out[:, :, empty] == FLOOR) and torch.all(orc(wav)[:, :, empty] == FLOOR)
    if c.kind == "zeros":
        assert torch.all(out == FLOOR)
    if c.kind == "quiet":
        mel = torch.matmul(orc.power_spectrogram(wav, torch.float64).transpose(-1, -2), orc.fb.double())
        below = float((mel < 1e-6).double().mean())
        assert 0.2 < below < 0.8, below


class Fp32NoiseMiss(AssertionError):
    pass


@pytest.mark.parametrize("case,measured", [
    pytest.param(c, m, id=c.id, marks=pytest.mark.xfail(strict=True, raises=Fp32NoiseMiss, reason=f"fp32 noise: {m}"))
    for c, m in fc.FP32_NOISE_MISSES])
def test_known_fp32_noise_misses_of_the_1e4_bar(case, measured):
    """Music / tone inputs on which the kernel's fp32 FFT noise takes a bin 55-59 dB under its frame's peak past the 1e-4 bar
    (tests/frontend_cases.py FP32_NOISE_MISSES).  Strict: if the kernel becomes accurate enough the case passes and
    this test fails, and the entry goes.  Everything else asserted here (the plan, the noise-model bound, the class percentiles) must
    hold; only the well-conditioned 1e-4 assertion may fail, and the worst bin's level is printed."""
    from logmel_check import TOL, classify
    c = case
    out, wav, orc = _run_case(c)
    l64, well, _ = classify(orc, wav)
    mel64 = torch.matmul(orc.power_spectrogram(wav, torch.float64).transpose(-1, -2), orc.fb.double())
    db = 10 * torch.log10(mel64 / mel64.amax(-1, keepdim=True))
    err = torch.maximum((out.double() - l64).abs(), (out.double() - orc(wav).double()).abs())
    err[~well] = 0
    i = int(err.flatten().argmax())
    print(f"[{c.id}] worst well-conditioned bin: error {float(err.flatten()[i]):.3e}, {float(db.flatten()[i]):.1f} dB under its frame's "
          f"peak (recorded: {measured})")
    assert float(err.max()) < 2 * TOL, "beyond the recorded fp32 noise: a real error"
    try:
        check_logmel(out, wav, orc, c.id)
    except AssertionError as e:
        if "well-conditioned bin off by" not in str(e):
            raise
        raise Fp32NoiseMiss(str(e)) from e


@pytest.mark.parametrize("hop,form", [(256, "v2_nj6"), (512, "v1_taps_lds")])
@pytest.mark.parametrize("k", [31, 32])
def test_lengths_at_the_frame_edges(hop, form, k):
    """T = 1 025 (the shortest accepted), 1 026, 2 047 .. 2 049 and k hop - 1 / k hop / k hop + 1 (frame counts 31, 32, 33:
    F % 16 = 15, 0, 1) in one form each, all clips of one length in one call.  Noise clips: music at two of these lengths is in
    fc.FP32_NOISE_MISSES."""
    fe = LogMelSpectrogram(16000, 2048, hop, 20.0, 384)
    orc = _oracle(16000, hop, 20.0, 384)
    lengths = [k * hop - 1, k * hop, k * hop + 1] + ([1025, 1026, 2047, 2048, 2049] if k == 31 else [])
    for T in lengths:
        _plan_matches(fe, 2, T, form=form)
        wav = _wave("noise", 2, T, first=T)
        check_logmel(fe(wav.cuda()).cpu(), wav, orc, f"hop {hop} T {T}")


# ---------------------------------------------------------------------------------------------------- exact invariances
def _tiled(base, B):
    return base[torch.arange(B, device=base.device) % base.shape[0]].contiguous()


def _assert_rows_tile(out, ref):
    idx = torch.arange(out.shape[0], device=out.device) % ref.shape[0]
    for s in range(0, out.shape[0], 4096):
        assert torch.equal(out[s:s + 4096], ref[idx[s:s + 4096]]), f"rows {s}.."


@pytest.mark.parametrize("hop,form", [(256, "v2_nj6"), (512, "v1_taps_lds")])
def test_batch_width_invariance(hop, form):
    """A clip's rows do not depend on the batch: 1 to 1 000 clips (one workgroup per clip walks every chunk once B passes the CU
    count in the second form; two chunks per workgroup by default in the first form from B = 256 here)."""
    fe = LogMelSpectrogram(16000, 2048, hop, 20.0, 384)
    base = _wave("music", 3, 48000, first=7).cuda()
    ref = fe(base)
    F = ref.shape[1]
    for B in (1, 3, 255, 256, 257, 1000):
        p = _plan_matches(fe, B, 48000, form=form)
        if form.startswith("v2") and B >= 257:
            assert (p["grid_x"], p["chunks"]) == (1, -(-F // 16))
        if form.startswith("v1"):
            assert p["chunks"] == (2 if -(-F // (2 * p["frames_per_chunk"])) * B >= 1536 else 1)
            assert p["chunks"] == (2 if B >= 256 else 1)
        _assert_rows_tile(fe(_tiled(base, B)), ref)


@pytest.mark.parametrize("hop,form", [(256, "v2_nj6"), (160, "v2_nj8"), (512, "v1_taps_lds"), (1024, "v1_taps_lds")])
def test_chunks_per_workgroup_invariance(monkeypatch, hop, form):
    """M2M_FE_CHUNKS (read per call) changes only how chunks are spread over workgroups, never a value."""
    n_mels = 449 if form == "v2_nj8" else 384
    fe = LogMelSpectrogram(16000, 2048, hop, 20.0, n_mels)
    wav = _wave("music", 3, 60001, first=11).cuda()
    ref = fe(wav)
    p = fe.plan(3, 60001)
    cpc = -(-p["frames"] // p["frames_per_chunk"])
    for n in (1, 2, 3, cpc, cpc + 5):
        monkeypatch.setenv("M2M_FE_CHUNKS", str(n))
        _plan_matches(fe, 3, 60001, form=form, chunks=n, grid_x=-(-cpc // n))
        assert torch.equal(fe(wav), ref), n


def test_frames_per_workgroup_invariance(monkeypatch):
    """M2M_FE_FR (read per call) in the first form: FR 4, 8, 12 and 16 give the same rows."""
    fe = LogMelSpectrogram(16000, 2048, 274, 20.0, 384)
    wav = _wave("music", 2, 40000, first=13).cuda()
    ref = fe(wav)
    for fr in (4, 8, 12, 16):
        monkeypatch.setenv("M2M_FE_FR", str(fr))
        _plan_matches(fe, 2, 40000, form="v1_taps_lds", frames_per_chunk=fr)
        assert torch.equal(fe(wav), ref), fr


@pytest.mark.parametrize("hop,n_mels", [(256, 384), (200, 449), (512, 384)])
def test_row_offset_and_batch_stride_write_exactly_the_target(hop, n_mels):
    """m2m_logmel_f32 with a row offset and a batch stride that is not a whole number of rows, into a buffer filled with a
    sentinel: every target element is written with the plain call's value, no other element changes."""
    fe = LogMelSpectrogram(16000, 2048, hop, 20.0, n_mels)
    B, T, off, sentinel = 3, 9001, 2, 12345.5
    wav = _wave("noise", B, T, first=17).cuda()
    F = fe.num_frames(T)
    ref = torch.full((B * F * n_mels + 64,), sentinel, device="cuda")
    fe.forward_into(wav, ref[:B * F * n_mels].view(B, F, n_mels))     # the plain layout, with room behind it
    assert torch.all(ref[B * F * n_mels:] == sentinel)
    ref = ref[:B * F * n_mels].view(B, F, n_mels)
    stride = (off + F) * n_mels + 37
    buf = torch.full((B * stride + 101,), sentinel, device="cuda")
    lib = native.load()
    native.check(lib.m2m_logmel_f32(fe._get_plan(), wav.data_ptr(), B, T, buf.data_ptr(), stride, off,
                                    native.stream_handle(wav.device)), "m2m_logmel_f32")
    buf = buf.cpu()
    target = torch.zeros_like(buf, dtype=torch.bool)
    for b in range(B):
        s = b * stride + off * n_mels
        target[s:s + F * n_mels] = True
        assert torch.equal(buf[s:s + F * n_mels], ref[b].flatten().cpu()), b
    assert torch.all(buf[~target] == sentinel)


def test_batch_limit():
    """B = 65 535 (the grid's y limit) at the shortest T runs and equals a B = 4 run; B = 65 536 is refused and writes nothing."""
    fe = LogMelSpectrogram(16000, 2048, 256, 20.0, 384)
    base = _wave("noise", 4, 1025, first=19).cuda()
    ref = fe(base)
    _assert_rows_tile(fe(_tiled(base, 65535)), ref)
    x = _tiled(base, 65536)
    out = torch.full((65536, 5, 384), 7.0, device="cuda")
    with pytest.raises(native.NativeError, match="batch 65536 out of range"):
        fe.forward_into(x, out)
    with pytest.raises(native.NativeError, match="batch 65536 out of range"):
        fe.plan(65536, 1025)
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)


@pytest.mark.parametrize("hop,form", [(256, "v2_nj8"), (512, "v1_taps_lds")])
def test_indices_beyond_2_31(hop, form):
    """B T > 2^31 input samples and B F n_mels > 2^31 output floats: 4 distinct clips tiled over 65 535 rows, every row equal to
    the B = 4 run."""
    B, T, M = 65535, 32770, 512
    F = 1 + T // hop
    assert B * T > 2 ** 31 and B * F * M > 2 ** 31
    need = 4 * (B * T + B * F * M) + (2 << 30)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB of free device memory, {free / 2 ** 30:.1f} GiB free")
    fe = LogMelSpectrogram(16000, 2048, hop, 20.0, M)
    _plan_matches(fe, B, T, form=form)
    base = _wave("music", 4, T, first=23).cuda()
    ref = fe(base)
    x = _tiled(base, B)
    out = fe(x)
    del x
    assert torch.equal(out[-4:], ref[torch.arange(B - 4, B, device="cuda") % 4])
    _assert_rows_tile(out, ref)


# ---------------------------------------------------------------------------------------------------- a loaded filterbank
def _custom_fb(seed, n_mels=512):
    """widths 1..48 bins, an interior zero in most filters, every 37th filter empty, filter 0 starts at bin 0, the last filter
    ends at bin 1 024, random positions otherwise: every group of 64 has a 48-bin filter, so the padded table is 96 x 256 floats."""
    rng = np.random.default_rng(seed)
    fb = np.zeros((1025, n_mels), np.float32)
    for m in range(n_mels):
        if m % 37 == 5:
            continue
        w = 1 + m % 48
        s = 0 if m == 0 else (1025 - w if m == n_mels - 1 else int(rng.integers(0, 1025 - w + 1)))
        col = rng.uniform(0.05, 1.0, w).astype(np.float32)
        if w >= 3:
            col[int(rng.integers(1, w - 1))] = 0.0
        fb[s:s + w, m] = col
    return fb


def test_loaded_filterbank_runs_global_taps_and_follows_in_place_changes():
    fe = LogMelSpectrogram(16000, 2048, 256, 20.0, 512)
    orc = _oracle(16000, 256, 20.0, 512)
    wav = _wave("music", 2, 20000, first=29)
    x = wav.cuda()
    fe(x)                                                           # a plan exists for the mel filterbank
    fb = _custom_fb(0)
    start, width = fc.taps(fb)
    assert width.max() == 48 and width[width > 0].min() == 1 and start[0] == 0 and start[-1] + width[-1] - 1 == 1024
    sd = fe.state_dict()
    sd["melspectrogram.mel_scale.fb"] = torch.from_numpy(fb)
    fe.load_state_dict(sd)
    p = _plan_matches(fe, 2, 20000, form="v1_taps_global", n_wpad=fc.n_wpad(width))
    assert p["n_wpad"] > fc.FE_FBW_LDS
    out = fe(x).cpu()
    orc.fb = torch.from_numpy(fb)
    check_logmel(out, wav, orc, "loaded fb, taps in memory")
    empty = torch.from_numpy(np.nonzero(width == 0)[0])
    assert torch.all(out[:, :, empty] == FLOOR)
    # a second change in place: the plan is rebuilt (the key holds the buffer's version) and the rows follow it
    buf = fe.melspectrogram.mel_scale.fb
    with torch.no_grad():
        buf[:, torch.from_numpy(width > 12)] = 0.0
        buf[:, ::3] *= 0.5
    fb2 = buf.clone()
    _, width2 = fc.taps(fb2.numpy())
    _plan_matches(fe, 2, 20000, form="v1_taps_lds", n_wpad=fc.n_wpad(width2))
    out2 = fe(x).cpu()
    orc.fb = fb2
    check_logmel(out2, wav, orc, "loaded fb, changed in place")
    assert torch.all(out2[:, :, torch.from_numpy(width2 == 0)] == FLOOR)


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("args,T,msg", [
    ((22050, 256, 120), 4096, "more than 48 frequency bins"),
    ((16000, 256, 100), 4096, "more than 48 frequency bins"),
    ((16000, 256, 0), 4096, "bad n_mels"),
    ((16000, 256, 513), 4096, "n_mels=513 > 512 unsupported"),
    ((16000, 255, 384), 4096, "hop_length=255 must be even"),
    ((16000, 1026, 384), 4096, "hop_length=1026 must be even and in"),
    ((16000, 256, 384), 1024, "T=1024 too short for reflect padding"),
], ids=["49-bins", "53-bins", "mels0", "mels513", "hop255", "hop1026", "T1024"])
def test_refusals_raise_and_launch_nothing(args, T, msg):
    sr, hop, n_mels = args
    fe = LogMelSpectrogram(sr, 2048, hop, 20.0, n_mels)
    x = _wave("noise", 2, T).cuda()
    out = torch.full((2, fe.num_frames(T) + 1, n_mels), 3.0, device="cuda")
    with pytest.raises(native.NativeError, match=msg):
        fe.forward_into(x, out)
    torch.cuda.synchronize()
    assert torch.all(out == 3.0)


# ---------------------------------------------------------------------------------------------------- NaN / Inf
@pytest.mark.parametrize("hop,n_mels,form", [(256, 384, "v2_nj6"), (256, 512, "v2_nj8"), (512, 384, "v1_taps_lds")])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
def test_non_finite_sample_propagates_like_the_oracle(hop, n_mels, form, bad):
    """clamp(min=1e-6).log() keeps NaN: a frame that sees a NaN / Inf sample is non-finite on exactly the oracle's elements, and
    every other frame is bit-identical to the clean clip's.  Positions in the reflect-padded head, the middle and the tail."""
    T = 16000
    fe = LogMelSpectrogram(16000, 2048, hop, 20.0, n_mels)
    _plan_matches(fe, 1, T, form=form)
    orc = _oracle(16000, hop, 20.0, n_mels)
    clean = _wave("music", 1, T, first=31)
    positions = [0, 5, 700, 1023, 8000, T - 1024, T - 700, T - 1]
    wav = clean.repeat(len(positions) + 1, 1)
    for i, pos in enumerate(positions):
        wav[i + 1, pos] = bad
    out = fe(wav.cuda()).cpu()
    ref = orc(wav)
    assert torch.equal(out[0], fe(clean.cuda()).cpu()[0])
    for i, pos in enumerate(positions):
        row, bad_ref = out[i + 1], ~torch.isfinite(ref[i + 1])
        assert bad_ref.any(), pos
        assert torch.equal(~torch.isfinite(row), bad_ref), pos
        if bad != bad:
            assert torch.isnan(row[bad_ref]).all(), pos
        fine = ~bad_ref.any(1)
        assert torch.equal(row[fine], out[0][fine]), pos


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,da_clips", [(3, 48000, None), (64, 220500, "2"), (96, 220500, "4")])
def test_generate_refuses_a_clip_with_a_nan_sample(monkeypatch, precision, B, T, da_clips):
    """A NaN sample must not turn into plausible ids: it reaches the encoder as NaN rows and the decoder's range guard raises.  B = 3
    decodes with dec_attn_kernel; B = 64 / 96 at S = 864 are large chains whose attention is dec_attn_mc_kernel with 2 / 4 clips per
    workgroup (M2M_DA_CLIPS pins the form)."""
    if da_clips is not None:
        monkeypatch.setenv("M2M_DA_CLIPS", da_clips)
    import copy
    from music2midi_amd.checkpoint import load_t5_state
    from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry
    from music2midi_amd.model import Music2MIDI
    geom = T5Geometry(DEFAULT_CONFIG["model"]["t5"])
    sd = synth.t5_state_dict(geom, seed=0)
    m = Music2MIDI(copy.deepcopy(DEFAULT_CONFIG))
    load_t5_state(m.model, sd, strict=False)
    model = m.model.cuda().eval()
    model.set_precision(precision)
    wav = torch.from_numpy(synth.waveform_batch(40, B, T))
    idx = torch.from_numpy(synth.cond_index_batch(40, B))
    ok = model.generate(ModelInputs(input_waveform=wav.cuda(), cond_index=idx.cuda()), max_length=16)
    assert ok.shape[0] == B
    wav[B // 2 + 1, T // 2] = float("nan")
    with pytest.raises(native.NativeError, match="not finite"):
        model.generate(ModelInputs(input_waveform=wav.cuda(), cond_index=idx.cuda()), max_length=16)
