"""GPU: the on-device augmentation (music2midi_amd.augment -> csrc/augment.hip) against its definition, the host functions of
music2midi_amd/audio.py (float64 inside): parity of the result and of every stage on well-conditioned input, the defined
properties on ill-conditioned input, the bit-exact parts, the training loop's keyword, and the refusals.

Shapes: T = 2 085 (5 frames, not a multiple of the hop), T = 5 000, T = 66 150 (the training clip, B = 3); every batch mixes
steps, with 0, -6 and +5 among them, so the ragged extents and the step-0 copy run in one call.  The host references and the
device results of a case are computed once and shared by the tests of that case."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from music2midi_amd import audio, augment, native, synth
from music2midi_amd.config import DEFAULT_CONFIG
from music2midi_amd.input import ModelInputs

pytestmark = pytest.mark.gpu

SR = 22050

# max |gpu - host| / max |host| per clip (the stages: per frame, relative to the frame's own maximum), worst case over CASES as
# measured on an MI355X; the bars are 4 x that (FMA contraction and summation order differ between builds), and no bar may pass 1e-3:
# the host function moves by <= 4.6e-6 under fp32-sized input noise on this signal, so more than 1e-3 is a wrong kernel, not noise.
# Measured: out 2.863e-06 (T66150, step +5), stft 1.416e-07 (T2085, +12), stretched_stft 1.512e-05 (T66150, +5: 174 phasor steps),
# stretched_wave 2.399e-06 (T66150, +5); at T <= 5 000 the output is within 5.2e-07.
MEASURED = {"out": 2.863e-06, "stft": 1.416e-07, "stretched_stft": 1.512e-05, "stretched_wave": 2.399e-06}
BAR = {k: 4 * v for k, v in MEASURED.items()}

CASES = {
    "T2085": (2085, [0, -6, 5, 12], [False, True, False, True]),
    "T5000": (5000, [-6, 0, 5, -12, 3], [True, False, False, False, True]),
    "T66150": (66150, [-6, 0, 5], [False, True, True]),
}


def _signal(T, seed):
    """Well conditioned: every bin of every frame carries energy far above fp32 noise."""
    t = np.arange(T) / SR
    y = 0.25 * np.random.default_rng(seed).standard_normal(T) + 0.2 * np.sin(2 * np.pi * 440 * t) + 0.15 * np.sin(2 * np.pi * 1318.5 * t)
    return y.astype(np.float32)


def _host(y, step, norm):
    """The oracle and its intermediates for one clip: (out, stft [F, 1025], stretched stft [F', 1025], stretched wave)."""
    y = audio.normalize(y) if norm else y
    out = audio.pitch_shift(y, SR, step)
    if step == 0:
        return out, None, None, None
    rate = 2.0 ** (-float(step) / 12)
    D = audio._stft(np.asarray(y, dtype=np.float64), 2048, 512)
    return out, D.T, audio._phase_vocoder(D, rate, 512, 2048).T, audio.time_stretch(y, rate)


_done = {}


def _case(name):
    if name not in _done:
        T, steps, norms = CASES[name]
        wav = np.stack([_signal(T, T + b) for b in range(len(steps))])
        out, stages = augment.pitch_shift_batch(torch.from_numpy(wav).cuda(), steps, norms, return_stages=True)
        host = [_host(wav[b], steps[b], norms[b]) for b in range(len(steps))]
        _done[name] = (wav, out.cpu().numpy(), stages, host)
    return _done[name]


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _rel_frames(a, b):
    """worst frame of max_k |a - b| / max_k |b|; a frame the host has all zero must be all zero"""
    top = np.abs(b).max(axis=1)
    err = np.abs(a - b).max(axis=1)
    assert np.all(err[top == 0] == 0)
    return float((err[top > 0] / top[top > 0]).max()) if (top > 0).any() else 0.0


def test_bars_are_four_times_the_measurement_and_below_the_cap():
    assert all(BAR[k] == 4 * MEASURED[k] and BAR[k] <= 1e-3 for k in MEASURED)


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("name", list(CASES))
def test_pitch_shift_matches_the_host_function(name):
    wav, out, _, host = _case(name)
    T, steps, _ = CASES[name]
    assert out.shape == wav.shape and out.dtype == np.float32 and np.isfinite(out).all()
    worst = 0.0
    for b, step in enumerate(steps):
        if step == 0:
            assert np.array_equal(out[b], host[b][0])
            continue
        worst = max(worst, _rel(out[b], host[b][0]))
        print(f"  {name} clip {b} step {step:+d}: out rel err {_rel(out[b], host[b][0]):.3e}")
    print(f"{name}: worst out rel err {worst:.3e} (bar {BAR['out']:.1e})")
    assert worst <= BAR["out"]


@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_matches_the_host_intermediates(name):
    wav, out, stages, host = _case(name)
    T, steps, _ = CASES[name]
    worst = dict(stft=0.0, stretched_stft=0.0, stretched_wave=0.0)
    for b, step in enumerate(steps):
        if step == 0:
            assert stages.stft[b] is None and stages.stretched_stft[b] is None and stages.stretched_wave[b] is None
            continue
        p = augment.plan(T, step)
        S, P, W = stages.stft[b].cpu().numpy(), stages.stretched_stft[b].cpu().numpy(), stages.stretched_wave[b].cpu().numpy()
        assert S.shape == host[b][1].shape == (p.frames, 1025)
        assert P.shape == host[b][2].shape == (p.stretched_frames, 1025)
        assert W.shape == host[b][3].shape == (p.stretched_len,)
        e = dict(stft=_rel_frames(S, host[b][1]), stretched_stft=_rel_frames(P, host[b][2]), stretched_wave=_rel(W, host[b][3]))
        print(f"  {name} clip {b} step {step:+d}: " + ", ".join(f"{k} {v:.3e}" for k, v in e.items()))
        worst = {k: max(worst[k], e[k]) for k in worst}
    print(f"{name}: worst " + ", ".join(f"{k} {v:.3e} (bar {BAR[k]:.1e})" for k, v in worst.items()))
    for k in worst:
        assert worst[k] <= BAR[k], k


# ------------------------------------------------------------------------------------------------ 2. ill-conditioned input
def _dominant_hz(seg):
    spec = np.abs(np.fft.rfft(seg * np.hanning(len(seg))))
    return float(np.argmax(spec)) * SR / len(seg)


def test_ill_conditioned_input_is_held_to_what_is_defined():
    """A tone after digital silence and a tone followed by noise: bins pass through frames that hold fp32 noise only, where the
    accumulated phase is arbitrary — the HOST output moves by 1.2 to 1.6 x its peak under 6e-8 input noise, so the waveforms are not
    compared.  Held instead: the magnitudes of both spectra, the length, the pitch of the shifted tone, the energy, no NaN, and
    exact zeros for a silent clip."""
    T = SR
    t = np.arange(T) / SR
    tone = (0.5 * np.sin(2 * np.pi * 440 * t)).astype(np.float32)
    after_silence = tone.copy()
    after_silence[:8192] = 0.0
    then_noise = tone.copy()
    then_noise[12000:] = (0.25 * np.random.default_rng(3).standard_normal(T - 12000)).astype(np.float32)
    wav = np.stack([after_silence, then_noise, np.zeros(T, np.float32), after_silence, then_noise])
    steps = [-6, 5, 3, 5, -6]
    tone_at = [slice(10240, 21000), slice(1024, 10800), None, slice(10240, 21000), slice(1024, 10800)]
    out, stages = augment.pitch_shift_batch(torch.from_numpy(wav).cuda(), steps, None, return_stages=True)
    out = out.cpu().numpy()
    assert out.shape == (5, T) and np.isfinite(out).all()
    assert np.all(out[2] == 0.0)
    for b, step in enumerate(steps):
        h_out, h_S, h_P, _ = _host(wav[b], step, False)
        S, P = stages.stft[b].cpu().numpy(), stages.stretched_stft[b].cpu().numpy()
        assert np.isfinite(S).all() and np.isfinite(P).all()
        e_s, e_p = _rel_frames(np.abs(S), np.abs(h_S)), _rel_frames(np.abs(P), np.abs(h_P))
        print(f"  clip {b} step {step:+d}: |stft| {e_s:.3e}, |stretched stft| {e_p:.3e}")
        assert e_s <= BAR["stft"] and e_p <= BAR["stretched_stft"]
        if tone_at[b] is None:
            continue
        want = 440.0 * 2 ** (step / 12)
        got, got_host = _dominant_hz(out[b][tone_at[b]]), _dominant_hz(h_out[tone_at[b]])
        ratio = float(np.sqrt((out[b] ** 2).mean()) / np.sqrt((h_out ** 2).mean()))
        print(f"           tone {got:.1f} Hz (host {got_host:.1f}, wanted {want:.1f}), energy ratio to the host {ratio:.4f}")
        assert abs(got - want) <= SR / 2048                   # one bin of the analysis FFT
        assert 0.8 < ratio < 1.1                              # the band tests/test_next_rows_cpu.py holds the host function to


# ------------------------------------------------------------------------------------------------ 3. exactness
def test_step_zero_and_normalise_only_are_bit_exact():
    T = 5000
    wav = np.stack([_signal(T, 70 + b) for b in range(5)])
    wav[3] = 0.0
    wav[4] = np.float32(1e-39) * np.sign(wav[4])              # below FLT_MIN: audio.normalize leaves the clip alone
    x = torch.from_numpy(wav).cuda()
    out = augment.pitch_shift_batch(x, [0, 0, -6, 0, 0], [False, True, False, True, True])
    assert torch.equal(out[0], x[0])
    assert torch.equal(out[1].cpu(), torch.from_numpy(audio.normalize(wav[1])))
    assert float(out[1].abs().max()) == 1.0
    assert torch.equal(out[3], x[3]) and torch.equal(out[4], x[4])
    assert torch.equal(augment.pitch_shift_batch(x, [0] * 5), x)


def test_a_clip_does_not_depend_on_its_batch_and_calls_repeat_bit_for_bit():
    name = "T5000"
    wav, out, _, _ = _case(name)
    T, steps, norms = CASES[name]
    x = torch.from_numpy(wav).cuda()
    again = augment.pitch_shift_batch(x, steps, norms)
    assert np.array_equal(again.cpu().numpy(), out)
    for b in (0, 2, 3):
        alone = augment.pitch_shift_batch(x[b:b + 1], steps[b:b + 1], norms[b:b + 1])
        assert np.array_equal(alone.cpu().numpy()[0], out[b]), b
    # other neighbours, another position, a larger batch (the workspace grows)
    order = [4, 3, 2, 1, 0, 2, 2]
    mixed = augment.pitch_shift_batch(x[order], [steps[i] for i in order], [norms[i] for i in order]).cpu().numpy()
    for pos, i in enumerate(order):
        assert np.array_equal(mixed[pos], out[i]), (pos, i)


def test_calls_on_two_streams_have_workspaces_of_their_own():
    name = "T5000"
    wav, out, _, _ = _case(name)
    T, steps, norms = CASES[name]
    x = torch.from_numpy(wav).cuda()
    aug = augment._augmenter(x.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = augment.pitch_shift_batch(x, steps, norms)
        ws_side = aug.workspace_for(len(steps), T)
    on_main = augment.pitch_shift_batch(x, steps, norms)
    ws_main = aug.workspace_for(len(steps), T)
    torch.cuda.synchronize()
    assert ws_side.data_ptr() != ws_main.data_ptr()
    assert np.array_equal(on_side.cpu().numpy(), out) and np.array_equal(on_main.cpu().numpy(), out)


# ------------------------------------------------------------------------------------------------ 4. the training loop
def _batches(n, B=3):
    out = []
    for i in range(n):
        notes = tuple(np.array([[0.1 * (b + 1), 0.4 + 0.1 * b, 50.0 + 3 * b + i, 80.0], [0.6, 0.9, 62.0 + b, 80.0]]) for b in range(B))
        wav = torch.from_numpy(synth.waveform_batch(300 + i, B, 16000, "music")).cuda()
        idx = torch.from_numpy(synth.cond_index_batch(11 + i, B)).cuda()
        out.append(ModelInputs(input_waveform=wav, notes_batch=notes, cond_index=idx))
    return out


def test_fit_batches_augments_every_batch_and_is_unchanged_without_the_keyword(monkeypatch):
    from music2midi_amd.model import Music2MIDI
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["model"]["t5"].update(d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2)
    cfg["dataloader"]["batch_size"] = 3
    cfg["trainer"]["log_every_n_steps"] = 1000
    batches = _batches(2)
    kept = [(b.input_waveform.clone(), [n.copy() for n in b.notes_batch]) for b in batches]

    def fresh():
        torch.manual_seed(5)
        m = Music2MIDI(copy.deepcopy(cfg)).cuda()
        m.train_precision = "bf16"
        return m

    plain = fresh().fit_batches(batches)                       # no keyword; the guarded block in fit_batches is the only change to the loop
    assert fresh().fit_batches(batches, augment=None) == plain

    seen = []
    m = fresh()
    step = m.training_step
    monkeypatch.setattr(m, "training_step", lambda batch, i: (seen.append(batch), step(batch, i))[1])
    losses = m.fit_batches(batches, augment=np.random.default_rng(42))
    rng = np.random.default_rng(42)
    by_hand = [augment.transpose_batch(b, *augment.draw(3, rng)) for b in batches]
    assert len(seen) == 2 and len(losses) == 2
    rng = np.random.default_rng(42)
    for got, want, src in zip(seen, by_hand, batches):
        steps, norms = augment.draw(3, rng)
        assert torch.equal(got.input_waveform, want.input_waveform) and got.cond_index is src.cond_index
        for b in range(3):
            assert np.array_equal(got.notes_batch[b][:, 2], src.notes_batch[b][:, 2] + steps[b])
            assert np.array_equal(got.notes_batch[b][:, [0, 1, 3]], src.notes_batch[b][:, [0, 1, 3]])
    assert any(s != 0 for s in steps)
    assert fresh().fit_batches(by_hand) == losses and losses != plain
    # augment=True is default_rng(0); the caller's batches are untouched
    rng = np.random.default_rng(0)
    assert fresh().fit_batches(batches, augment=True) == fresh().fit_batches([augment.augment(b, rng) for b in batches])
    for b, (w, notes) in zip(batches, kept):
        assert torch.equal(b.input_waveform, w) and all(np.array_equal(x, y) for x, y in zip(b.notes_batch, notes))


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_raise_and_launch_nothing():
    x = torch.from_numpy(np.stack([_signal(2085, 90), _signal(2085, 91)])).cuda()
    for steps, msg in [([0, 13], "step 13 of clip 1"), ([-13, 0], "step -13 of clip 0")]:
        with pytest.raises(native.NativeError, match=msg):
            augment.pitch_shift_batch(x, steps)
    with pytest.raises(native.NativeError, match="batch 0 out of range"):
        augment.pitch_shift_batch(x[:0], [])
    with pytest.raises(native.NativeError, match="T=0 out of range"):
        augment.pitch_shift_batch(x[:, :0], [1, 2])
    # straight at the library, with an output it must not touch
    lib, aug = native.load(), augment._augmenter(x.device)
    ws = aug.workspace_for(2, 2085)
    out = torch.full_like(x, 3.0)
    ws.zero_()
    torch.cuda.synchronize()

    def call(steps, out_ptr, B=2, T=2085):
        arr = (C.c_int * len(steps))(*steps)
        return lib.m2m_pitch_shift_f32(aug.handle, x.data_ptr(), B, T, arr, None, out_ptr, ws.data_ptr(), None, native.stream_handle(x.device))

    for steps, ptr, msg in [([1, 13], out.data_ptr(), b"step 13"), ([1, 2], x.data_ptr(), b"overlaps"),
                            ([1, 2], x.data_ptr() + 4 * 2085, b"overlaps"), ([1, 2], 0, b"null waveform / output")]:
        assert call(steps, ptr) == -1 and msg in lib.m2m_last_error()
    assert call([1, 2], out.data_ptr(), B=65536) == -1 and call([1, 2], out.data_ptr(), T=(1 << 22) + 1) == -1
    torch.cuda.synchronize()
    assert torch.all(out == 3.0) and not ws.any()
    assert torch.equal(x.cpu(), torch.from_numpy(np.stack([_signal(2085, 90), _signal(2085, 91)])))
    assert call([1, 2], out.data_ptr()) == 0                    # the same call with valid arguments runs
    torch.cuda.synchronize()
    assert not torch.any(out == 3.0)
