"""GPU: the on-device tokeniser (music2midi_amd.tokenize, csrc/tokenize.hip) against the host's ``MidiTokenizer``.  Every comparison
is ``torch.equal``: the kernel writes the ids the host loop writes, the labels form is ``Music2MIDI._labels``' tensor, and a
training step fed by it returns the same loss and gradients bit for bit."""
import copy

import numpy as np
import pytest
import torch

from music2midi_amd import augment, scoring, synth, tokenize
from music2midi_amd.config import DEFAULT_CONFIG, load_config
from music2midi_amd.input import ModelInputs
from music2midi_amd.tokenizer import PAD, MidiTokenizer

pytestmark = pytest.mark.gpu


def _tokenizer(ms=50, n_time=200):
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["tokenizer"]["midi_quantize_ms"] = ms
    cfg["tokenizer"]["vocab_size"]["time"] = n_time
    return MidiTokenizer(load_config(cfg))


@pytest.fixture(scope="module")
def tok():
    return _tokenizer()


def _clip(rng, n, duration=3.0, decimals=None):
    """n notes in array order as drawn (not sorted by onset), whole pitches 21..108."""
    on = rng.uniform(0.0, duration, n)
    off = on + rng.uniform(0.02, 0.8, n)
    if decimals is not None:
        on, off = np.round(on, decimals), np.round(off, decimals)
    return np.stack([on, off, rng.integers(21, 109, n).astype(np.float64), np.full(n, 80.0)], axis=1)


def _same(tok, batch, cutoff_time=None):
    """The device ids of the batch equal the host's; returns them (on the host)."""
    want = tok(batch, cutoff_time)
    out = tokenize.tokenize(tok, batch, cutoff_time)
    got = out.ids.cpu()
    assert got.dtype == torch.int64 and out.ids.is_cuda and got.shape == want.shape, (got.shape, want.shape)
    assert torch.equal(got, want), np.argwhere((got != want).numpy())[:5]
    assert out.lengths.cpu().tolist() == [len(tok._tokenize(n, cutoff_time)) for n in batch]
    return got


def test_random_clips_at_the_reference_geometry(tok):
    rng = np.random.default_rng(0)
    for B in (1, 5, 16):
        batch = [_clip(rng, int(n)) for n in rng.integers(1, 91, B)]
        batch[-1] = _clip(rng, 90)
        ids = _same(tok, batch)
        assert ids.shape[1] > 200 and (ids == PAD).any() == (B > 1)


def test_times_on_the_millisecond_grid_carry_the_ties(tok):
    rng = np.random.default_rng(1)
    batch = [_clip(rng, 90, decimals=3) for _ in range(8)]
    q = np.concatenate([b[:, 0] for b in batch]) / tok.time_step
    assert (q - np.floor(q) == 0.5).any()                     # quotients that are exact .5 ties: rint alone would send them down
    _same(tok, batch)
    ties = np.arange(25, 3000, 50) / 1000.0                   # every onset and offset on a tie
    _same(tok, [np.stack([ties, ties + 0.1, np.full(len(ties), 60.0), np.full(len(ties), 80.0)], axis=1)])


def test_chords_keep_the_array_order_inside_a_group(tok):
    rng = np.random.default_rng(2)
    chords = []
    for onset, offset in ((0.5, 1.0), (1.0, 1.5), (1.5, 1.0)):                   # the third chord ends where the second starts
        pitches = rng.permutation(np.r_[np.arange(50, 66), [60, 60, 52, 65]])    # 20 notes, repeated pitches among them
        chords.append(np.stack([np.full(20, onset), np.full(20, offset), pitches.astype(np.float64), np.full(20, 80.0)], axis=1))
    mixed = np.concatenate(chords)
    ids = _same(tok, [chords[0], mixed, mixed[rng.permutation(60)], mixed[::-1].copy()])
    assert ids[0, :22].tolist() == [tok.time_token_offset + 10, 3] + (chords[0][:, 2] + 5).astype(int).tolist()


def test_short_notes_and_offsets_before_their_onsets(tok):
    rng = np.random.default_rng(3)
    on = rng.uniform(0, 3, 40)
    short = np.stack([on, on + rng.uniform(0, 0.05, 40), rng.integers(40, 80, 40).astype(np.float64), np.full(40, 80.0)], axis=1)
    backwards = short.copy()
    backwards[:, 1] = on - rng.uniform(0, 1.5, 40)            # offset < onset, some of them negative
    zero = short.copy()
    zero[:, 1] = zero[:, 0]
    _same(tok, [short, backwards, zero, np.array([[0.0, 0.0, 60.0, 80.0]]), np.array([[0.0, -3.0, 60.0, 80.0], [0.049, 0.0, 61.0, 80.0]])])


def test_times_past_the_last_index_collapse_into_it(tok):
    rng = np.random.default_rng(4)
    late = _clip(rng, 30, duration=14.0)                       # indices up to 280 for 200 time ids
    beyond = np.array([[9.93, 9.94, 60.0, 80.0], [9.96, 12.0, 61.0, 80.0], [11.0, 11.5, 62.0, 80.0], [1e300, 1e300, 63.0, 80.0],
                       [1e17, 1.7e308, 64.0, 80.0], [3.0, 1e300, 65.0, 80.0]])
    ids = _same(tok, [late, beyond, np.array([[500.0, 600.0, 60.0, 80.0]])])
    last = tok.time_token_offset + 199
    assert ids[2, :6].tolist() == [last, 3, 65, 4, 65, 2] and (ids[1] == last).sum() == 1


def test_empty_one_note_and_full_clips_in_one_batch(tok):
    rng = np.random.default_rng(5)
    k = tokenize.MAX_NOTES
    wide = _tokenizer(10, 4096)                                # 4096 time ids: every onset and offset of 1024 notes on an index of its own
    distinct = np.stack([np.arange(k) * 0.04, np.arange(k) * 0.04 + 0.02, rng.integers(21, 109, k).astype(np.float64), np.full(k, 80.0)], axis=1)
    distinct = distinct[rng.permutation(k)]
    batch = [np.zeros((0, 4)), np.array([[0.3, 0.9, 72.0, 80.0]]), distinct, [], _clip(rng, k, duration=40.0)]
    ids = _same(wide, batch)
    assert ids.shape[1] == 6 * k + 1 == tokenize.row_bound(k, 4096)
    assert ids[0].tolist() == [2] + [PAD] * (6 * k) and ids[3, 0] == 2 and (ids[1, 7:] == PAD).all()
    # the same clips on the reference vocabulary: 1024 notes on 200 indices, groups of many pitches
    _same(tok, [batch[0], batch[1], _clip(rng, k), _clip(rng, 333)])
    with pytest.raises(ValueError, match="1025 notes"):
        tokenize.tokenize(tok, [batch[1], _clip(rng, k + 1)])
    empty = tokenize.tokenize(tok, [])
    assert empty.ids.shape == tok([]).shape == (0, 0) and empty.ids.is_cuda and empty.lengths.shape == (0,)


def test_pitches_that_are_no_whole_number_or_fall_below_the_pitch_ids(tok):
    notes = np.array([[0.1, 0.5, 60.5, 80.0], [0.2, 0.6, -5.0, 80.0], [0.3, 0.7, -6.0, 80.0], [0.4, 0.8, -4.5, 80.0], [0.5, 0.9, 127.99, 80.0],
                      [0.6, 1.0, -32768.0, 80.0], [0.7, 1.1, 32768.0, 80.0], [0.8, 1.2, 16777216.5 - 5 - 16777216, 80.0]])
    ids = _same(tok, [notes, notes[:3]])
    assert ids[1, :4].tolist() == [tok.time_token_offset + 2, 3, 65, tok.time_token_offset + 4]
    assert ids[1, 4:8].tolist() == [3, 0, tok.time_token_offset + 6, 3] and ids[1, 8] == -1      # -5 -> id 0 (PAD's), -6 -> -1
    # labels mode: id 0 becomes -100 wherever it stands, -1 stays
    want = tok([notes, notes[:3]])
    want[want == PAD] = -100
    got = tokenize.tokenize(tok, [notes, notes[:3]], labels=True).ids.cpu()
    assert torch.equal(got, want) and got[1, 5] == -100 and got[1, 8] == -1


@pytest.mark.parametrize("cutoff", [1.5, 0.30000000000000004, 0.0, 3, 100.0, float("nan")])
def test_cutoff_time_drops_notes(tok, cutoff):
    rng = np.random.default_rng(6)
    batch = [_clip(rng, 60, decimals=1), _clip(rng, 7), np.zeros((0, 4)), np.array([[0.3, 0.5, 60.0, 80.0], [0.30000000000000004, 0.5, 61.0, 80.0]])]
    ids = _same(tok, batch, cutoff)
    if cutoff == 0.0 or cutoff != cutoff:
        assert ids.shape == (4, 1) and (ids == 2).all()       # every clip emptied: [EOS]


def test_a_second_vocabulary_10_ms_steps_1000_time_ids():
    tok10 = _tokenizer(10, 1000)
    rng = np.random.default_rng(7)
    batch = [_clip(rng, 90, duration=9.5, decimals=3), _clip(rng, 250, duration=12.0), _clip(rng, 3)]
    ids = _same(tok10, batch)
    assert ids.max() == tok10.time_token_offset + 999           # the 12 s clip runs past the last index
    _same(_tokenizer(30, 200), batch)
    _same(_tokenizer(50, 1), batch[1:])                         # one time id: a single group


def test_width_cuts_a_long_row_in_place_and_reports_it(tok):
    rng = np.random.default_rng(8)
    batch = [_clip(rng, 5), _clip(rng, 90), _clip(rng, 6), np.zeros((0, 4))]
    want = tok(batch)
    full = [len(tok._tokenize(n)) for n in batch]
    width = 64
    assert full[1] > width > max(full[0], full[2])
    sentinel = -7
    out = tokenize.tokenize(tok, batch, width=width)
    assert out.ids.shape == (4, width) and out.lengths.cpu().tolist() == full         # the true length of the row that was cut
    assert torch.equal(out.ids.cpu(), want[:, :width])
    with pytest.raises(ValueError, match="clip 1 gives .* ids, more than width=64"):
        out.check()
    # nothing is written beyond `width`: the same call into a wider buffer leaves the columns behind it as they were
    from music2midi_amd import native
    flat, per_clip = tokenize._flat_notes(batch)
    packed = torch.from_numpy(tokenize._pack(flat, per_clip)).cuda()
    buf = torch.full((4, width + 8), sentinel, dtype=torch.int64, device="cuda")
    lengths = torch.empty(4, dtype=torch.int32, device="cuda")
    native.check(native.load().m2m_tokenize_notes(packed.data_ptr(), packed.data_ptr() + 24 * len(flat), len(flat), 4, tok.time_step, 5,
                                                  tok.time_token_offset, 200, 0, 0.0, PAD, 0, PAD, buf.data_ptr(), width, width + 8,
                                                  lengths.data_ptr(), native.stream_handle()), "m2m_tokenize_notes")
    assert torch.equal(buf[:, :width].cpu(), want[:, :width]) and (buf[:, width:] == sentinel).all() and lengths.cpu().tolist() == full
    # a width that holds every row raises nothing and is the host tensor, padded
    roomy = tokenize.tokenize(tok, batch, width=600).check()
    assert torch.equal(roomy.ids[:, :want.shape[1]].cpu(), want) and (roomy.ids[:, want.shape[1]:] == PAD).all()


def test_a_row_the_kernel_cannot_place_is_reported_not_written(tok):
    """The eligibility rule keeps such values away from the kernel; handed to it directly, the row is all fill and its length -1."""
    from music2midi_amd import native
    good = np.array([[0.1, 0.5, 60.0, 80.0]])
    for bad in ([0.2, np.nan, 61.0, 80.0], [-0.1, 0.5, 61.0, 80.0], [np.inf, 0.5, 61.0, 80.0], [0.2, 0.5, np.nan, 80.0], [0.2, 0.5, 40000.0, 80.0]):
        flat = np.concatenate([good, good, np.array([bad]), good])
        per_clip = np.array([1, 2, 1])
        packed = torch.from_numpy(tokenize._pack(flat, per_clip)).cuda()
        buf = torch.full((3, 12), -7, dtype=torch.int64, device="cuda")
        lengths = torch.empty(3, dtype=torch.int32, device="cuda")
        native.check(native.load().m2m_tokenize_notes(packed.data_ptr(), packed.data_ptr() + 24 * 4, 4, 3, tok.time_step, 5, tok.time_token_offset,
                                                      200, 0, 0.0, PAD, 0, PAD, buf.data_ptr(), 10, 12, lengths.data_ptr(),
                                                      native.stream_handle()), "m2m_tokenize_notes")
        assert lengths.cpu().tolist() == [7, -1, 7]
        assert buf[0, :10].tolist() == tok([good])[0].tolist() + [PAD] * 3 == [135, 3, 65, 143, 4, 65, 2, 0, 0, 0]
        assert (buf[1, :10] == PAD).all() and (buf[:, 10:] == -7).all() and torch.equal(buf[0], buf[2])


def _host_labels(tok, batch, bucket=16):
    labels = tok(batch)
    labels[labels == PAD] = -100
    return torch.nn.functional.pad(labels, (0, -labels.shape[1] % bucket), value=-100)


def test_labels_form_at_bucket_16(tok):
    rng = np.random.default_rng(9)
    side = torch.cuda.Stream()
    for sizes in ((3, 1, 0), (90, 45, 2, 60), (5,)):
        batch = [_clip(rng, n) for n in sizes]
        want = _host_labels(tok, batch)
        got = tokenize.tokenize(tok, batch, labels=True, bucket=16).ids
        assert got.shape[1] % 16 == 0 and torch.equal(got.cpu(), want)
        helper = tokenize.training_labels(tok, batch, "cuda", PAD, 16, side)
        assert helper.is_cuda and torch.equal(helper.cpu(), want)
    assert tokenize.training_labels(tok, batch, "cuda", 1, 16, side) is None                    # another pad id: the host's business
    assert tokenize.training_labels(tok, [np.array([[np.nan, 1.0, 60.0, 80.0]])], "cuda", PAD, 16, side) is None


def test_detokenize_of_the_device_ids_is_decode_of_the_host_ids(tok):
    rng = np.random.default_rng(10)
    batch = [_clip(rng, 40), _clip(rng, 3), np.zeros((0, 4)), _clip(rng, 90, decimals=3)]
    dev = tokenize.tokenize(tok, batch).ids
    got = scoring.detokenize(tok, dev).to_numpy()
    want = tok.decode(tok(batch))
    assert len(got) == len(want) == 4 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert sum(len(w) for w in want) > 60


def test_after_shift_notes(tok):
    rng = np.random.default_rng(12)
    batch = [_clip(rng, 50), _clip(rng, 20), _clip(rng, 1)]
    shifted = augment.shift_notes(batch, [-12, 7, 0])
    ids = _same(tok, shifted)
    assert not torch.equal(ids, tok(batch))


# ------------------------------------------------------------------------------------------------ the callers
def _tiny_cfg(device_labels):
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["model"]["t5"].update(d_model=128, d_ff=256, num_layers=2, num_decoder_layers=2, num_heads=2)
    cfg["dataloader"]["batch_size"] = 2
    cfg["trainer"]["log_every_n_steps"] = 1000
    if device_labels is not None:
        cfg["trainer"]["device_labels"] = device_labels
    return cfg


def _labelled_batch():
    rng = np.random.default_rng(13)
    notes = (_clip(rng, 9, duration=1.0), _clip(rng, 4, duration=1.0))
    wav = torch.from_numpy(synth.waveform_batch(400, 2, 16000, "music")).cuda()
    idx = torch.from_numpy(synth.cond_index_batch(14, 2)).cuda()
    return ModelInputs(input_waveform=wav, notes_batch=notes, cond_index=idx)


def test_training_step_with_device_labels_is_the_host_step_bit_for_bit(monkeypatch):
    from music2midi_amd.model import Music2MIDI
    batch = _labelled_batch()
    runs = {}
    for key in (None, True):
        torch.manual_seed(5)
        m = Music2MIDI(_tiny_cfg(key)).cuda().eval()           # the same weights; eval(): no dropout
        m.train_precision = "fp32"
        labels = m._labels(batch.notes_batch)
        assert labels.is_cuda == bool(key) and labels.shape[1] % m.LABEL_BUCKET == 0
        if key:
            host = tokenize.training_labels
            asked = []
            monkeypatch.setattr(tokenize, "training_labels", lambda *a, **k: asked.append(1) or host(*a, **k))
        loss = m.training_step(batch, 0)
        if key:
            assert asked == [1] and m.model._label_stream is not None
        runs[key] = (labels.cpu(), loss.clone(), m._trainer.grads.clone(), m)
    (lab_h, loss_h, g_h, _), (lab_d, loss_d, g_d, m) = runs[None], runs[True]
    assert torch.equal(lab_h, lab_d) and torch.equal(lab_d, _host_labels(m.model.tokenizer, batch.notes_batch))
    assert torch.equal(loss_h, loss_d) and torch.isfinite(loss_d) and torch.equal(g_h, g_d) and float(g_d.abs().max()) > 0
    # notes the device path does not take go to the host with the key set
    odd = (np.array([[0.1, 0.5, 40000.0, 80.0]]), batch.notes_batch[1])
    assert not m._labels(odd).is_cuda


def test_forward_with_device_labels_is_the_host_forward_bit_for_bit():
    from music2midi_amd.transformer import T5Transformer
    batch = _labelled_batch()
    outs = []
    for key in (None, True):
        torch.manual_seed(5)
        t5 = T5Transformer(_tiny_cfg(key)).cuda().eval()
        assert (t5.device_labels(batch.notes_batch) is not None) == bool(key)
        outs.append(t5(batch))
    assert torch.equal(outs[0].loss, outs[1].loss) and torch.isfinite(outs[0].loss) and torch.equal(outs[0].logits, outs[1].logits)
