"""GPU: the frame-level piano-roll counts and the TP / FN / FP notes on the device (scoring.frame_counts, scoring.error_notes,
csrc/frame_roll.hip) against their definition on the host (music2midi_amd.frame_metrics) applied to what ``scoring.detokenize``
returns: every integer and every note is compared with ``==`` - on the crafted cases, at the edges of the frame tile, on random
batches, across the rows of a sequential decode, under a sweep of confidence thresholds, and end to end through ``Music2MIDI`` on
random-init weights."""
import copy

import numpy as np
import pytest
import torch

import frame_metrics_cases as fc
from music2midi_amd import confidence, evaluation, frame_metrics, native, note_metrics, scoring, synth
from music2midi_amd.config import DEFAULT_CONFIG, T5Geometry

pytestmark = pytest.mark.gpu
TOK = fc.TOK
TILE = scoring.FRAME_TILE
KEYS = ("tp", "fn", "fp", "melody_tp", "melody_fn", "melody_fp")


def _want(labels, decoded):
    """[T, 6] of the definition."""
    return np.asarray([frame_metrics.frame_counts(l, d) for l, d in zip(labels, decoded)], dtype=np.int64).reshape(-1, 6)


def _got(c, k=0):
    return np.stack([getattr(c, name)[:, k] for name in KEYS], axis=1)


def _check_notes(found, labels, decoded, melody_only):
    """``ErrorNotes.to_numpy()`` against roll_to_notes(error_rolls(...)) per timeline and kind; the largest share of a slot used."""
    got = found.to_numpy()
    assert len(got) == len(labels)
    for t, (l, d) in enumerate(zip(labels, decoded)):
        for kind, roll in enumerate(frame_metrics.error_rolls(l, d, melody_only)):
            want = frame_metrics.roll_to_notes(roll)
            assert got[t][kind].dtype == np.float64 and np.array_equal(got[t][kind], want), (t, frame_metrics.KINDS[kind], melody_only,
                                                                                          got[t][kind][:5], want[:5])
    counts = found.counts.cpu().numpy()
    assert found.notes.shape[:2] == (len(labels), 3) and found.notes.shape[3] == 3 and (counts <= found.notes.shape[2]).all()
    return counts.max() / found.notes.shape[2] if counts.size else 0.0


def _check_batched(ids, labels, notes_too=True):
    ids_dev = torch.from_numpy(ids).cuda()
    decoded = scoring.detokenize(TOK, ids_dev).to_numpy()
    c = scoring.frame_counts(TOK, ids_dev, labels)
    assert c.tp.dtype == np.int64 and all(getattr(c, k).shape == (len(ids), 1) for k in KEYS) and c.frames.shape == (len(ids),)
    want = _want(labels, decoded)
    assert np.array_equal(_got(c), want), (_got(c).tolist(), want.tolist())
    assert c.frames.tolist() == [frame_metrics.n_frames_of(l, d) for l, d in zip(labels, decoded)]
    if notes_too:
        for melody_only in (False, True):
            found = scoring.error_notes(TOK, ids_dev, labels, melody_only=melody_only)
            _check_notes(found, labels, decoded, melody_only)
            # the runs of the rolls add up to the counts, for every kind
            frames = [[int((a[:, 1] * 100).round().sum() - (a[:, 0] * 100).round().sum()) for a in kinds] for kinds in found.to_numpy()]
            assert np.array_equal(np.asarray(frames).reshape(-1, 3), want[:, 3:] if melody_only else want[:, :3])
    return c, want, decoded


def test_crafted_cases_through_the_kernels():
    names = list(fc.CRAFTED)
    ids = fc.id_rows([fc.CRAFTED[n][1] for n in names], 24)
    labels = [fc.CRAFTED[n][0] for n in names]
    c, want, decoded = _check_batched(ids, labels)
    for r, n in enumerate(names):
        assert np.array_equal(decoded[r], fc.est_seconds(fc.CRAFTED[n][1])), n
        assert tuple(_got(c)[r].tolist()) == fc.CRAFTED[n][2], n
    ids_dev = torch.from_numpy(ids).cuda()
    full, melody = scoring.error_notes(TOK, ids_dev, labels).to_numpy(), scoring.error_notes(TOK, ids_dev, labels, melody_only=True).to_numpy()
    for r, n in enumerate(names):
        for kind in range(3):
            assert np.array_equal(full[r][kind], fc.note_list(fc.CRAFTED[n][3][kind])), (n, kind)
            if n in fc.CRAFTED_MELODY:
                assert np.array_equal(melody[r][kind], fc.note_list(fc.CRAFTED_MELODY[n][kind])), (n, kind)
    # one case alone (one timeline, one workgroup) and the micro-average of the batch
    r = names.index("melody top changes mid-note")
    alone, _, _ = _check_batched(ids[r:r + 1], labels[r:r + 1])
    assert tuple(_got(alone)[0].tolist()) == (199, 50, 0, 149, 50, 50)
    assert alone.precision.tolist() == [1.0] and alone.recall.tolist() == [199 / 249] and alone.melody_precision.tolist() == [149 / 199]
    sums = want.sum(axis=0)
    p, rec, f = note_metrics.precision_recall_f1(sums[0], sums[0] + sums[1], sums[0] + sums[2])
    assert (c.precision[0], c.recall[0], c.f1[0]) == (p, rec, f) and c.per_timeline_f1.shape == (len(names), 1)
    scores = evaluation.frame_scores_tokens(TOK, ids_dev, labels)
    assert scores["f1"].tolist() == [f] and [scores[k].tolist() for k in KEYS] == [[v] for v in sums.tolist()]
    # empty sides, alone: labels empty with the output non-empty, and the other way round
    for n in ("no labels", "cut at the last frame, nothing decoded", "nothing at all"):
        r = names.index(n)
        one, _, _ = _check_batched(ids[r:r + 1], labels[r:r + 1])
        assert tuple(_got(one)[0].tolist()) == fc.CRAFTED[n][2]


# n_frames of the timelines of the tile-edge batch: frames [0, n_frames - 1) are compared, hence the + 1 and + 2.  The longest
# timeline sits next to the one of 1 frame.
EDGE_FRAMES = [0, 2 * TILE + 2, 1, 2, 31, 32, 33, 34, 64, 65, TILE, TILE + 1, TILE + 2, 2 * TILE + 1]


def _edge_batch():
    rng = np.random.default_rng(5)
    frames = EDGE_FRAMES + [int(n) for n in rng.integers(3, 3 * TILE, 33 - len(EDGE_FRAMES) - 3)] + [3 * TILE + 7, 3 * TILE + 1, 4 * TILE]
    labels, rows = [], []
    for t, n in enumerate(frames):
        if n == 0:
            labels.append(fc.ref())
            rows.append([])
            continue
        lab = fc.labels_ending_at(rng, n)
        # decoded notes on the 50 ms grid that end before the labels do, so that the labels decide n_frames; none in short timelines
        top = min((n - 2) // 5, 55)
        dec = [(int(a), int(a + rng.integers(1, 8)), int(rng.choice((48, 60, 64, 76)))) for a in rng.integers(0, max(top, 1), 9)] if top > 8 else []
        rows.append([(a, min(b, top), p) for a, b, p in dec if a < min(b, top)])
        labels.append(lab)
    edge = TILE / 100
    assert int(edge * 100) == TILE and int(2 * edge * 100) == 2 * TILE
    # a run that ends exactly at a tile edge (last frame TILE - 1), one that starts exactly at one, one that spans two whole tiles
    labels[-3] = np.concatenate([labels[-3], fc.ref((edge - 0.5, edge, 50), (edge, edge + 0.5, 52), (2 * edge - 0.01, 2 * edge, 53))])
    labels[-2] = np.concatenate([labels[-2], fc.ref((edge / 2, 3 * edge, 51), (0.0, 3 * edge + 0.01, 90))])
    labels[-1] = np.concatenate([labels[-1], fc.ref((edge - 0.01, 3 * edge + 0.01, 49), (edge, 2 * edge, 55), (0.0, 4 * edge, 1))])
    return frames, labels, fc.id_rows(rows, 64)


def test_tile_edges_in_one_batch():
    frames, labels, ids = _edge_batch()
    assert len(labels) == 33 and frames[1] == max(frames[:14]) and frames[2] == 1
    c, want, decoded = _check_batched(ids, labels)
    assert c.frames.tolist() == frames                            # the labels decide n_frames, as built
    assert sum(len(d) == 0 for d in decoded) >= 5 and sum(len(d) > 0 for d in decoded) >= 20
    assert want[0].tolist() == [0] * 6 and want[2].tolist() == [0] * 6 and want[:, 0].sum() > 0 and want[:, 2].sum() > 0
    # the three runs at the tile edges came out as one note each
    fn = scoring.error_notes(TOK, torch.from_numpy(ids).cuda(), labels).to_numpy()
    rows = [tuple(n) for n in fn[-3][1][:, :3].tolist()]
    assert ((TILE - 50) / 100, TILE / 100, 50.0) in rows and (TILE / 100, (TILE + 50) / 100, 52.0) in rows
    assert ((2 * TILE - 1) / 100, 2 * TILE / 100, 53.0) in rows
    assert [tuple(n) for n in fn[-2][1][:, :3].tolist() if n[2] == 51.0] == [(TILE / 200, 3 * TILE / 100, 51.0)]
    assert [tuple(n) for n in fn[-1][1][:, :3].tolist() if n[2] == 1.0] == [(0.0, (4 * TILE - 1) / 100, 1.0)]


@pytest.mark.parametrize("seed", range(20))
def test_random_batches(seed):
    rng = np.random.default_rng(400 + seed)
    cases = [fc.random_pair(rng) for _ in range(5)]
    ids = fc.tokenised([c[1] for c in cases], 64)
    _, want, _ = _check_batched(ids, [c[0] for c in cases])
    assert want[:, :3].sum() > 0


def _sequential_case():
    """4 rows of 3 s against one label array; the decoded pitch 60 is held across the boundary at 3 s (row 0 ends it at index 60,
    row 1 starts it there: one run), the label pitch 62 across the one at 6 s."""
    rng = np.random.default_rng(9)
    labels, decoded = fc.random_pair(rng, max_notes=20, span=11.0)
    labels = np.concatenate([labels, fc.ref((5.5, 6.5, 62), (2.6, 3.4, 60), (11.2, 11.93, 67))])
    decoded = [n for n in decoded if n[1] // 60 == n[0] // 60] + [(50, 60, 60), (60, 70, 60), (110, 125, 62)]
    rows = [[n for n in decoded if n[0] // 60 == r] for r in range(4)]
    return labels, fc.id_rows(rows, 6 * max(len(r) for r in rows) + 1, steps_per_row=60)


def test_sequential_rows_are_one_timeline():
    label, ids = _sequential_case()
    ids_dev = torch.from_numpy(ids).cuda()
    decoded = scoring.detokenize(TOK, ids_dev, "sequential", 3).to_numpy()
    assert np.array_equal(decoded, TOK.decode(ids, mode="sequential", duration_per_batch=3)) and len(ids) == 4
    c = scoring.frame_counts(TOK, ids_dev, label, mode="sequential", duration_per_batch=3)
    want = _want([label], [decoded])
    assert c.tp.shape == (1, 1) and np.array_equal(_got(c), want), (_got(c).tolist(), want.tolist())
    assert c.frames.tolist() == [1193] and want[0, 0] > 0
    for melody_only in (False, True):
        found = scoring.error_notes(TOK, ids_dev, label, "sequential", 3, melody_only=melody_only)
        _check_notes(found, [label], [decoded], melody_only)
    tp = scoring.error_notes(TOK, ids_dev, label, "sequential", 3).to_numpy()[0][0]
    assert (2.6, 3.4, 60.0) in [tuple(n) for n in tp[:, :3].tolist()]          # the held note is one run across the row boundary
    with pytest.raises(ValueError, match="2 label arrays for 4 timelines"):
        scoring.frame_counts(TOK, ids_dev, [label] * 2)


def _threshold_case():
    """(labels, ids [4, 64], lp [4, 64]): closed groups of six ids per note, so every note has six tokens of its own; a NaN in the
    first note of row 0, -inf in its second."""
    rng = np.random.default_rng(7)
    cases = [fc.random_pair(rng, max_notes=9) for _ in range(4)]
    cases = [(l, d[:10]) for l, d in cases]
    ids = fc.id_rows([c[1] for c in cases], 64)
    lp = (-rng.exponential(0.12, ids.shape)).astype(np.float32)
    assert len(cases[0][1]) >= 2
    lp[0, 2] = np.float32(np.nan)
    lp[0, 8] = np.float32(-np.inf)
    return [c[0] for c in cases], ids, lp


def test_threshold_sweep_in_one_launch():
    labels, ids, lp = _threshold_case()
    notes, conf = confidence.decode_with_confidence(TOK, ids, lp)
    assert np.isnan(conf[0][0]) and conf[0][1] == 0.0
    flat = np.sort(np.concatenate(conf))
    flat = flat[np.isfinite(flat) & (flat > 0)]
    own = float(flat[len(flat) // 2])                          # one note lies exactly on this threshold: it is kept
    thresholds = [0.0, 0.3, own, own * (1 + 1e-5), 1.0]
    ids_dev, lp_dev = torch.from_numpy(ids).cuda(), torch.from_numpy(lp).cuda()
    c = scoring.frame_counts(TOK, ids_dev, labels, token_logprobs=lp_dev, thresholds=thresholds)
    assert c.tp.shape == (4, 5) and c.f1.shape == (5,) and c.melody_f1.shape == (5,) and c.per_timeline_f1.shape == (4, 5)
    kept_notes = []
    for k, floor in enumerate(thresholds):
        kept, _ = confidence.decode_with_confidence(TOK, ids, lp, min_confidence=floor)
        kept_notes.append(sum(len(n) for n in kept))
        want = _want(labels, kept)
        assert np.array_equal(_got(c, k), want), (floor, _got(c, k).tolist(), want.tolist())
        found = scoring.error_notes(TOK, ids_dev, labels, token_logprobs=lp_dev, min_confidence=floor)
        _check_notes(found, labels, kept, False)
    assert kept_notes[2] == kept_notes[3] + 1                  # the note on the threshold leaves one step above it
    assert kept_notes[4] == 1                                  # only the NaN total survives a threshold of 1: every other note is dropped
    assert (c.tp[1:, 4] == 0).all() and (c.fp[1:, 4] == 0).all() and c.fn[1:, 4].sum() > 0 and c.tp[0, 4] + c.fp[0, 4] > 0
    assert c.frames.tolist() == [frame_metrics.n_frames_of(l, d) for l, d in zip(labels, notes)]
    scores = evaluation.frame_scores_tokens(TOK, ids_dev, labels, token_logprobs=lp_dev, thresholds=thresholds)
    assert np.array_equal(scores["precision"], c.precision) and np.array_equal(scores["melody_tp"], c.melody_tp.sum(axis=0))
    # K = 1, 2 and 64 in one call equal K calls with one threshold each
    many = np.linspace(0.0, 1.0, 64).tolist()
    single = {}
    for sweep in ([0.4], [0.0, 0.6], many):
        c = scoring.frame_counts(TOK, ids_dev, labels, token_logprobs=lp_dev, thresholds=sweep)
        assert c.tp.shape == (4, len(sweep))
        for k, floor in enumerate(sweep):
            if floor not in single:
                single[floor] = _got(scoring.frame_counts(TOK, ids_dev, labels, token_logprobs=lp_dev, thresholds=[floor]))
            assert np.array_equal(_got(c, k), single[floor]), (len(sweep), k)
    for k in (0, 17, 40, 63):
        kept, _ = confidence.decode_with_confidence(TOK, ids, lp, min_confidence=many[k])
        assert np.array_equal(single[many[k]], _want(labels, kept)), k
    # no log-probabilities with K = 3: the one column, repeated; and it is the threshold 0
    plain = scoring.frame_counts(TOK, ids_dev, labels, thresholds=[0.0, -1.0, 0.0])
    assert plain.tp.shape == (4, 3) and all(np.array_equal(_got(plain, k), single[0.0]) for k in range(3))
    with pytest.raises(ValueError, match="65 thresholds out of range"):
        scoring.frame_counts(TOK, ids_dev, labels, token_logprobs=lp_dev, thresholds=[0.5] * 65)


def test_a_total_one_ulp_below_the_floor_is_dropped():
    """The floors go to the kernel as float32: a note whose float32 total equals the floor is kept, the same note against the next
    float32 above its total (the total is one ulp below the floor) is dropped."""
    labels, ids, lp = _threshold_case()
    ids_dev, lp_dev = torch.from_numpy(ids).cuda(), torch.from_numpy(lp).cuda()
    dn = scoring.detokenize_scored(TOK, ids_dev, lp_dev)
    decoded, parts = dn.to_numpy(), dn.note_lp_numpy()
    totals = [p[:, 0] + p[:, 1] for p in parts]
    assert all(t.dtype == np.float32 for t in totals)
    pick = np.sort(np.concatenate(totals)[np.isfinite(np.concatenate(totals))])[3]
    floors = np.asarray([pick, np.nextafter(pick, np.float32(np.inf)), np.nextafter(pick, np.float32(-np.inf))], dtype=np.float32)
    packed, offsets, label_frames = scoring._pack_labels(labels)
    out = scoring._enqueue_frame_counts(dn, torch.from_numpy(packed).cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(floors).cuda(),
                                        scoring._frame_cap(TOK, dn, None, label_frames, "test")).cpu().numpy()
    got = out[:4 * 3 * 6].reshape(4, 3, 6)
    n_kept = []
    for k, floor in enumerate(floors):
        with np.errstate(invalid="ignore"):
            kept = [d[~(t < floor)] for d, t in zip(decoded, totals)]
        n_kept.append(sum(len(n) for n in kept))
        assert np.array_equal(got[:, k], _want(labels, kept)), k
    assert n_kept[0] == n_kept[2] == n_kept[1] + 1


def test_many_runs_stay_within_the_capacity():
    """Alternating 1-frame label notes (every other frame of 2 s) on 20 pitches against alternating 5-frame decoded notes on the same
    pitches: 2000 label notes and 40 decoded notes in one timeline.  The largest kind (FN) reaches 0.85 of ``cap`` on the full roll
    (1901 of 2241 slots: every label note is a run of its own, of TP or FN) and 0.04 on the melody roll (192 of 4482)."""
    pitches = list(range(40, 60))
    labels = np.asarray([[(f + 0.2) / 100, (f + 1.2) / 100, p, 80.0] for p in pitches for f in range(p % 2, 200, 2)])
    assert all(int(s * 100) + 1 == int(e * 100) for s, e in labels[:, :2])
    decoded = [(i, i + 1, p) for p in pitches for i in (2 + p % 3, 20 + p % 5)]
    ids = fc.id_rows([decoded], 6 * len(decoded) + 1)
    ids_dev = torch.from_numpy(ids).cuda()
    got = scoring.detokenize(TOK, ids_dev).to_numpy()
    assert np.array_equal(got[0], fc.est_seconds(decoded)) and len(labels) == 2000
    c = scoring.frame_counts(TOK, ids_dev, [labels])
    assert np.array_equal(_got(c), _want([labels], got))
    for melody_only, most in ((False, 1901), (True, 192)):
        found = scoring.error_notes(TOK, ids_dev, [labels], melody_only=melody_only)
        share = _check_notes(found, [labels], got, melody_only)
        cap = native.load().m2m_score_error_notes_capacity(1, ids.shape[1], 0, len(labels), int(melody_only))
        assert found.notes.shape[2] == cap == (2 if melody_only else 1) * (2000 + ids.shape[1])
        print(f"many runs, melody_only={melody_only}: counts {found.counts.cpu().numpy().tolist()} of cap {cap}: share {share:.3f}")
        assert int(found.counts.max()) == most and share == most / cap


def _raw_error_notes(dn, labels, melody, stream=None, poison=True):
    """``m2m_score_error_notes`` called as ``scoring.error_notes`` calls it, with the workspace and the outputs filled with 0xFF
    first; (notes, counts) on the host."""
    lib = native.load()
    packed, offsets, label_frames = scoring._pack_labels(labels)
    R, L = dn.notes.shape[0], dn.notes.shape[1]
    T, max_labels = len(labels), int(np.diff(offsets).max())
    frame_cap = scoring._frame_cap(TOK, dn, None, label_frames, "test")
    cap, need = lib.m2m_score_error_notes_capacity(R, L, 0, max_labels, melody), lib.m2m_score_error_notes_workspace_bytes(T, frame_cap, melody)
    lab, off = torch.from_numpy(packed).cuda(), torch.from_numpy(offsets).cuda()
    ws = torch.full((need // 8,), -1 if poison else 0, dtype=torch.int64, device="cuda")
    notes = torch.full((T, 3, cap, 3), -1, dtype=torch.int32, device="cuda")
    counts = torch.full((T, 3), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    handle = native.stream_handle(notes.device) if stream is None else int(stream.cuda_stream)
    native.check(lib.m2m_score_error_notes(dn.notes.data_ptr(), dn.counts.data_ptr(), None, R, L, 0, TOK.time_step, lab.data_ptr(), off.data_ptr(),
                                           packed.shape[1], T, frame_cap, float("-inf"), melody, max_labels, ws.data_ptr(), need,
                                           notes.data_ptr(), counts.data_ptr(), handle), "m2m_score_error_notes")
    if stream is not None:
        stream.synchronize()
    return notes.cpu().numpy(), counts.cpu().numpy()


def test_launch_behaviour():
    frames, labels, ids = _edge_batch()
    ids_dev = torch.from_numpy(ids).cuda()
    dn = scoring.detokenize(TOK, ids_dev)
    first = scoring.frame_counts(TOK, ids_dev, labels)
    for melody in (0, 1):
        found = scoring.error_notes(TOK, ids_dev, labels, melody_only=bool(melody))
        want_notes, want_counts = found.notes.cpu().numpy(), found.counts.cpu().numpy()
        # the workspace and the outputs poisoned with 0xFF before the call; then on another stream
        side = torch.cuda.Stream()
        for stream in (None, side):
            notes, counts = _raw_error_notes(dn, labels, melody, stream)
            assert np.array_equal(counts, want_counts)
            for t in range(len(labels)):
                for q in range(3):
                    assert np.array_equal(notes[t, q, :counts[t, q]], want_notes[t, q, :counts[t, q]]), (t, q)
                    assert (notes[t, q, counts[t, q]:] == -1).all()        # nothing is written past a kind's count
    # another stream, through the Python surface; then a second call on memory the allocator hands out again, dirty
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = scoring.frame_counts(TOK, ids_dev, labels)
    side.synchronize()
    assert np.array_equal(_got(other), _got(first)) and np.array_equal(other.frames, first.frames)
    dirty = torch.full((1 << 22,), -1, dtype=torch.int32, device="cuda")
    del dirty
    again = scoring.frame_counts(TOK, ids_dev, labels)
    assert np.array_equal(_got(again), _got(first))
    assert np.array_equal(ids_dev.cpu().numpy(), ids)


def test_timelines_beyond_the_callers_bounds_get_minus_one():
    """``frame_cap`` and ``max_timeline_labels`` are the caller's bounds: a timeline beyond one of them gets -1 and no counts or notes,
    the other timelines of the call are unharmed and nothing is written past a buffer."""
    lib = native.load()
    labels = [fc.ref((0.0, 1.0, 60)), fc.ref((0.0, 30.0, 60), (1.0, 2.0, 62), (3.0, 4.0, 64))]
    ids = fc.id_rows([[(0, 10, 60)], [(0, 10, 60)]], 8)
    ids_dev = torch.from_numpy(ids).cuda()
    dn = scoring.detokenize(TOK, ids_dev)
    good = scoring.frame_counts(TOK, ids_dev, labels)
    assert good.frames.tolist() == [100, 3000]
    packed, offsets, _ = scoring._pack_labels(labels)
    lab, off = torch.from_numpy(packed).cuda(), torch.from_numpy(offsets).cuda()
    out = scoring._enqueue_frame_counts(dn, lab, off, None, 2999).cpu().numpy()          # one frame short for timeline 1
    assert out[12:].tolist() == [100, -1] and out[:6].tolist() == _got(good)[0].tolist() and out[6:12].tolist() == [0] * 6
    want = scoring.error_notes(TOK, ids_dev, labels)
    want_notes, want_counts = want.notes.cpu().numpy(), want.counts.cpu().numpy()
    for frame_cap, max_labels in ((2999, 3), (3000, 2)):
        cap, need = lib.m2m_score_error_notes_capacity(2, 8, 0, max_labels, 0), lib.m2m_score_error_notes_workspace_bytes(2, frame_cap, 0)
        ws = torch.full((need // 8,), -1, dtype=torch.int64, device="cuda")
        notes = torch.full((2, 3, cap, 3), -1, dtype=torch.int32, device="cuda")
        counts = torch.full((2, 3), -7, dtype=torch.int32, device="cuda")
        native.check(lib.m2m_score_error_notes(dn.notes.data_ptr(), dn.counts.data_ptr(), None, 2, 8, 0, TOK.time_step, lab.data_ptr(),
                                               off.data_ptr(), 4, 2, frame_cap, float("-inf"), 0, max_labels, ws.data_ptr(), need,
                                               notes.data_ptr(), counts.data_ptr(), native.stream_handle(notes.device)), "m2m_score_error_notes")
        notes, counts = notes.cpu().numpy(), counts.cpu().numpy()
        assert counts[1].tolist() == [-1, -1, -1] and (notes[1] == -1).all(), (frame_cap, max_labels)
        assert np.array_equal(counts[0], want_counts[0])
        for q in range(3):
            assert np.array_equal(notes[0, q, :counts[0, q]], want_notes[0, q, :counts[0, q]]) and (notes[0, q, counts[0, q]:] == -1).all()
    with pytest.raises(native.NativeError, match="beyond its bounds"):
        scoring.ErrorNotes(torch.from_numpy(notes).cuda(), torch.from_numpy(counts).cuda(), dn.counts, False).to_numpy()


def test_bad_rows_and_no_rows():
    labels, ids, _ = _threshold_case()
    bad = ids.copy()
    bad[2, 5] = 400
    for call in (scoring.frame_counts, lambda *a: scoring.error_notes(*a).to_numpy()):
        with pytest.raises(ValueError, match="token row 2 holds an id outside"):
            call(TOK, torch.from_numpy(bad).cuda(), labels)
    none = scoring.frame_counts(TOK, torch.zeros((0, 5), dtype=torch.long).cuda(), [])
    assert none.tp.shape == (0, 1) and none.f1.tolist() == [0.0] and none.frames.shape == (0,)
    assert scoring.error_notes(TOK, torch.zeros((0, 5), dtype=torch.long).cuda(), []).to_numpy() == []


# ------------------------------------------------------------------------------------------------ Music2MIDI
@pytest.fixture(scope="module")
def random_init_model():
    from music2midi_amd.checkpoint import load_t5_state
    from music2midi_amd.model import Music2MIDI
    geom = T5Geometry(DEFAULT_CONFIG["model"]["t5"])
    sd = synth.t5_state_dict(geom, seed=0)
    synth.perturb_layer_norms(sd, 0)
    synth.force_eos_head(sd, geom, active=340, eos_scale=1.6)
    m = Music2MIDI(copy.deepcopy(DEFAULT_CONFIG))
    load_t5_state(m.model, sd, strict=False)
    m = m.cuda().eval()
    m.config.inference["midi_grammar"] = True                  # random weights close notes only under the token grammar
    return m


def _recorded(m, call):
    """(the call's result, [(keywords, output)] of every ``model.generate`` it made)."""
    seen, real = [], m.model.generate

    def recording(*a, **kw):
        out = real(*a, **kw)
        seen.append((kw, out))
        return out
    m.model.generate = recording
    try:
        return call(), seen
    finally:
        m.model.generate = real


def _same(got, want):
    assert set(got) == set(want) == {p + k for p in ("", "melody_") for k in ("precision", "recall", "f1", "tp", "fn", "fp")}
    for name in want:
        assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (name, got[name], want[name])


def _same_midi(got, want):
    assert [(i.name, i.program) for i in got.instruments] == [(i.name, i.program) for i in want.instruments] == [("TP", 0), ("FN", 1), ("FP", 2)]
    for a, b in zip(got.instruments, want.instruments):
        assert [(n.start, n.end, n.pitch, n.velocity) for n in a.notes] == [(n.start, n.end, n.pitch, n.velocity) for n in b.notes], a.name


def test_music2midi_frame_scores(random_init_model, tmp_path):
    from music2midi_amd.input import ModelInputs
    m = random_init_model
    # a labelled batch: 16 label notes per clip, so the decode budget is 64 ids
    wav = torch.from_numpy(synth.waveform_batch(40, 2, 48000))
    idx = torch.from_numpy(synth.cond_index_batch(40, 2))
    probe = m.model.generate(ModelInputs(input_waveform=wav.cuda(), cond_index=idx.cuda()), max_length=64, midi_grammar=True)
    decoded = TOK.decode(probe.cpu().numpy())
    labels = tuple(np.concatenate([d[::2] + [0.013, 0.021, 0, 0], [[0.5, 2.5, 60, 80]] * (16 - len(d[::2]))])[:16] for d in decoded)
    assert all(len(l) == 16 for l in labels)
    inputs = ModelInputs(input_waveform=wav.cuda(), notes_batch=labels, cond_index=idx.cuda())
    plain, seen = _recorded(m, lambda: m.frame_scores_batch(inputs))
    assert len(seen) == 1 and seen[0][0]["max_length"] == 64 and "output_logprobs" not in seen[0][0] and seen[0][0]["midi_grammar"] is True
    ids = seen[0][1].cpu().numpy()
    print(f"labelled batch: {[len(d) for d in TOK.decode(ids)]} notes decoded, {plain}")
    _same(plain, evaluation.frame_scores_host(TOK, ids, labels))
    assert plain["tp"][0] > 0 and plain["fn"][0] > 0
    swept, seen = _recorded(m, lambda: m.frame_scores_batch(inputs, thresholds=[0.0, 0.4, 0.8]))
    assert len(seen) == 1 and seen[0][0]["output_logprobs"] is True and seen[0][0]["max_length"] == 64
    s_ids = seen[0][1].sequences.cpu().numpy()
    s_lp = np.concatenate([np.zeros((2, 1), dtype=np.float32), seen[0][1].logprobs.cpu().numpy()], axis=1)
    _same(swept, evaluation.frame_scores_host(TOK, s_ids, labels, token_logprobs=s_lp, thresholds=[0.0, 0.4, 0.8]))
    for name in plain:                                         # threshold 0 of the scored path is the plain path
        assert swept[name][0] == plain[name][0], name
    # ineligible labels (a velocity numpy_to_midi truncates to 0) take the host route and give the definition's dict
    bad = (labels[0], np.concatenate([labels[1][:15], [[0.5, 1.0, 64, 0.5]]]))
    assert not scoring.labels_eligible(bad)
    routed, seen = _recorded(m, lambda: m.frame_scores_batch(ModelInputs(input_waveform=wav.cuda(), notes_batch=bad, cond_index=idx.cuda())))
    _same(routed, evaluation.frame_scores_host(TOK, seen[0][1].cpu().numpy(), bad))
    # a recording of three segments
    audio = synth.waveform(33, 7 * 16000)
    notes = m.generate_notes(audio_y=audio, cond_index=[4, 2])
    label = np.concatenate([notes[::2] + [0.013, 0.021, 0, 0], [[0.5, 2.5, 60, 80]]])
    plain, seen = _recorded(m, lambda: m.frame_scores_recording(label, audio_y=audio, cond_index=[4, 2]))
    assert len(seen) == 1 and seen[0][1].shape[0] == 3
    _same(plain, evaluation.frame_scores_host(TOK, seen[0][1].cpu().numpy(), label, "sequential", 3))
    assert tuple(int(plain[k][0]) for k in KEYS) == frame_metrics.frame_counts(label, notes)
    swept, seen = _recorded(m, lambda: m.frame_scores_recording(label, audio_y=audio, cond_index=[4, 2], thresholds=[0.0, 0.5, 1.0]))
    s_ids = seen[0][1].sequences.cpu().numpy()
    s_lp = np.concatenate([np.zeros((3, 1), dtype=np.float32), seen[0][1].logprobs.cpu().numpy()], axis=1)
    _same(swept, evaluation.frame_scores_host(TOK, s_ids, label, "sequential", 3, token_logprobs=s_lp, thresholds=[0.0, 0.5, 1.0]))
    print(f"recording: {len(notes)} notes, {swept}")
    for name in plain:
        assert swept[name][0] == plain[name][0], name
    # the error MIDI of the recording: the definition's three instruments, and they survive a file
    for melody_only in (False, True):
        midi = m.error_midi_recording(label, audio_y=audio, cond_index=[4, 2], melody_only=melody_only)
        _same_midi(midi, evaluation.evaluate_midi_result(label, notes, melody_only))
    kept, _ = confidence.decode_with_confidence(TOK, s_ids, s_lp, "sequential", 3, 0.5)
    _same_midi(m.error_midi_recording(label, audio_y=audio, cond_index=[4, 2], min_confidence=0.5), evaluation.evaluate_midi_result(label, kept))
    midi.write(tmp_path / "errors.mid")
    data = (tmp_path / "errors.mid").read_bytes()
    assert data[:4] == b"MThd" and data[8:12] == bytes([0, 1, 0, 4]) and data.count(b"MTrk") == 4
