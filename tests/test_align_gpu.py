"""GPU: the aligner's kernels (csrc/align.hip) EQUAL to the definition (music2midi_amd/align.py) on identical inputs - features with
planted ties and short clips, DTW totals, paths and lengths at every size around the strip width - and the whole device path held
to the planted truth of align_cases.py."""
import numpy as np
import pytest
import torch

from music2midi_amd import align

from align_cases import CAP_SECONDS, CASES, case, onset_error

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ m2m_align_features
def _planted_L(rng, frames):
    """Random log energies with exact ties at every threshold, silent frames and a frame at exactly -6.0."""
    L = rng.uniform(-9.0, 2.0, (frames, 88)).astype(np.float32)
    for t in range(0, frames, 3):
        M = L[t].max()
        bands = rng.choice(np.flatnonzero(L[t] < M), 8, replace=False)
        for k in range(4):
            L[t, bands[k]] = M - align.D_THRESH[k]                             # L == M - d[k]: the comparison must hold
            L[t, bands[4 + k]] = np.nextafter(M - align.D_THRESH[k], np.float32(-100))     # one ulp below: it must not
    if frames > 12:
        L[5] = rng.uniform(-13.8, -6.5, 88)                                    # silent
        L[6] = -13.815511
        L[9] = np.minimum(L[9], np.float32(-6.0))
        L[9, 40] = -6.0                                                        # M == -6.0 exactly: silent
        L[10] = np.minimum(L[10], np.float32(-6.5))
        L[10, 41] = np.nextafter(np.float32(-6.0), np.float32(0))              # one ulp above: not silent
        t = 11                                                                 # a rise of exactly ln 4, and one ulp less
        L[t, 20], L[t, 21] = L[t - 2, 20] + align.ONSET_RISE, np.nextafter(L[t - 2, 21] + align.ONSET_RISE, np.float32(-100))
    return L


def test_features_equal_the_definition():
    rng = np.random.default_rng(0)
    clips = [_planted_L(rng, f) for f in (1, 2, 3, 1025, 4, 7, 33, 64, 65)]    # 32 frames per workgroup: 33, 64, 65 cross its edge
    # onsets that begin in the last frames of one workgroup and tail into the next
    clips[3][30:34, :] = -9.0
    clips[3][32:, 50] = 1.5
    got = align.align_features(clips)
    for k, (L, (chroma, onset)) in enumerate(zip(clips, got)):
        want = align.features_host(L)
        assert chroma.dtype == onset.dtype == torch.uint8 and chroma.is_cuda
        assert np.array_equal(chroma.cpu().numpy(), want[0]), (k, len(L))
        assert np.array_equal(onset.cpu().numpy(), want[1]), (k, len(L))
    want = align.features_host(clips[3])
    assert want[0].max() > 8 and want[1].max() >= 4 and not want[0][5].any() and not want[0][9].any() and want[0][10].any()
    one = align.align_features(clips[3])
    assert np.array_equal(one[0].cpu().numpy(), want[0]) and np.array_equal(one[1].cpu().numpy(), want[1])


# ------------------------------------------------------------------ m2m_align_dtw
def _random_features(rng, n, coarse=False):
    if coarse:
        f = rng.integers(0, 673, (n, 12)).astype(np.int32)
        f[rng.random(n) < 0.1] = 0
        return f
    chroma = (rng.integers(0, 33, (n, 12)) * (rng.random((n, 12)) < 0.4)).astype(np.uint8)
    onset = (rng.integers(0, 33, (n, 12)) * (rng.random((n, 12)) < 0.1)).astype(np.uint8)       # mostly zero vectors, as real onsets are
    return chroma, onset


def _check(got, want, what):
    assert got[0] == want[0], (what, got[0], want[0])
    assert got[1].dtype == np.int32 and got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), what


def _sizes():
    Ws = align.strip_width()                                                   # columns of a strip of the kernel
    return [(1, 1), (1, 7), (7, 1), (2, 2), (5, 300), (300, 5), (Ws - 1, Ws - 1), (Ws, Ws), (Ws + 1, Ws + 1), (2 * Ws + 1, 2 * Ws + 1), (Ws + 1, 3)]


def test_dtw_sizes_and_feature_kinds_in_one_batch():
    """Zero features (cost 512 everywhere: every cell a tie), identical sides (a pure diagonal) and random ones at every size, as ONE
    launch of mixed sizes - the smallest problem sits next to the largest."""
    rng = np.random.default_rng(1)
    sizes = _sizes()
    sizes = sizes[:1] + sizes[-2:-1] + sizes[1:-2] + sizes[-1:]                # 1 x 1 next to (2 Ws + 1)^2
    fa, fb, kinds = [], [], []
    for n, m in sizes:
        zero = (np.zeros((n, 12), np.uint8), np.zeros((n, 12), np.uint8)), (np.zeros((m, 12), np.uint8), np.zeros((m, 12), np.uint8))
        ra, rb = _random_features(rng, n), _random_features(rng, m)
        sa = tuple(rng.integers(1, 33, (n, 12)).astype(np.uint8) for _ in range(2))          # no zero vector: equal frames cost 0
        same = (sa, sa) if n == m else (sa, tuple(x[np.minimum(np.arange(m) * n // m, n - 1)] for x in sa))
        for kind, (a, b) in (("zero", zero), ("same", same), ("random", (ra, rb))):
            fa.append(a), fb.append(b), kinds.append((kind, n, m))
    got = align.dtw(fa, fb)
    assert len(got) == 3 * len(sizes)
    for g, a, b, what in zip(got, fa, fb, kinds):
        want = align.dtw_features_host(a, b)
        _check(g, want, what)
        kind, n, m = what
        if kind == "zero":
            assert g[0] == 512 * (4 * min(n, m) + 3 * abs(n - m))
        if kind == "same" and n == m:
            assert g[0] == 0 and np.array_equal(g[1], np.stack([np.arange(n), np.arange(n)]))


def test_dtw_every_shift_and_single_call():
    rng = np.random.default_rng(2)
    a, b = _random_features(rng, 70), _random_features(rng, 90)
    got = align.dtw([a] * 12, [b] * 12, shift=list(range(12)))
    for s in range(12):
        _check(got[s], align.dtw_features_host(a, b, s), s)
        _check(align.dtw_features_host(a, (np.roll(b[0], s, axis=1), np.roll(b[1], s, axis=1))), got[s], s)
    assert len({g[0] for g in got}) > 6                                        # the shift matters
    _check(align.dtw(a, b, shift=5), got[5], "one problem")
    ca, cb = _random_features(rng, 40, True), _random_features(rng, 55, True)
    got = align.dtw([ca] * 12, [cb] * 12, shift=list(range(12)), coarse=True)
    for s in range(12):
        _check(got[s], align.dtw_features_host(ca, cb, s, True), ("coarse", s))
    with pytest.raises(ValueError, match="32768"):
        align.dtw(np.zeros((0, 12), np.int32), ca, coarse=True)


def test_dtw_coarse_features_at_their_largest_value():
    """672 in every class: 65536 * (12 * 672^2)^2 = 1.93e18, the bound of the 64-bit arithmetic."""
    Ws = align.strip_width()
    rng = np.random.default_rng(3)
    top = np.full((Ws + 9, 12), 672, np.int32)
    near = top.copy()
    near[rng.random(near.shape) < 0.05] = 671
    mixed = _random_features(rng, 100, True)
    mixed[::3] = 672
    got = align.dtw([top, top, mixed], [top[:77], near, top[:60]], coarse=True)
    _check(got[0], align.dtw_features_host(top, top[:77], 0, True), "top")
    _check(got[1], align.dtw_features_host(top, near, 0, True), "near")
    _check(got[2], align.dtw_features_host(mixed, top[:60], 0, True), "mixed")
    assert got[0][0] == 0


def test_dtw_4096_square():
    """One problem of 4096 x 4096 random features: 8 strips, 4 MiB of direction bits, a path of thousands of points.  (The definition
    takes a few seconds in numpy.)"""
    rng = np.random.default_rng(4)
    a, b = _random_features(rng, 4096), _random_features(rng, 4096)
    _check(align.dtw(a, b, shift=7), align.dtw_features_host(a, b, 7), "4096")


def test_dtw_on_another_stream_and_twice():
    rng = np.random.default_rng(5)
    a, b = _random_features(rng, 700), _random_features(rng, 520)
    first = align.dtw(a, b, shift=2)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = align.dtw(a, b, shift=2)
    side.synchronize()
    again = align.dtw(a, b, shift=2)
    _check(other, first, "stream")
    _check(again, first, "second call")
    assert first[1].tobytes() == again[1].tobytes() == other[1].tobytes()
    _check(first, align.dtw_features_host(a, b, 2), "definition")


# ------------------------------------------------------------------ the whole device path
def _differing_feature_bytes(y):
    dev = torch.device("cuda", torch.cuda.current_device())
    L, frames = align._band_log_energies_device([torch.from_numpy(y).to(dev)], dev)
    chroma, onset = align._features_device(L, frames, dev)
    want = align.features_host(align.band_log_energies_host(y))
    assert frames == [len(want[0])]
    host_L = align.band_log_energies_host(y)
    loud = host_L > -10
    print(f"  log band energies: max |device - host| {np.abs(L.cpu().numpy() - host_L)[loud].max():.2e} over the bands above -10")
    differ = (chroma.cpu().numpy() != want[0]).sum() + (onset.cpu().numpy() != want[1]).sum()
    return differ / (2 * want[0].size)


def test_align_batch_finds_the_planted_shift_and_curve():
    """Held to the truth, not to the definition: the band energies come from the frontend kernel and differ from numpy's in the last
    bits, so a few quantised features, and with them the path, may differ.  Three pairs of different lengths, one launch per stage."""
    specs = (CASES[0], CASES[-1], CASES[3])
    cases = [case(*s) for s in specs]
    cases[2] = dict(cases[2], audio=np.concatenate([cases[2]["audio"], np.zeros(9000, np.float32)]))       # a third length: silence at the end
    results = align.align_batch([c["audio"] for c in cases], [c["cover"] for c in cases])
    for spec, c, r in zip(specs, cases, results):
        err = onset_error(r, c)
        print(f"{spec}: shift {r.opt_chroma_shift}, median onset error {1000 * err:.1f} ms, {len(r.notes)} of {len(c['truth'])} notes, total {r.total_cost}")
        print(f"  feature bytes that differ from the definition's: {_differing_feature_bytes(c['audio']):.5f}")
        assert isinstance(r, align.AlignResult) and r.opt_chroma_shift == c["shift"]
        assert err <= CAP_SECONDS
        assert (np.diff(r.warp_path, axis=1) > 0).all() and set(r.metrics) == {"wp_std", "time_diff_ratio"}


def test_align_notes_one_pair_other_rate_and_host_routes():
    c = case(*CASES[1])
    r = align.align_notes(c["audio"], c["cover"])
    err = onset_error(r, c)
    print(f"{CASES[1]}: shift {r.opt_chroma_shift}, median onset error {1000 * err:.1f} ms")
    assert r.opt_chroma_shift == c["shift"] and err <= CAP_SECONDS
    from music2midi_amd import audio
    r16 = align.align_notes(torch.from_numpy(audio.resample(c["audio"], 22050, 16000)).cuda(), c["cover"], sr=16000)
    assert r16.opt_chroma_shift == c["shift"] and onset_error(r16, c) <= CAP_SECONDS
    # no notes, and audio that is not finite, go through the definition
    empty = align.align_notes(c["audio"], np.zeros((0, 4)))
    assert empty.notes.shape == (0, 4) and empty.opt_chroma_shift == 0
    bad = c["audio"].copy()
    bad[100] = np.inf
    assert isinstance(align.align_notes(bad, c["cover"]), align.AlignResult)
