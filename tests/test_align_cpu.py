"""CPU: the definition of the aligner (music2midi_amd/align.py) on hand-made inputs with the results worked out by hand, its quality on
the seeded cases of align_cases.py, and what the library answers on its arguments alone."""
import ctypes as C
import math

import numpy as np
import pytest

from music2midi_amd import align, native

from align_cases import CAP_SECONDS, CASES, DENSE_CASE, case, onset_error

M2M_ERR_INVALID = -1


# ------------------------------------------------------------------ the first stage
def test_pitch_filterbank():
    fb = align.pitch_filterbank()
    assert fb.dtype == np.float32 and fb.shape == (1025, 88) and fb.min() >= 0 and fb.max() <= 1
    f = np.arange(1025) * 22050 / 2048
    col = fb[:, 69 - 21]                                                       # A4: zero at G#4 and A#4 and beyond, its peak next to 440 Hz
    inside = (f > 440 * 2 ** (-1 / 12)) & (f < 440 * 2 ** (1 / 12))
    assert (col[inside] > 0).all() and not col[~inside].any() and abs(f[np.argmax(col)] - 440) <= 22050 / 2048 / 2 + 1e-9
    k = int(np.argmax(col))
    assert abs(col[k] - (1 - abs(f[k] - 440) / (440 - 440 * 2 ** (-1 / 12) if f[k] < 440 else 440 * 2 ** (1 / 12) - 440))) < 1e-6
    assert not fb[:, 0].any()                                                  # pitch 21: 25.96..29.14 Hz holds no bin of 10.77 Hz spacing
    assert fb[:, 87].any() and np.count_nonzero(fb[:, 87]) <= 48               # the widest band fits the frontend's 48 taps


def test_band_log_energies_of_a_sine():
    t = np.arange(22050) / 22050
    L = align.band_log_energies_host(np.sin(2 * np.pi * 440 * t).astype(np.float32))
    assert L.dtype == np.float32 and L.shape == (51, 88) and align.num_frames(22050) == 51
    assert (np.argmax(L[2:-2], axis=1) == 69 - 21).all()
    assert np.array_equal(align.band_log_energies_host(np.zeros(4000, np.float32)), np.full((10, 88), np.log(np.float32(1e-6)), np.float32))
    with pytest.raises(ValueError, match="1025"):
        align.band_log_energies_host(np.zeros(1024, np.float32))


# ------------------------------------------------------------------ the features
def test_features_by_hand():
    floor = np.float32(-13.8)
    L = np.full((8, 88), floor, dtype=np.float32)
    L[2:, 0] = 0.0                                                             # pitch 21, class 9, from frame 2 on
    L[4, 12] = np.float32(0.0) - align.D_THRESH[1]                             # pitch 33, class 9: exactly M - ln 5, so ln 5, ln 10 and ln 20 hold
    chroma, onset = align.features_host(L)
    assert chroma.dtype == onset.dtype == np.uint8 and chroma.shape == onset.shape == (8, 12)
    want = np.zeros((8, 12), np.uint8)
    want[2:, 9] = 4
    want[4, 9] = 4 + 3                                                         # L >= M - d[k] for k = 1, 2, 3 (the tie at k = 1 counts)
    assert np.array_equal(chroma, want)
    # on[2][0] (rise 13.8 >= ln 4) is a first; on[3][0] holds too but on[2][0] did: no first.  Frame 4: band 12 rises by 13.8 - ln 5 and
    # lies above M - ln 20: a first.  on[5][12] fails (L falls back).  The tail is 4, 3, 2, 1 after each first.
    want = np.zeros((8, 12), np.uint8)
    want[2:6, 9] = [4, 3, 2, 1]
    want[4:8, 9] = np.maximum(want[4:8, 9], [4, 3, 2, 1])
    assert np.array_equal(onset, want)
    # a frame at exactly -6.0 is silent, one just above is not
    L = np.full((2, 88), floor, dtype=np.float32)
    L[0, 5], L[1, 5] = -6.0, np.nextafter(np.float32(-6.0), np.float32(0))
    chroma, _ = align.features_host(L)
    assert not chroma[0].any() and chroma[1, (21 + 5) % 12] == 4 and chroma[1].sum() == 4
    assert all(x.shape == (0, 12) for x in align.features_host(np.zeros((0, 88), np.float32)))
    assert [float(x).hex() for x in align.D_THRESH] == ["0x1.d524100000000p-1", "0x1.9c04200000000p+0", "0x1.26bb1c0000000p+1", "0x1.7f74280000000p+1"]
    assert float(align.ONSET_RISE).hex() == "0x1.62e4300000000p+0"            # the literals csrc/align.hip writes out


def test_coarse_by_hand():
    got = align.coarse(np.ones((25, 12), np.uint8))
    assert got.dtype == np.int32 and got.shape == (3, 12) and got[:, 0].tolist() == [11, 21, 15] and (got == got[:, :1]).all()
    assert align.coarse(np.full((1, 12), 32, np.uint8)).tolist() == [[32] * 12]
    assert align.coarse(np.full((400, 12), 32, np.uint8)).max() == 672         # the bound the cost's 64-bit arithmetic rests on
    ramp = np.arange(40)[:, None] * np.ones((1, 12), np.int64)
    assert align.coarse(ramp.astype(np.uint8))[:, 3].tolist() == [sum(range(0, 11)), sum(range(0, 21)), sum(range(10, 31)), sum(range(20, 40))]


# ------------------------------------------------------------------ the cost
def _unit(*pairs):
    v = np.zeros(12, np.int64)
    for c, x in pairs:
        v[c] = x
    return v


def test_cost_by_hand():
    assert align.cost(_unit((0, 1), (1, 2)), _unit((0, 2), (1, 4))) == 0       # parallel
    assert align.cost(_unit((0, 3)), _unit((5, 7))) == 256                     # orthogonal
    assert align.cost(np.zeros(12), _unit((2, 9))) == 256 and align.cost(_unit((2, 9)), np.zeros(12)) == 256 and align.cost(np.zeros(12), np.zeros(12)) == 256
    assert align.cost(_unit((0, 1)), _unit((0, 1), (1, 1))) == 256 - 181       # 65536 // 2 = 32768, 181^2 = 32761 <= 32768 < 182^2
    assert align.cost(np.full(12, 672), np.full(12, 672)) == 0                 # 65536 * (12 * 672^2)^2 = 1.93e18 < 2^63
    assert 65536 * (12 * 672 ** 2) ** 2 < 2 ** 63


def test_cost_matrix_against_python_integers():
    rng = np.random.default_rng(0)
    A = np.concatenate([rng.integers(0, 673, (20, 12)), np.full((1, 12), 672), np.zeros((1, 12), np.int64), rng.integers(0, 3, (8, 12)),
                        np.concatenate([np.full((1, 11), 672), [[671]]], axis=1)])
    Cm = align.cost_matrix(A, A)
    assert Cm.dtype == np.int32 and Cm.shape == (31, 31)
    for i in range(31):
        for j in range(31):
            u, v = [int(x) for x in A[i]], [int(x) for x in A[j]]
            dot, den = sum(a * b for a, b in zip(u, v)), sum(a * a for a in u) * sum(b * b for b in v)
            assert Cm[i, j] == (256 if den == 0 else 256 - math.isqrt(65536 * dot * dot // den)), (i, j)
    assert Cm.min() >= 0 and Cm.max() == 256
    pair = (rng.integers(0, 33, (5, 12)).astype(np.uint8), rng.integers(0, 33, (5, 12)).astype(np.uint8))
    full = align.feature_cost_host(pair, pair, shift=4)
    assert np.array_equal(full, align.cost_matrix(pair[0], np.roll(pair[0], 4, axis=1)) + align.cost_matrix(pair[1], np.roll(pair[1], 4, axis=1)))


# ------------------------------------------------------------------ DTW
def test_dtw_three_by_three_by_hand():
    # D = [[0, 27, 54], [0, 27, 54], [27, 0, 0]]: (1, 1) comes from the left (27 < 36 < 54), (2, 1) from the diagonal, (2, 2) from the left
    total, path = align.dtw_host(np.array([[0, 9, 9], [0, 9, 9], [9, 0, 0]]))
    assert total == 0 and path.dtype == np.int32 and path.tolist() == [[0, 1, 2, 2], [0, 0, 1, 2]]
    total, path = align.dtw_host(np.array([[1, 5, 5], [5, 1, 5], [5, 5, 1]]))
    assert total == 12 and path.tolist() == [[0, 1, 2], [0, 1, 2]]


def test_dtw_all_equal_costs_tie_to_the_diagonal():
    # every inner cell ties between the diagonal and an edge step: 3 x 3 is the diagonal, 3 * 4 = 12
    total, path = align.dtw_host(np.ones((3, 3), np.int64))
    assert total == 12 and path.tolist() == [[0, 1, 2], [0, 1, 2]]
    # 2 x 4: D[0] = 4, 7, 10, 13; D[1] = 7, 8, 11 (diagonal 7 + 4 ties with left 8 + 3), 14 (diagonal 10 + 4 ties with left 11 + 3).
    # From the end the ties take the diagonal, then the edge of row 0 is forced.
    total, path = align.dtw_host(np.ones((2, 4), np.int64))
    assert total == 14 and path.tolist() == [[0, 0, 0, 1], [0, 1, 2, 3]]
    total, path = align.dtw_host(np.ones((4, 2), np.int64))
    assert total == 14 and path.tolist() == [[0, 1, 2, 3], [0, 0, 0, 1]]
    # (i-1, j) before (i, j-1): D[1][1] of [[1, 1], [1, 9]] is min(4 + 36, 7 + 27, 7 + 27): the two edges tie, up wins
    total, path = align.dtw_host(np.array([[1, 1], [1, 9]]))
    assert total == 34 and path.tolist() == [[0, 0, 1], [0, 1, 1]]


def test_dtw_single_rows_and_columns():
    assert align.dtw_host(np.array([[7]]))[0] == 28 and align.dtw_host(np.array([[7]]))[1].tolist() == [[0], [0]]
    total, path = align.dtw_host(np.array([[1, 2, 3, 4, 5]]))
    assert total == 4 * 1 + 3 * (2 + 3 + 4 + 5) and path.tolist() == [[0] * 5, [0, 1, 2, 3, 4]]
    total, path = align.dtw_host(np.array([[1], [2], [3], [4], [5]]))
    assert total == 46 and path.tolist() == [[0, 1, 2, 3, 4], [0] * 5]
    with pytest.raises(ValueError):
        align.dtw_host(np.zeros((0, 3)))


def test_dtw_against_a_plain_loop():
    rng = np.random.default_rng(1)
    for n, m in ((6, 9), (9, 6), (17, 17)):
        Cm = rng.integers(0, 4, (n, m))                                        # small values: many ties
        D = np.full((n + 1, m + 1), 10 ** 9, np.int64)
        D[0, 0] = 0
        step = np.zeros((n, m), int)
        for i in range(n):
            for j in range(m):
                cands = [D[i, j] + 4 * Cm[i, j], D[i, j + 1] + 3 * Cm[i, j], D[i + 1, j] + 3 * Cm[i, j]]
                step[i, j] = int(np.argmin(cands))                            # the first minimum: diagonal, up, left
                D[i + 1, j + 1] = min(cands)
        i, j, want = n - 1, m - 1, []
        while True:
            want.append((i, j))
            if (i, j) == (0, 0):
                break
            i, j = [(i - 1, j - 1), (i - 1, j), (i, j - 1)][step[i, j]]
        total, path = align.dtw_host(Cm)
        assert total == D[n, m] and path.T.tolist() == [list(x) for x in want[::-1]]


def test_shift_search_by_hand():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 33, (120, 12)).astype(np.uint8)
    for s in (0, 1, 6, 7, 11):
        found, totals = align.optimal_shift_host(np.roll(a, s, axis=1), a)
        assert found == s and totals[s] == 0 and len(totals) == 12
    assert align.optimal_shift_host(np.zeros((30, 12), np.uint8), a)[0] == 0   # all ties: the smallest s
    assert [align.semitones(s) for s in range(12)] == [0, 1, 2, 3, 4, 5, 6, -5, -4, -3, -2, -1]


# ------------------------------------------------------------------ the path and the notes
def test_strictly_monotonic():
    path = np.array([[0, 0, 1, 2, 2, 3], [0, 1, 1, 2, 3, 4]])
    assert align.strictly_monotonic(path).tolist() == [[0, 1, 2, 3], [0, 1, 2, 4]]
    assert align.strictly_monotonic(np.array([[5], [7]])).tolist() == [[5], [7]]
    assert align.strictly_monotonic(np.array([[0, 0, 0], [0, 1, 2]])).tolist() == [[0], [0]]


def test_apply_warp_drops_clamps_and_collapses():
    wp = np.array([[-0.5, 0.5, 2.5], [1.0, 2.0, 3.0]])                          # [0] the recording's clock, [1] the notes'
    notes = np.array([[0.5, 1.5, 60, 80],                                      # begins before the path: dropped
                      [1.0, 2.0, 61, 81],                                      # -0.5 -> clamped to 0; ends at 0.5
                      [1.0, 1.2, 62, 82],                                      # -0.5 and -0.3, both clamped to 0: collapses, dropped
                      [2.0, 3.0, 63, 83],                                      # 0.5 .. 2.5
                      [2.25, 2.5, 64, 84],                                     # 1.0 .. 1.5
                      [2.5, 3.5, 65, 85]])                                     # ends after the path: dropped
    got = align.apply_warp(notes, wp)
    assert got.dtype == np.float64 and got.tolist() == [[0.0, 0.5, 61, 81], [0.5, 2.5, 63, 83], [1.0, 1.5, 64, 84]]
    assert align.apply_warp(np.zeros((0, 4)), wp).shape == (0, 4)
    m = align.warp_metrics(np.array([[0.0, 1.0, 2.0], [0.0, 0.5, 1.0]]), 2.0, np.array([[0.0, 1.5, 60, 80], [0.2, 0.4, 60, 80]]))
    assert set(m) == {"wp_std", "time_diff_ratio"} and m["wp_std"] == np.std([0.0, 0.5, 1.0]) and m["time_diff_ratio"] == 0.25
    assert align.transpose(np.array([[0, 1, 125, 80], [0, 1, 3, 80], [0, 1, 60, 80]]), 5)[:, 2].tolist() == [8, 65]      # 130 leaves 0..127
    assert align.transpose(np.array([[0, 1, 125, 80], [0, 1, 3, 80]]), 8)[:, 2].tolist() == [121]                        # -4 semitones: -1 leaves


# ------------------------------------------------------------------ the C ABI
def test_binding_matches_the_header():
    lib = native.load()
    header = (native._LIB_PATH.parents[2] / "include" / "music2midi_amd.h").read_text()
    for name in ("m2m_align_features", "m2m_align_coarse", "m2m_align_dtw_strip", "m2m_align_dtw_workspace_bytes", "m2m_align_dtw"):
        assert name in native.EXPORTED_SYMBOLS and hasattr(lib, name) and f" {name}(" in header, name
        decl = header[header.index(f" {name}("):]
        decl = decl[:decl.index(";")]
        assert decl.count(",") + (0 if "(void)" in decl else 1) == len(native._SIGNATURES[name][1]), name
    assert C.sizeof(native.AlignProblem) == 24 and [n for n, _ in native.AlignProblem._fields_] == ["a_offset", "n", "b_offset", "m", "shift", "path_offset"]
    assert "#define M2M_ABI_VERSION 1" in header and lib.m2m_abi_version() == 1
    ws = lib.m2m_align_dtw_strip()
    assert ws == align.strip_width() and 64 <= ws <= 1024 and ws % 64 == 0
    assert align.MAX_FRAMES == 32768 and "#define M2M_ALIGN_MAX_FRAMES 32768" in header


def _sizes(rows, cols):
    r, c = np.asarray(rows, np.int32), np.asarray(cols, np.int32)
    return native.load().m2m_align_dtw_workspace_bytes(r.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), len(r))


def test_workspace_bytes_and_its_refusals():
    # the table (256 bytes), then per problem ceil(n / 16) * m + 2 (n + m) dwords rounded up to 64
    assert _sizes([1], [1]) == 256 + 4 * 64
    assert _sizes([12000], [12000]) == 256 + 4 * ((750 * 12000 + 48000 + 63) // 64 * 64)           # 36 MB of direction bits
    assert _sizes([32768], [32768]) == 256 + 4 * (2048 * 32768 + 131072)                            # 256 MiB at the size limit
    assert _sizes([17, 1], [5, 300]) == 256 + 4 * (64 + 960)
    for rows, cols in (([0], [5]), ([5], [0]), ([32769], [5]), ([5], [32769]), ([5, -1], [5, 5])):
        assert _sizes(rows, cols) == M2M_ERR_INVALID, (rows, cols)
        assert b"m2m_align_dtw_workspace_bytes" in native.load().m2m_last_error()


def test_every_refusal_is_made_without_a_gpu():
    """M2M_ERR_INVALID on the arguments alone: the pointers are never dereferenced, no HIP call is made."""
    lib = native.load()
    buf = (C.c_float * 4096)()
    a = (C.addressof(buf) + 255) // 256 * 256                                  # never touched: only compared
    ok = dict(a0=a, a1=a + 1024, fa=100, b0=a + 2048, b1=a + 3072, fb=80, coarse=0, P=1, ws=a + 4096, wsb=1 << 20, tot=a + 8192, path=a + 8448,
              cap=179, plen=a + 12288, prob=(0, 100, 0, 80, 0, 0))

    def call(**change):
        k = dict(ok, **change)
        probs = None if k["prob"] is None else (native.AlignProblem * 1)(native.AlignProblem(*k["prob"]))
        return lib.m2m_align_dtw(k["a0"], k["a1"], k["fa"], k["b0"], k["b1"], k["fb"], k["coarse"], probs, k["P"], k["ws"], k["wsb"], k["tot"],
                                 k["path"], k["cap"], k["plen"], None)
    bad = [dict(prob=(0, 0, 0, 80, 0, 0)), dict(prob=(0, 100, 0, 0, 0, 0)), dict(prob=(0, 32769, 0, 80, 0, 0), fa=40000, cap=40000),
           dict(prob=(0, 100, 0, 32769, 0, 0), fb=40000, cap=40000), dict(prob=(1, 100, 0, 80, 0, 0)), dict(prob=(0, 100, 1, 80, 0, 0)),
           dict(prob=(-1, 100, 0, 80, 0, 0)), dict(prob=(0, 100, 0, 80, 12, 0)), dict(prob=(0, 100, 0, 80, -1, 0)), dict(prob=(0, 100, 0, 80, 0, 1)),
           dict(prob=(0, 100, 0, 80, 0, -1)), dict(cap=178), dict(cap=0), dict(P=0), dict(P=65536), dict(coarse=2), dict(fa=0), dict(a0=None),
           dict(b1=None), dict(ws=None), dict(tot=None), dict(path=None), dict(plen=None), dict(prob=None), dict(a0=a + 2), dict(coarse=1, b0=a + 2052),
           dict(ws=a + 4100), dict(tot=a + 8193)]
    for change in bad:
        assert call(**change) == M2M_ERR_INVALID, change
        assert b"m2m_align_dtw" in lib.m2m_last_error(), change
    assert call(wsb=1000) == -3 and b"needed" in lib.m2m_last_error()        # M2M_ERR_NOMEM
    for fn, args in ((lib.m2m_align_features, (a, a + 1024, 0, 5, 5, a + 2048, a + 3072, None)),
                     (lib.m2m_align_features, (a, a + 1024, 1, 6, 5, a + 2048, a + 3072, None)),
                     (lib.m2m_align_features, (a, a + 1024, 1, 5, 0, a + 2048, a + 3072, None)),
                     (lib.m2m_align_features, (a, None, 1, 5, 5, a + 2048, a + 3072, None)),
                     (lib.m2m_align_features, (a + 2, a + 1024, 1, 5, 5, a + 2048, a + 3072, None)),
                     (lib.m2m_align_coarse, (a, a + 1024, a + 1100, 1, 1, 5, 1, 0, 10, a + 2048, None)),
                     (lib.m2m_align_coarse, (a, a + 1024, a + 1100, 1, 1, 5, 1, 21, 256, a + 2048, None)),
                     (lib.m2m_align_coarse, (a, a + 1024, a + 1100, 1, 2, 5, 1, 21, 10, a + 2048, None)),
                     (lib.m2m_align_coarse, (a, a + 1024, a + 1100, 1, 1, 5, 6, 21, 10, a + 2048, None)),
                     (lib.m2m_align_coarse, (None, a + 1024, a + 1100, 1, 1, 5, 1, 21, 10, a + 2048, None))):
        assert fn(*args) == M2M_ERR_INVALID, args


# ------------------------------------------------------------------ the quality of the definition
@pytest.mark.parametrize("spec", CASES, ids=lambda s: f"seed{s[0]}-{int(s[1])}s-shift{s[2]}")
def test_definition_finds_the_planted_shift_and_curve(spec):
    c = case(*spec)
    assert len(c["truth"]) <= spec[3] * spec[1]
    result = align.align_notes_host(c["audio"], c["cover"])
    err = onset_error(result, c)
    print(f"{spec}: {len(c['truth'])} notes, shift {result.opt_chroma_shift}, median onset error {1000 * err:.1f} ms, {len(result.notes)} notes kept, "
          f"total {result.total_cost}, {result.metrics}")
    assert result.opt_chroma_shift == c["shift"]
    assert err <= CAP_SECONDS
    wp = result.warp_path
    assert wp.shape[0] == 2 and (np.diff(wp, axis=1) > 0).all() and wp[0, 0] == 0 and wp[1, 0] == 0
    assert len(result.notes) >= 0.9 * len(c["truth"])
    assert set(result.notes[:, 2]) <= set(c["truth"][:, 2])                                  # transposed back to the recording's key
    assert result.metrics["wp_std"] < 5 and result.metrics["time_diff_ratio"] < 0.2          # config.dataset.filter_threshold


def test_shift_margins_of_the_cases():
    """The cases were chosen with second-best / best of the shift search's totals at least 1.25; this keeps them so."""
    for spec in CASES[:2] + CASES[-1:]:
        c = case(*spec)
        fa = align.features_host(align.band_log_energies_host(c["audio"]))
        z = align.render.render_host(c["cover"], align.FS, align.notes_length(c["cover"]), normalize=True)
        fb = align.features_host(align.band_log_energies_host(z))
        s, totals = align.optimal_shift_host(fa[0], fb[0])
        best, second = sorted(totals)[:2]
        print(f"{spec}: totals {totals}, margin {second / max(best, 1):.2f}")
        assert s == c["shift"] and second >= 1.25 * best


def test_dense_case_is_a_documented_limit():
    """Six random notes per second: the case exists and runs; nothing is asserted about its alignment (align_cases.DENSE_CASE)."""
    c = case(*DENSE_CASE)
    assert len(c["truth"]) == 180
    result = align.align_notes_host(c["audio"], c["cover"])
    print(f"dense: shift {result.opt_chroma_shift} (planted {c['shift']}), median onset error {1000 * onset_error(result, c):.1f} ms")
    assert isinstance(result, align.AlignResult) and 0 <= result.opt_chroma_shift <= 11


def test_pairs_the_device_would_not_take_run_in_the_definition():
    c = case(*CASES[0])
    empty = align.align_notes_host(c["audio"], np.zeros((0, 4)))
    assert empty.notes.shape == (0, 4) and empty.opt_chroma_shift == 0 and empty.total_cost > 0
    from music2midi_amd import audio
    other_rate = align.align_notes_host(audio.resample(c["audio"], 22050, 16000), c["cover"], sr=16000)
    assert other_rate.opt_chroma_shift == c["shift"]
