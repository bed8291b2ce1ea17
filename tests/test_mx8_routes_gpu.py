"""GPU: every MXFP8 kernel route of the fp8 training step on single products (csrc/mx8.hip, mxq_weights_kernel of csrc/train_gemm.hip).

tests/test_mx8_gpu.py reaches the row quantiser and the two forward-style product kernels with the fp32-store epilogue only.  The
step runs more: the weight quantiser (both images of every projection matrix), the transposing quantiser and the split-K product
+ reduce of the fp8 weight gradient, the bf16-store / accumulate / residual-with-dropout epilogues, and the e5m2 gradient format
on the dX and dW routes.  The hooks used here (m2m_mx8_quantize_cols / _rows / _weight, m2m_mx8_step_product) call the very
functions Ops::mm / dX / dW_on call (mx8_fwd / mx8_dx / mx8_dw, w8_add_matrix), so what is pinned is the step's own code.

* Quantisers: exact.  Scale bytes equal oracle.mx8.mx_quantize's and the dequantised elements are torch.equal (the FP8 bytes
  themselves are not compared with the host's: the sign of a zero is not pinned); padding is zero with scale byte 0; no 0xFF of the
  hooks' prefill survives.  The weight quantiser's two images are also byte-equal to the row quantiser's on W and on W^T.
* Products against the fp64 product of the host-dequantised operands, each quantised along that route's own reduction dimension.
  The bars are the ones the project measured for this matrix-core accumulate (test_mx8_gpu.py: 1e-4 of a row's largest output on
  ordinary data with per-row scales; test_train_configs4_gpu.py: relative l2 3e-4); the fp32 reorder floor of a 128-chunked sum
  against fp64 is 3.5e-8, so split-K adds nothing near them.  The data of these cases is test_mx8_gpu's ordinary recipe (per-row
  magnitudes, a zero block, no planted outlier: that test gives rows dominated by an outlier 5e-3); the exact relations below
  (epilogues, repeatability) run on the wide-range recipe, outliers included.
* Integer data per route: exactly representable operands, sums below 2^24: the device result equals the exact product, through
  every k-split and on top of an integer C.
* Epilogues as exact relations to the fp32-store run of the same inputs; the dropout mask is regenerated on the host.
* Every product is issued twice and must repeat bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from music2midi_amd import native, synth
from test_mx8_cpu import wide_range

pytestmark = pytest.mark.gpu

FMTS = ["e4m3", "e5m2"]
BF16_STORE, F32_STORE, F32_ACC, RESID = 0, 1, 2, 3
FWD, DX, DW = 0, 1, 2
GOLDEN = 0x9E3779B97F4A7C15
WORST = {}                    # route -> (per-row error, relative l2): the worst over the cases run so far


def _up(n, m):
    return (n + m - 1) // m * m


# ------------------------------------------------------------------ device calls
def _quantize(which, src, R, Cc, fmt):
    """src: [R][ld] fp32 or bf16 (host) -> (bytes, scale bytes) of the transposing (`cols`) or the row quantiser, host uint8."""
    lib = native.load()
    s = src.cuda().contiguous()
    if which == "cols":
        shape, fn = (Cc, _up(R, 128)), lib.m2m_mx8_quantize_cols
    else:
        shape, fn = (R, _up(Cc, 128)), lib.m2m_mx8_quantize_rows
    q = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    sc = torch.zeros((shape[0], shape[1] // 32), dtype=torch.uint8, device="cuda")
    native.check(fn(s.data_ptr(), int(s.dtype == torch.bfloat16), R, Cc, s.shape[1], int(fmt == "e5m2"), q.data_ptr(), sc.data_ptr(),
                    native.stream_handle()), f"m2m_mx8_quantize_{which}")
    return q.cpu(), sc.cpu()


def _quantize_weight(W):
    lib = native.load()
    N, K = W.shape
    w = W.cuda().contiguous()
    q, qs = torch.zeros((N, K), dtype=torch.uint8, device="cuda"), torch.zeros((N, K // 32), dtype=torch.uint8, device="cuda")
    qt, qts = torch.zeros((K, N), dtype=torch.uint8, device="cuda"), torch.zeros((K, N // 32), dtype=torch.uint8, device="cuda")
    native.check(lib.m2m_mx8_quantize_weight(w.data_ptr(), N, K, q.data_ptr(), qs.data_ptr(), qt.data_ptr(), qts.data_ptr(), native.stream_handle()),
                 "m2m_mx8_quantize_weight")
    return q.cpu(), qs.cpu(), qt.cpu(), qts.cpu()


def _product(kind, a, b, M, N, K, fmt="e4m3", fused=1, epi=F32_STORE, c0=None, r=None, p=0.0, step_key=0, salt=0):
    """One product of the step (see include/music2midi_amd.h m2m_mx8_step_product), issued TWICE from the same inputs: the two
    results must be bit-identical.  a / b: host tensors (bf16 / fp32 for a weight, bf16 for the x of a weight gradient).
    Returns (result on the host, ksplit, kchunk)."""
    lib = native.load()
    shape = {FWD: (M, N), DX: (M, K), DW: (N, K)}[kind]
    a_d, b_d = a.cuda().contiguous(), b.cuda().contiguous()
    assert a_d.dtype == torch.bfloat16 and b_d.dtype == (torch.bfloat16 if kind == DW else torch.float32)
    r_d = None if r is None else r.cuda().contiguous()
    outs = []
    for _ in range(2):
        if epi == F32_ACC:
            c_d = c0.cuda().contiguous().clone()
        else:
            c_d = torch.full(shape, float("nan"), dtype=torch.bfloat16 if epi == BF16_STORE else torch.float32, device="cuda")
        ks, kc = C.c_int(-1), C.c_int(-1)
        native.check(lib.m2m_mx8_step_product(kind, a_d.data_ptr(), b_d.data_ptr(), M, N, K, int(fmt == "e5m2"), fused, epi, c_d.data_ptr(),
                                              None if r_d is None else r_d.data_ptr(), p, step_key, salt, C.byref(ks), C.byref(kc),
                                              native.stream_handle()), "m2m_mx8_step_product")
        outs.append(c_d.cpu())
    assert torch.equal(outs[0].view(torch.int16 if epi == BF16_STORE else torch.int32), outs[1].view(torch.int16 if epi == BF16_STORE else torch.int32)), \
        "the same product issued twice differs"
    return outs[0], ks.value, kc.value


# ------------------------------------------------------------------ data
def _ordinary(rows, cols, seed, name):
    """test_mx8_product_matches_the_ocp_restatement's activation recipe: N(0, 1) with per-row magnitudes over 2^-10 .. 2^10 and a zero
    block; bf16 (what the step feeds its products)."""
    a = torch.from_numpy(synth.normal(rows + cols + seed, name, (rows, cols), 1.0))
    a = a * torch.exp2(torch.from_numpy((synth.uniform01(1 + seed, "r" + name, rows) * 20 - 10).astype(np.float32)))[:, None]
    a[0, :32] = 0.0
    return a.bfloat16()


def _weight(N, K, seed=0):
    return torch.from_numpy(synth.normal(N + K + seed, "b", (N, K), 0.05))


def _integers(rows, cols, mul, add, mod, half):
    """test_mx8_integer_data_is_exact's operands: small integers (the callers put one 32-block of the reduction dimension on
    another power-of-two scale, as that test does)."""
    return torch.from_numpy(((np.arange(rows * cols).reshape(rows, cols) * mul + add) % mod - half).astype(np.float32))


_REF = {}


def _reference(kind, a, b, fmt, key):
    """fp64 product of the host-dequantised operands, each quantised along the route's reduction dimension (computed once per case)."""
    from oracle.mx8 import mx_quant_dequant
    if key not in _REF:
        af, bf = a.float(), b.float()
        if kind == FWD:
            qa, qb = mx_quant_dequant(af, "e4m3"), mx_quant_dequant(bf, "e4m3")                                   # Qk(x) Qk(W)^T
        elif kind == DX:
            qa, qb = mx_quant_dequant(af, fmt), mx_quant_dequant(bf.T.contiguous(), "e4m3")                      # Qn(dy) Qn(W^T)^T
        else:
            qa, qb = mx_quant_dequant(af.T.contiguous(), fmt), mx_quant_dequant(bf.T.contiguous(), "e4m3")       # Qm(dy^T) Qm(x^T)^T
        _REF[key] = qa.double() @ qb.double().T
    return _REF[key]


def _errors(route, got, want):
    g, w = got.double(), want
    row = float(((g - w).abs().amax(dim=1) / w.abs().amax(dim=1).clamp_min(1e-30)).max())
    l2 = float((g - w).norm() / (w.norm() + 1e-300))
    old = WORST.get(route, (0.0, 0.0))
    WORST[route] = (max(old[0], row), max(old[1], l2))
    return row, l2


def _check_bars(route, what, got, want):
    assert torch.isfinite(got).all()
    row, l2 = _errors(route, got, want)
    print(f"[mx8 route] {route} {what}: per-row max error {row:.2e} of the row's largest output, rel l2 {l2:.2e}; "
          f"worst {route} so far {WORST[route][0]:.2e} / {WORST[route][1]:.2e}")
    assert row <= 1e-4 and l2 <= 3e-4, (route, what, row, l2)


# ------------------------------------------------------------------ quantisers
COLS_CASES = [(1, 128, 0), (31, 128, 0), (33, 200, 0), (100, 128, 0), (261, 384, 0), (300, 128, 0), (100, 200, 64)]


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("src_bf16", [False, True])
@pytest.mark.parametrize("R,Cc,extra", COLS_CASES)
def test_mxq_cols_is_the_ocp_rule_along_the_rows_with_zero_padding(R, Cc, extra, src_bf16, fmt):
    """launch_mxq_cols, the transposing quantiser of the fp8 weight gradient: src [R][C] -> qt [C][Rp], blocks along the R rows."""
    from oracle.mx8 import mx_dequantize, mx_quantize
    a = wide_range(R, Cc)
    if src_bf16:
        a = a.bfloat16()
    src = torch.full((R, Cc + extra), 7.0e4 if not src_bf16 else 3.0e4, dtype=a.dtype)      # (what lies past column C must not be read as data)
    src[:, :Cc] = a
    qt, sc = _quantize("cols", src, R, Cc, fmt)
    Rp, nb = _up(R, 128), (R + 31) // 32
    assert qt.shape == (Cc, Rp) and sc.shape == (Cc, Rp // 32)
    assert not (qt == 0xFF).any() and not (sc == 0xFF).any(), "bytes the kernel never wrote"
    want_q, want_s = mx_quantize(a.float().T.contiguous(), fmt)
    assert torch.equal(sc[:, :nb], want_s), int((sc[:, :nb] != want_s).sum())
    assert (sc[:, nb:] == 0).all()
    got = mx_dequantize(qt, sc, fmt)
    assert torch.equal(got[:, :R], mx_dequantize(want_q, want_s, fmt)), int((got[:, :R] != mx_dequantize(want_q, want_s, fmt)).sum())
    assert (got[:, R:] == 0).all() and ((qt[:, R:] & 0x7F) == 0).all()


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("R,Cc", [(33, 128), (70, 200), (261, 1152)])
def test_mxq_rows_raw_image_is_the_ocp_rule(R, Cc, fmt):
    """The row quantiser's raw bytes (test_mx8_gpu.py sees them only through a product): the image the checks below compare with."""
    from oracle.mx8 import mx_dequantize, mx_quantize
    a = wide_range(R, Cc).bfloat16()
    q, sc = _quantize("rows", a, R, Cc, fmt)
    nb = (Cc + 31) // 32
    assert not (q == 0xFF).any() and not (sc == 0xFF).any()
    want_q, want_s = mx_quantize(a.float(), fmt)
    assert torch.equal(sc[:, :nb], want_s) and (sc[:, nb:] == 0).all()
    got = mx_dequantize(q, sc, fmt)
    assert torch.equal(got[:, :Cc], mx_dequantize(want_q, want_s, fmt)) and (got[:, Cc:] == 0).all()


@pytest.mark.parametrize("N,K", [(128, 128), (384, 256), (128, 640), (1536, 512)])
def test_mxq_weights_writes_both_images_of_a_matrix(N, K):
    """mxq_weights_kernel through the step's table builder: q / qs = Qk(W), qt / qts = Qn(W^T); also byte for byte what the row
    quantiser gives on W and on W^T (device against device)."""
    from oracle.mx8 import mx_dequantize, mx_quantize
    W = wide_range(N, K, seed=5)
    q, qs, qt, qts = _quantize_weight(W)
    for name, img, scl, src in (("rows", q, qs, W), ("transposed", qt, qts, W.T.contiguous())):
        assert not (img == 0xFF).any() and not (scl == 0xFF).any(), name
        want_q, want_s = mx_quantize(src, "e4m3")
        assert torch.equal(scl, want_s), (name, int((scl != want_s).sum()))
        assert torch.equal(mx_dequantize(img, scl), mx_dequantize(want_q, want_s)), name
        rq, rs = _quantize("rows", src, src.shape[0], src.shape[1], "e4m3")
        assert torch.equal(img, rq) and torch.equal(scl, rs), name


# ------------------------------------------------------------------ products against the fp64 restatement
FWD_CASES = [(1, 128, 128), (33, 128, 128), (70, 384, 128), (100, 512, 128), (261, 128, 1152), (1100, 256, 128), (520, 1024, 128)]
DX_CASES = [(33, 128, 128), (100, 384, 128), (261, 1536, 512)]
DW_CASES = [(1, 128, 128), (100, 128, 128), (300, 128, 128), (520, 128, 256), (1100, 1536, 512)]


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("M,N,K", FWD_CASES)
def test_forward_route(M, N, K, fused):
    """Y = Qk(x) Qk(W)^T: weights from mxq_weights_kernel's row image, x quantised in the staging (mxgemm_q_kernel) or by the row
    quantiser (mxgemm_p_kernel); N >= 512 takes the 64 x 128 tile, 72 tiles take the XCD-order remap."""
    x, W = _ordinary(M, K, 0, "x"), _weight(N, K)
    got, _, _ = _product(FWD, x, W, M, N, K, fused=fused)
    _check_bars("fwd", f"[{M}x{K}] . [{N}x{K}]^T fused={fused}", got, _reference(FWD, x, W, "e4m3", ("fwd", M, N, K)))


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M,Nw,Kw", DX_CASES)
def test_dx_route(M, Nw, Kw, fmt, fused):
    """dX = Qn(dy) Qn(W^T)^T: weights from mxq_weights_kernel's transposed image [Kw][Nw], dy in the gradient format."""
    dy, W = _ordinary(M, Nw, 1, "dy"), _weight(Nw, Kw, 1)
    got, _, _ = _product(DX, dy, W, M, Nw, Kw, fmt=fmt, fused=fused)
    _check_bars("dx", f"{fmt} [{M}x{Nw}] . [{Nw}x{Kw}] fused={fused}", got, _reference(DX, dy, W, fmt, ("dx", M, Nw, Kw, fmt)))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M,Ny,Kx", DW_CASES)
def test_dw_route(M, Ny, Kx, fmt, accumulate):
    """dW = Qm(dy^T) Qm(x^T)^T: two launches of the transposing quantiser, then the product over the M rows under the step's split-K
    policy (mxgemm_kernel + mx_splitk_reduce_kernel, or the prefetching kernel when the policy does not split)."""
    # The product's operand rows are the FEATURES here (A = dy^T [Ny][M], B = x^T [Kx][M]): "per-row scales" are per feature, and the zero
    # block lies along M.  (Magnitudes over 2^-10 .. 2^10 per M row on both operands — i.e. ALONG the reduction — put every 64-step in
    # the regime of test_mx8_gpu's planted outliers, bar 5e-3: measured 1.2e-4 on the unsplit mxgemm_p_kernel that test pins, 2.1e-4 at
    # ksplit 3, relative l2 <= 5e-5 — the matrix core's alignment of a step's products to the largest one, not the route.)
    dy, x = _ordinary(Ny, M, 2, "dy").T.contiguous(), _ordinary(Kx, M, 3, "x").T.contiguous()
    want = _reference(DW, dy, x, fmt, ("dw", M, Ny, Kx, fmt))
    c0 = None
    if accumulate:          # C0 of the products' own size; the bars are on what the route ADDED (C0 is subtracted in fp64)
        c0 = torch.from_numpy(synth.normal(M + Ny, "c0", (Ny, Kx), 1.0)) * float(want.abs().mean())
    got, ks, kc = _product(DW, dy, x, M, Ny, Kx, fmt=fmt, epi=F32_ACC if accumulate else F32_STORE, c0=c0)
    print(f"[mx8 route] dw [{M}x{Ny}]^T . [{M}x{Kx}]: ksplit {ks}, kchunk {kc} of {_up(M, 128)}")
    assert ks >= 1 and kc % 128 == 0 and (ks - 1) * kc < _up(M, 128) <= ks * kc
    if accumulate:
        # C0 + v is one fp32 rounding at the magnitude of the sum: half an ulp of max(|C0|, |C0 + v|) per element, far inside the bars
        plain, _, _ = _product(DW, dy, x, M, Ny, Kx, fmt=fmt)
        assert torch.equal(got, c0 + plain), "accumulate is not C0 + the stored product"
        got = plain
    _check_bars("dw", f"{fmt} [{M}x{Ny}]^T . [{M}x{Kx}] ksplit {ks} accumulate={accumulate}", got, want)


def test_dw_cases_reach_the_unsplit_the_even_and_the_uneven_split():
    """The policy is the step's own (mx8_dw); the cases above were chosen to reach all three forms.  Asserted on what the route
    reports, not assumed."""
    seen = {}
    for M, Ny, Kx in DW_CASES:
        z = torch.zeros((M, Ny), dtype=torch.bfloat16), torch.zeros((M, Kx), dtype=torch.bfloat16)
        got, ks, kc = _product(DW, z[0], z[1], M, Ny, Kx)
        assert (got == 0).all()
        Mp = _up(M, 128)
        form = "unsplit" if ks == 1 else ("even" if Mp % kc == 0 else "uneven")
        seen.setdefault(form, []).append((M, Ny, Kx, ks, kc))
        print(f"[mx8 route] dw policy: M={M} Ny={Ny} Kx={Kx}: ksplit {ks}, kchunk {kc} of {Mp} ({form})")
    assert set(seen) == {"unsplit", "even", "uneven"}, seen


# ------------------------------------------------------------------ integer data: exact
def _assert_quantises_exactly(t, fmt):
    from oracle.mx8 import mx_quant_dequant
    assert torch.equal(mx_quant_dequant(t, fmt), t), "test data: not exactly representable"


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("M,N,K", [(261, 128, 1152), (100, 512, 128)])
def test_forward_route_integer_data_is_exact(M, N, K, fused):
    x, W = _integers(M, K, 7, 0, 13, 6), _integers(N, K, 5, 3, 11, 5)
    x[:, 64:96] *= 1024.0                      # one k-block of every row on a different scale
    W[3] *= 0.125
    _assert_quantises_exactly(x, "e4m3"); _assert_quantises_exactly(W, "e4m3")
    want = x.double() @ W.double().T
    assert want.abs().max() < 2 ** 24
    got, _, _ = _product(FWD, x.bfloat16(), W, M, N, K, fused=fused)
    assert torch.equal(got.double(), want), float((got.double() - want).abs().max())


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M,Nw,Kw", [(261, 1536, 512), (100, 384, 128)])
def test_dx_route_integer_data_is_exact(M, Nw, Kw, fmt, fused):
    dy, W = _integers(M, Nw, 7, 0, 13, 6), _integers(Nw, Kw, 5, 3, 11, 5)
    dy[:, 64:96] *= 1024.0                     # one n-block of every row on a different scale
    W[3] *= 0.125                              # one row INSIDE an n-block of W^T: its elements sit lower in the block's range
    _assert_quantises_exactly(dy, fmt); _assert_quantises_exactly(W.T.contiguous(), "e4m3")
    want = dy.double() @ W.double()
    assert want.abs().max() < 2 ** 24
    got, _, _ = _product(DX, dy.bfloat16(), W, M, Nw, Kw, fmt=fmt, fused=fused)
    assert torch.equal(got.double(), want), float((got.double() - want).abs().max())


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("M,Ny,Kx", DW_CASES)
def test_dw_route_integer_data_is_exact_through_every_split(M, Ny, Kx, fmt, accumulate):
    dy, x = _integers(M, Ny, 7, 0, 13, 6), _integers(M, Kx, 5, 3, 11, 5)
    dy[64:96] *= 1024.0                        # one m-block of every column on a different scale (no such rows at M = 1)
    x[3 % M] *= 0.125                          # one row inside an m-block
    _assert_quantises_exactly(dy.T.contiguous(), fmt); _assert_quantises_exactly(x.T.contiguous(), "e4m3")
    assert torch.equal(dy.bfloat16().float(), dy) and torch.equal(x.bfloat16().float(), x)
    want = dy.double().T @ x.double()
    c0 = None
    if accumulate:
        c0 = torch.from_numpy(((np.arange(Ny * Kx).reshape(Ny, Kx) * 3) % 17 - 8).astype(np.float32))
        want = want + c0.double()
    assert want.abs().max() < 2 ** 24
    got, ks, kc = _product(DW, dy.bfloat16(), x.bfloat16(), M, Ny, Kx, fmt=fmt, epi=F32_ACC if accumulate else F32_STORE, c0=c0)
    assert torch.equal(got.double(), want), (ks, kc, float((got.double() - want).abs().max()))


# ------------------------------------------------------------------ epilogues: exact relations to the fp32-store run
def _ulp(t):
    t = t.abs().float()
    return (torch.nextafter(t, torch.full_like(t, float("inf"))) - t).double()


EPI_CASES = [(FWD, 261, 128, 1152, "e4m3"), (FWD, 70, 384, 128, "e4m3"), (FWD, 520, 1024, 128, "e4m3"),
             (DX, 100, 384, 128, "e4m3"), (DX, 261, 1536, 512, "e5m2")]


@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("kind,M,N,K,fmt", EPI_CASES)
def test_epilogues_are_exact_relations_to_the_fp32_store(kind, M, N, K, fmt, fused):
    """TG_STORE_T (bf16), TG_ACC_F32 and TG_RESID_F32 without and with dropout, in mxgemm_q_kernel (fused) and mxgemm_p_kernel, at both
    tile widths; wide-range data, outliers included."""
    from oracle.train import DropoutMasks
    a = wide_range(M, K if kind == FWD else N, seed=7).bfloat16()
    W = _weight(N, K, 7)
    rows, cols = (M, N) if kind == FWD else (M, K)
    run = lambda **kw: _product(kind, a, W, M, N, K, fmt=fmt, fused=fused, **kw)[0]
    v = run()
    assert torch.isfinite(v).all() and (v != 0).any()
    # bf16 store: round to nearest even of the fp32 result
    assert torch.equal(run(epi=BF16_STORE).view(torch.int16), v.bfloat16().view(torch.int16))
    # accumulate / residual: one fp32 add
    other = torch.from_numpy(synth.normal(M + N + K, "c0", (rows, cols), 1.0)) * v.abs().amax(dim=1, keepdim=True)      # of each row's own size
    assert torch.equal(run(epi=F32_ACC, c0=other), other + v)
    assert torch.equal(run(epi=RESID, r=other), other + v)
    # residual + dropout: mask regenerated on the host, element index row * ldc + col
    p, site = 0.1, 3
    dm = DropoutMasks(p, 11, 0)
    mask = dm.mask(site, rows * cols).view(rows, cols)
    got = run(epi=RESID, r=other, p=p, step_key=int(dm.step_key), salt=(site * GOLDEN) & 0xFFFFFFFFFFFFFFFF)
    kept = mask != 0
    share = float(kept.float().mean())
    assert torch.equal(got[~kept], other[~kept]), "a dropped position is not R"
    scale = torch.tensor(dm.scale, dtype=torch.float32)
    exact = other.double() + v.double() * scale.double()
    # one fp32 ulp of the quantities being added (the compiler may fuse the multiply-add: either form is within it)
    tol = torch.maximum(torch.maximum(_ulp(other), _ulp(v * scale)), _ulp(got))
    bad = ((got.double() - exact).abs() > tol) & kept
    assert not bad.any(), (int(bad.sum()), float(((got.double() - exact).abs() / tol)[kept].max()))
    unfused = int((got == other + v * scale)[kept].sum())
    print(f"[mx8 route] epilogues kind={kind} [{M},{N},{K}] fused={fused}: kept share {share:.4f}; {unfused} of {int(kept.sum())} kept elements "
          f"equal the unfused R + (v * scale)")
    if (kind, M, N, K) == (FWD, 261, 128, 1152):
        assert abs(share - 0.9) <= 0.02, share


# ------------------------------------------------------------------ bad arguments: answered on the host
def test_hooks_answer_bad_arguments_with_err_invalid():
    lib = native.load()
    st = native.stream_handle()
    buf, out = torch.zeros(128 * 128, dtype=torch.float32, device="cuda"), torch.zeros(4 * 128, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    INVALID = -1
    assert lib.m2m_mx8_quantize_cols(None, 0, 4, 128, 128, 0, p, p, st) == INVALID
    assert lib.m2m_mx8_quantize_cols(p, 0, 4, 128, 64, 0, p, p, st) == INVALID            # row stride < C
    assert lib.m2m_mx8_quantize_cols(p, 2, 4, 128, 128, 0, p, p, st) == INVALID
    assert lib.m2m_mx8_quantize_rows(p, 0, 0, 128, 128, 0, p, p, st) == INVALID
    assert lib.m2m_mx8_quantize_weight(p, 128, 96, p, p, p, p, st) == INVALID             # K not a multiple of 128
    assert lib.m2m_mx8_quantize_weight(p, 64, 128, p, p, p, p, st) == INVALID
    args = lambda **kw: [kw.get(k, d) for k, d in (("kind", 0), ("a", p), ("b", p), ("M", 4), ("N", 128), ("K", 128), ("e5m2", 0), ("fused", 1),
                                                    ("epi", 1), ("c", out.data_ptr()), ("r", None), ("p", 0.0), ("key", 0), ("salt", 0), ("ks", None), ("kc", None),
                                                    ("st", st))]
    for bad in (dict(kind=3), dict(a=None), dict(c=None), dict(M=0), dict(N=96), dict(K=200), dict(e5m2=2), dict(fused=2), dict(epi=4), dict(epi=3),
                dict(epi=1, p=0.1), dict(epi=3, r=p, p=1.0), dict(kind=2, epi=0), dict(kind=2, epi=3, r=p)):
        assert lib.m2m_mx8_step_product(*args(**bad)) == INVALID, bad
    assert b"m2m_mx8_step_product" in lib.m2m_last_error()
    assert lib.m2m_mx8_step_product(*args()) == 0
