"""CPU: oracle/mx8.py's quantised image (mx_quantize / mx_dequantize: FP8 bytes + E8M0 bytes, what tests/test_mx8_routes_gpu.py
compares the device quantisers' raw output with) is the same rule as mx_quant_dequant, which the device products are pinned to."""
import numpy as np
import pytest
import torch

from music2midi_amd import synth


def wide_range(M, K, seed=0):
    """The data of test_mx8_fused_quantisation_equals_the_separate_quantiser: per-row magnitudes over 2^-20 .. 2^20, a zero block,
    a planted 3e4 (clamped in e4m3), bf16 subnormals and a row scaled by 1e-30 (fp32 [M, K])."""
    a = torch.from_numpy(synth.normal(3 * M + K + seed, "a", (M, K), 1.0))
    a = a * torch.exp2(torch.from_numpy((synth.uniform01(2 + seed, "ra", M) * 40 - 20).astype(np.float32)))[:, None]
    a[0, :32] = 0.0
    a[M // 2, K // 2] = 3.0e4
    a[M // 3, :8] = 1e-39
    a[M - 1] *= 1e-30
    return a


@pytest.mark.parametrize("fmt", ["e4m3", "e5m2"])
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("M,K", [(1, 128), (33, 128), (300, 384), (261, 200)])
def test_mx_quantize_then_dequantize_is_mx_quant_dequant(M, K, bf16, fmt):
    from oracle.mx8 import mx_dequantize, mx_quant_dequant, mx_quantize
    a = wide_range(M, K)
    if bf16:
        a = a.bfloat16().float()
    for x in (a, a.T.contiguous()):
        q, s = mx_quantize(x, fmt)
        assert q.dtype == torch.uint8 and s.dtype == torch.uint8
        assert q.shape == x.shape and s.shape == (x.shape[0], (x.shape[1] + 31) // 32)
        back = mx_dequantize(q, s, fmt)
        want = mx_quant_dequant(x, fmt)
        assert torch.isfinite(want).all()
        assert torch.equal(back, want), float((back - want).abs().max())
    if M >= 3:                                                                               # (one row: the subnormals sit in the zero block)
        q, s = mx_quantize(a, fmt)
        assert s[0, 0] == 0 and (mx_dequantize(q, s, fmt)[0, :32] == 0).all()                # the zero block: scale byte 0 (2^-127)


def test_mx_quantize_default_format_is_e4m3():
    from oracle.mx8 import mx_dequantize, mx_quant_dequant, mx_quantize
    x = wide_range(33, 128)
    assert torch.equal(mx_dequantize(*mx_quantize(x)), mx_quant_dequant(x))
