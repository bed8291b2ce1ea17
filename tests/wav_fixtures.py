"""RIFF/WAVE files built in memory for the ingest tests: every sample format read_wav converts, with its extreme values."""
import struct

import numpy as np


def wav_bytes(tag, n_ch, rate, bits, body, before_data=b"", extensible=False):
    """A RIFF/WAVE file: `body` is the data chunk's content, `before_data` raw chunks placed between `fmt ` and `data`."""
    block = n_ch * (bits // 8)
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, n_ch, rate, rate * block, block, bits)
    if extensible:
        fmt += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + b"\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71"
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + before_data
    chunks += b"data" + struct.pack("<I", len(body)) + body + (b"\x00" if len(body) & 1 else b"")
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def sample_bodies(n_ch, n_frames, seed=0):
    """kind -> (format tag, bits, interleaved bytes, the float32 [n_frames, n_ch] array read_wav's formulas give).  The first
    values of every format are its extremes."""
    rng = np.random.default_rng(seed)
    n = n_ch * n_frames
    out = {}
    u8 = rng.integers(0, 256, n, dtype=np.uint8)
    u8[:2] = [0, 255]
    out["u8"] = (1, 8, u8.tobytes(), (u8.astype(np.float32) - np.float32(128.0)) / np.float32(128.0))
    i16 = rng.integers(-32768, 32768, n).astype("<i2")
    i16[:2] = [-32768, 32767]
    out["s16"] = (1, 16, i16.tobytes(), i16.astype(np.float32) / np.float32(32768.0))
    i24 = rng.integers(-(1 << 23), 1 << 23, n).astype(np.int32)
    i24[:2] = [-(1 << 23), (1 << 23) - 1]                                           # 0x800000, 0x7FFFFF
    b24 = (i24 & 0xFFFFFF).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3]
    out["s24"] = (1, 24, b24.tobytes(), i24.astype(np.float32) / np.float32(8388608.0))
    i32 = rng.integers(-(1 << 31), 1 << 31, n).astype("<i4")
    i32[:2] = [-(1 << 31), (1 << 31) - 1]
    out["s32"] = (1, 32, i32.tobytes(), (i32.astype(np.float64) / 2147483648.0).astype(np.float32))
    f32 = rng.uniform(-1, 1, n).astype("<f4")
    f32[:4] = [1.0, -1.0, 1e-41, -0.0]                                              # 1e-41: a denormal
    out["f32"] = (3, 32, f32.tobytes(), f32.astype(np.float32))
    f64 = rng.uniform(-1, 1, n).astype("<f8")
    f64[:4] = [1.0, -1.0, 1e-41, 1e-320]                                            # a float32 denormal, a float64 denormal
    out["f64"] = (3, 64, f64.tobytes(), f64.astype(np.float32))
    return {k: (tag, bits, body, y.reshape(-1, n_ch)) for k, (tag, bits, body, y) in out.items()}
