// Audio ingest for gfx950: the sample bytes of a WAVE file -> mono fp32 -> the model's sample rate, zero-padded to whole segments.
// Replaces, for files the device path takes, the host step of ref: music2midi/model.py:83-84 (librosa.load); the definitions are
// music2midi_amd/audio.py (read_wav, load_audio's y.mean(axis=1), resample), which stay the oracle.  The results are EQUAL to theirs,
// not close: every sample repeats the host's rounded operations in the host's order, and nothing in this file may be contracted
// into a fused multiply-add (the pragma below) or reassociated.
//
// Two launches, both on the caller's stream, nothing returns to the host:
//   pcm       one thread per frame.  The frame's samples are converted as read_wav converts them and summed in channel order in
//             fp32 from +0 (numpy's mean(axis=1) below 8 channels), then divided by the fp32 channel count.  Samples are read with
//             one load when the buffer is aligned to the sample width and byte by byte otherwise (24-bit samples always are).
//   resample  out[n] = sum_m x[m] h[n down - m up + half], one thread per output, ONE fp32 accumulator, the taps in ascending m,
//             a rounded multiply then a rounded add: the order of scipy's upfirdn, so the sums are the same floats.  The filter comes
//             phase-major: output n uses the phase p = (n down + half) mod up only, whose taps are contiguous in row p, already in
//             the order of ascending m.  A workgroup is a tile of IG_TILE consecutive outputs; the inputs it touches are staged in
//             LDS when they fit IG_WINDOW floats (every ratio with down / up below ~30), and read from global memory otherwise.
//             Outputs in [n_out, capacity) are written as zero by the same launch.
// Index arithmetic: n down and m up pass 2^31 (five minutes at 44.1 kHz), so a tile's first output is placed with 64-bit
// arithmetic once; inside the tile the offsets are below 2^31 (IG_TILE down + up <= 257 000).
#include "common.h"

#pragma clang fp contract(off)

#include "ingest_pcm.h"

namespace m2m {
namespace {

constexpr int IG_THREADS = 256;
constexpr int IG_TILE = IG_THREADS;      // outputs per workgroup of the resampler, one per thread
constexpr int IG_WINDOW = 8192;          // floats of LDS for a tile's inputs (32 KiB)

// ------------------------------------------------------------------ PCM decode + downmix (the conversions: ingest_pcm.h)
template <int FORMAT>
__global__ __launch_bounds__(IG_THREADS) void ig_pcm_kernel(const unsigned char* __restrict__ src, int64_t n_frames, int channels,
                                                            int aligned, float* __restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * IG_THREADS + threadIdx.x;
  if (f >= n_frames) return;
  constexpr int width = FORMAT == M2M_PCM_U8 ? 1 : FORMAT == M2M_PCM_S16 ? 2 : FORMAT == M2M_PCM_S24 ? 3 : FORMAT == M2M_PCM_F64 ? 8 : 4;
  out[f] = ig_frame<FORMAT>(src + f * (int64_t)(channels * width), channels, aligned != 0);
}

// ------------------------------------------------------------------ polyphase resampler
struct IgResample {
  const float* x;        // [n_in]
  const float* hp;       // [up][J]: hp[p][J - 1 - j] = h[p + j up], zero where p + j up > 2 half
  float* out;            // [capacity]
  int64_t n_in, n_out, capacity;
  int up, down, half, J;
};

template <bool STAGED>
__global__ __launch_bounds__(IG_THREADS) void ig_resample_kernel(IgResample a) {
  __shared__ float xs[STAGED ? IG_WINDOW : 1];
  const int tid = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * IG_TILE, n = n0 + tid;
  if (n0 >= a.n_out) {                     // uniform: a tile of padding
    if (n < a.capacity) a.out[n] = 0.0f;
    return;
  }
  // output n0 + i reads filter index t - m up with t = (n0 + i) down + half = (q0 + r / up) up + r % up,  r = p0 + i down
  const int64_t t0 = n0 * a.down + a.half;
  const int64_t q0 = t0 / a.up;
  const int p0 = (int)(t0 - q0 * a.up);
  int64_t w_lo = 0;
  if constexpr (STAGED) {
    // the tile's inputs: from the first tap the first output can have to the last tap of the last output, inside [0, n_in)
    const int64_t last = (a.n_out - 1 - n0 < IG_TILE - 1) ? a.n_out - 1 - n0 : IG_TILE - 1;
    const int64_t q_last = q0 + (p0 + (int)last * a.down) / a.up;
    w_lo = q0 - (a.J - 1) > 0 ? q0 - (a.J - 1) : 0;
    const int64_t w_hi = q_last < a.n_in - 1 ? q_last : a.n_in - 1;
    const int count = (int)(w_hi - w_lo + 1);                      // <= IG_WINDOW: the host chose STAGED by the same bound
    for (int i = tid; i < count; i += IG_THREADS) xs[i] = a.x[w_lo + i];
    __syncthreads();
  }
  if (n >= a.n_out) {
    if (n < a.capacity) a.out[n] = 0.0f;
    return;
  }
  const int r = p0 + tid * a.down;
  const int64_t q = q0 + r / a.up;
  const int p = r % a.up;
  const int taps = (2 * a.half - p) / a.up + 1;                     // filter indices p, p + up, ... <= 2 half
  const int64_t m_lo = q - (taps - 1) > 0 ? q - (taps - 1) : 0;     // m = q - j reads h[p + j up]
  const int64_t m_hi = q < a.n_in - 1 ? q : a.n_in - 1;
  const int count = (int)(m_hi - m_lo + 1);
  const float* h = a.hp + (int64_t)p * a.J + (a.J - 1 - (int)(q - m_lo));
  const float* x = STAGED ? xs + (int)(m_lo - w_lo) : a.x + m_lo;
  float acc = 0.0f;
  // plain operators under this file's contract(off): the __fmul_rn / __fadd_rn wrappers are inlined from a header compiled with
  // contraction allowed, and the pair comes out as one v_fmac_f32
#pragma unroll 8
  for (int i = 0; i < count; ++i) {                                 // unrolled: eight taps' loads in flight, the sum still in order
    const float prod = x[i] * h[i];
    acc = acc + prod;
  }
  a.out[n] = acc;
}

__global__ __launch_bounds__(IG_THREADS) void ig_copy_kernel(const float* __restrict__ x, int64_t n_in, int64_t capacity,
                                                             float* __restrict__ out) {
  const int64_t n = (int64_t)blockIdx.x * IG_THREADS + threadIdx.x;
  if (n < capacity) out[n] = n < n_in ? x[n] : 0.0f;
}

}  // namespace
}  // namespace m2m

// ------------------------------------------------------------------ C ABI ---
using namespace m2m;

extern "C" int64_t m2m_ingest_resampled_length(int64_t n_in, int up, int down) {
  if (n_in < 0 || n_in > M2M_INGEST_MAX_FRAMES || up < 1 || up > M2M_INGEST_MAX_RATIO || down < 1 || down > M2M_INGEST_MAX_RATIO)
    return M2M_ERR_INVALID;
  return (n_in * up + down - 1) / down;
}

extern "C" int m2m_ingest_phase_taps(int up, int down) {
  if (up < 1 || up > M2M_INGEST_MAX_RATIO || down < 1 || down > M2M_INGEST_MAX_RATIO) return M2M_ERR_INVALID;
  return 20 * (up > down ? up : down) / up + 1;
}

extern "C" int m2m_ingest_pcm(const void* bytes_dev, int64_t n_frames, int channels, int format, float* out_dev, void* stream) {
  // every refusal is made on the arguments alone, before the first HIP call
  M2M_REQUIRE(n_frames >= 1 && n_frames <= M2M_INGEST_MAX_FRAMES, "m2m_ingest_pcm: %lld frames out of range (1..%d)", (long long)n_frames,
              M2M_INGEST_MAX_FRAMES);
  M2M_REQUIRE(channels >= 1 && channels <= M2M_INGEST_MAX_CHANNELS, "m2m_ingest_pcm: %d channels out of range (1..%d)", channels,
              M2M_INGEST_MAX_CHANNELS);
  const int width = ig_width(format);
  M2M_REQUIRE(width != 0, "m2m_ingest_pcm: unknown format code %d", format);
  M2M_REQUIRE(bytes_dev && out_dev, "m2m_ingest_pcm: null input / output");
  M2M_REQUIRE(!ig_overlap(bytes_dev, n_frames * channels * width, out_dev, n_frames * (int64_t)sizeof(float)),
              "m2m_ingest_pcm: the output overlaps the input");
  const unsigned char* src = (const unsigned char*)bytes_dev;
  const int aligned = (uintptr_t)bytes_dev % (uintptr_t)width == 0 ? 1 : 0;
  const dim3 grid((unsigned)((n_frames + IG_THREADS - 1) / IG_THREADS)), block(IG_THREADS);
  const hipStream_t s = (hipStream_t)stream;
  switch (format) {
    case M2M_PCM_U8: hipLaunchKernelGGL(ig_pcm_kernel<M2M_PCM_U8>, grid, block, 0, s, src, n_frames, channels, aligned, out_dev); break;
    case M2M_PCM_S16: hipLaunchKernelGGL(ig_pcm_kernel<M2M_PCM_S16>, grid, block, 0, s, src, n_frames, channels, aligned, out_dev); break;
    case M2M_PCM_S24: hipLaunchKernelGGL(ig_pcm_kernel<M2M_PCM_S24>, grid, block, 0, s, src, n_frames, channels, aligned, out_dev); break;
    case M2M_PCM_S32: hipLaunchKernelGGL(ig_pcm_kernel<M2M_PCM_S32>, grid, block, 0, s, src, n_frames, channels, aligned, out_dev); break;
    case M2M_PCM_F32: hipLaunchKernelGGL(ig_pcm_kernel<M2M_PCM_F32>, grid, block, 0, s, src, n_frames, channels, aligned, out_dev); break;
    default: hipLaunchKernelGGL(ig_pcm_kernel<M2M_PCM_F64>, grid, block, 0, s, src, n_frames, channels, aligned, out_dev); break;
  }
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

extern "C" int m2m_ingest_resample_f32(const float* x_dev, int64_t n_in, int up, int down, const float* h_phase_dev, int half,
                                       float* out_dev, int64_t capacity, void* stream) {
  M2M_REQUIRE(n_in >= 1 && n_in <= M2M_INGEST_MAX_FRAMES, "m2m_ingest_resample_f32: %lld samples out of range (1..%d)", (long long)n_in,
              M2M_INGEST_MAX_FRAMES);
  M2M_REQUIRE(up >= 1 && up <= M2M_INGEST_MAX_RATIO && down >= 1 && down <= M2M_INGEST_MAX_RATIO,
              "m2m_ingest_resample_f32: up / down = %d / %d out of range (1..%d)", up, down, M2M_INGEST_MAX_RATIO);
  M2M_REQUIRE(up == down || ig_gcd(up, down) == 1, "m2m_ingest_resample_f32: up / down = %d / %d is not in lowest terms", up, down);
  M2M_REQUIRE(half == 10 * (up > down ? up : down), "m2m_ingest_resample_f32: half = %d, the filter of %d / %d has 10 max(up, down) = %d",
              half, up, down, 10 * (up > down ? up : down));
  const int64_t n_out = (n_in * up + down - 1) / down;
  M2M_REQUIRE(capacity >= n_out && capacity <= M2M_INGEST_MAX_OUT,
              "m2m_ingest_resample_f32: capacity %lld out of range (n_out = %lld .. %lld)", (long long)capacity, (long long)n_out,
              (long long)M2M_INGEST_MAX_OUT);
  M2M_REQUIRE(x_dev && out_dev && (h_phase_dev || up == down), "m2m_ingest_resample_f32: null input / filter / output");
  M2M_REQUIRE(!ig_overlap(x_dev, n_in * (int64_t)sizeof(float), out_dev, capacity * (int64_t)sizeof(float)),
              "m2m_ingest_resample_f32: the output overlaps the input");
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((capacity + IG_TILE - 1) / IG_TILE)), block(IG_THREADS);
  if (up == down) {
    hipLaunchKernelGGL(ig_copy_kernel, grid, block, 0, s, x_dev, n_in, capacity, out_dev);
  } else {
    IgResample a;
    a.x = x_dev; a.hp = h_phase_dev; a.out = out_dev;
    a.n_in = n_in; a.n_out = n_out; a.capacity = capacity;
    a.up = up; a.down = down; a.half = half; a.J = 2 * half / up + 1;
    // inputs a tile can touch: J taps of its first output, then (p0 + (IG_TILE - 1) down) / up further ones with p0 <= up - 1
    const int window = (up - 1 + (IG_TILE - 1) * down) / up + a.J;
    if (window <= IG_WINDOW) hipLaunchKernelGGL(ig_resample_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(ig_resample_kernel<false>, grid, block, 0, s, a);
  }
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}
