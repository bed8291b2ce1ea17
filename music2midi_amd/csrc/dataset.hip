// The training dataset's crop for gfx950: B segments of B different recordings, whose sample bytes are in device memory, -> mono
// fp32 at the model's sample rate, in ONE launch.  Replaces, for the recordings the device path takes, the per-item host step of
// ref: music2midi/dataset.py:124-129 (librosa.load(offset=, duration=)); the definition is Music2MIDIDataset.crop_host
// (music2midi_amd/dataset.py).  This is ig_pcm_kernel and ig_resample_kernel<true> of ingest.hip fused: every sample repeats their
// rounded operations in their order, so a row is EQUAL to load_audio_device(path, sr, offset=, duration=) of that segment, and
// nothing in this file may be contracted into a fused multiply-add (the pragma below) or reassociated.
//
// One workgroup = one tile of DS_TILE consecutive outputs of one clip (blockIdx.y); the clip's descriptor - format, channels, ratio,
// filter - is read once and is uniform over the workgroup.  The tile's input frames, w_lo..w_hi with ingest.hip's arithmetic but
// clamped to [0, n_frames) OF THE CLIP (the recording's frames before and behind the clip do not exist for the filter), are decoded
// from the sample bytes straight into LDS as mono fp32; then each thread sums its output's taps from LDS: one fp32 accumulator, the
// taps in ascending input index, a rounded multiply then a rounded add.  up == down decodes and copies.  Outputs in [n_out, T) of a
// row are written as zero by the same launch.
// LDS: DS_WINDOW floats = 16 KiB per workgroup of 4 waves, so the 8 workgroups that fill a CU's 32 wave slots fit its 160 KiB; the
// host refuses a ratio whose tile needs more (down / up above ~14: the rates that occur need 114..1199 floats).
#include "common.h"

#pragma clang fp contract(off)

#include "ingest_pcm.h"

namespace m2m {
namespace {

constexpr int DS_THREADS = 256;
constexpr int DS_TILE = DS_THREADS;                  // outputs per workgroup, one per thread
constexpr int DS_WINDOW = M2M_DATASET_LDS_WINDOW;    // floats of LDS for a tile's input frames

template <int FORMAT>
__device__ inline void ds_stage(float* xs, const unsigned char* src, int frame_bytes, int channels, bool aligned, int count, int tid) {
  for (int i = tid; i < count; i += DS_THREADS) xs[i] = ig_frame<FORMAT>(src + (int64_t)i * frame_bytes, channels, aligned);
}

__global__ __launch_bounds__(DS_THREADS) void ds_crop_kernel(const m2m_dataset_clip* __restrict__ table, float* __restrict__ out,
                                                             int64_t row_stride, int64_t T) {
  __shared__ float xs[DS_WINDOW];
  const m2m_dataset_clip c = table[blockIdx.y];      // uniform over the workgroup
  float* row = out + (int64_t)blockIdx.y * row_stride;
  const int tid = threadIdx.x;
  const int64_t n0 = (int64_t)blockIdx.x * DS_TILE, n = n0 + tid;
  const int width = ig_width(c.format);
  const int frame_bytes = c.channels * width;
  const unsigned char* src = (const unsigned char*)c.bytes_dev;
  const bool aligned = (uintptr_t)src % (uintptr_t)width == 0;
  const int64_t n_out = c.up == c.down ? c.n_frames : (c.n_frames * c.up + c.down - 1) / c.down;
  if (n0 >= n_out) {                                 // uniform: a tile of padding
    if (n < T) row[n] = 0.0f;
    return;
  }
  // the tile's input frames.  up == down: frame n is output n.  Otherwise output n0 + i reads filter index t - m up with
  // t = (n0 + i) down + half = (q0 + r / up) up + r % up, r = p0 + i down: from the first tap the first output can have to the
  // last tap of the last output, inside [0, n_frames)
  const int64_t last = (n_out - 1 - n0 < DS_TILE - 1) ? n_out - 1 - n0 : DS_TILE - 1;
  int64_t w_lo = n0, w_hi = n0 + last, q0 = 0;
  int p0 = 0, J = 0;
  if (c.up != c.down) {
    J = 2 * c.half / c.up + 1;
    const int64_t t0 = n0 * c.down + c.half;
    q0 = t0 / c.up;
    p0 = (int)(t0 - q0 * c.up);
    const int64_t q_last = q0 + (p0 + (int)last * c.down) / c.up;
    w_lo = q0 - (J - 1) > 0 ? q0 - (J - 1) : 0;
    w_hi = q_last < c.n_frames - 1 ? q_last : c.n_frames - 1;
  }
  const int count = (int)(w_hi - w_lo + 1);          // <= DS_WINDOW: the host refused every ratio whose window is larger
  const unsigned char* first = src + w_lo * frame_bytes;
  switch (c.format) {                                // uniform
    case M2M_PCM_U8: ds_stage<M2M_PCM_U8>(xs, first, frame_bytes, c.channels, aligned, count, tid); break;
    case M2M_PCM_S16: ds_stage<M2M_PCM_S16>(xs, first, frame_bytes, c.channels, aligned, count, tid); break;
    case M2M_PCM_S24: ds_stage<M2M_PCM_S24>(xs, first, frame_bytes, c.channels, aligned, count, tid); break;
    case M2M_PCM_S32: ds_stage<M2M_PCM_S32>(xs, first, frame_bytes, c.channels, aligned, count, tid); break;
    case M2M_PCM_F32: ds_stage<M2M_PCM_F32>(xs, first, frame_bytes, c.channels, aligned, count, tid); break;
    default: ds_stage<M2M_PCM_F64>(xs, first, frame_bytes, c.channels, aligned, count, tid); break;
  }
  __syncthreads();
  if (n >= n_out) {
    if (n < T) row[n] = 0.0f;
    return;
  }
  if (c.up == c.down) {                              // decode and copy: thread i staged frame n0 + i itself
    row[n] = xs[tid];
    return;
  }
  const int r = p0 + tid * c.down;
  const int64_t q = q0 + r / c.up;
  const int p = r % c.up;
  const int taps = (2 * c.half - p) / c.up + 1;                     // filter indices p, p + up, ... <= 2 half
  const int64_t m_lo = q - (taps - 1) > 0 ? q - (taps - 1) : 0;     // m = q - j reads h[p + j up]
  const int64_t m_hi = q < c.n_frames - 1 ? q : c.n_frames - 1;
  const int n_taps = (int)(m_hi - m_lo + 1);
  const float* h = c.h_phase_dev + (int64_t)p * J + (J - 1 - (int)(q - m_lo));
  const float* x = xs + (int)(m_lo - w_lo);
  float acc = 0.0f;
  // plain operators under this file's contract(off), as in ig_resample_kernel: a rounded multiply, then a rounded add
#pragma unroll 8
  for (int i = 0; i < n_taps; ++i) {
    const float prod = x[i] * h[i];
    acc = acc + prod;
  }
  row[n] = acc;
}

inline int ds_window(int up, int down) {
  if (up == down) return 0;
  const int J = 20 * (up > down ? up : down) / up + 1;
  return (up - 1 + (DS_TILE - 1) * down) / up + J;
}

}  // namespace
}  // namespace m2m

// ------------------------------------------------------------------ C ABI ---
using namespace m2m;

extern "C" int m2m_dataset_crop_window(int up, int down) {
  if (up < 1 || up > M2M_INGEST_MAX_RATIO || down < 1 || down > M2M_INGEST_MAX_RATIO) return M2M_ERR_INVALID;
  return ds_window(up, down);
}

extern "C" int m2m_dataset_crop_f32(const m2m_dataset_clip* clips_host, int n_clips, void* table_dev, float* out_dev, int64_t row_stride,
                                    int64_t T, void* stream) {
  // every refusal is made on the arguments alone, before the first HIP call
  M2M_REQUIRE(n_clips >= 1 && n_clips <= M2M_DATASET_MAX_CLIPS, "m2m_dataset_crop_f32: %d clips out of range (1..%d)", n_clips,
              M2M_DATASET_MAX_CLIPS);
  M2M_REQUIRE(T >= 1 && T <= M2M_INGEST_MAX_OUT, "m2m_dataset_crop_f32: T = %lld out of range (1..%lld)", (long long)T,
              (long long)M2M_INGEST_MAX_OUT);
  M2M_REQUIRE(row_stride >= T, "m2m_dataset_crop_f32: row_stride %lld below T = %lld", (long long)row_stride, (long long)T);
  M2M_REQUIRE(clips_host && table_dev && out_dev, "m2m_dataset_crop_f32: null descriptors / table / output");
  M2M_REQUIRE((uintptr_t)table_dev % 8 == 0, "m2m_dataset_crop_f32: table_dev is not 8-byte aligned");
  const int64_t out_bytes = ((int64_t)(n_clips - 1) * row_stride + T) * (int64_t)sizeof(float);
  const int64_t table_bytes = (int64_t)n_clips * (int64_t)sizeof(m2m_dataset_clip);
  M2M_REQUIRE(!ig_overlap(out_dev, out_bytes, table_dev, table_bytes), "m2m_dataset_crop_f32: the output overlaps the descriptor table");
  for (int i = 0; i < n_clips; ++i) {
    const m2m_dataset_clip& c = clips_host[i];
    M2M_REQUIRE(c.n_frames >= 1 && c.n_frames <= M2M_INGEST_MAX_FRAMES, "m2m_dataset_crop_f32: clip %d: %lld frames out of range (1..%d)", i,
                (long long)c.n_frames, M2M_INGEST_MAX_FRAMES);
    M2M_REQUIRE(c.channels >= 1 && c.channels <= M2M_INGEST_MAX_CHANNELS, "m2m_dataset_crop_f32: clip %d: %d channels out of range (1..%d)", i,
                c.channels, M2M_INGEST_MAX_CHANNELS);
    const int width = ig_width(c.format);
    M2M_REQUIRE(width != 0, "m2m_dataset_crop_f32: clip %d: unknown format code %d", i, c.format);
    const int64_t src_bytes = c.n_frames * c.channels * width;
    M2M_REQUIRE(src_bytes < ((int64_t)1 << 31), "m2m_dataset_crop_f32: clip %d: %lld bytes, the limit is 2^31 - 1", i, (long long)src_bytes);
    M2M_REQUIRE(c.up >= 1 && c.up <= M2M_INGEST_MAX_RATIO && c.down >= 1 && c.down <= M2M_INGEST_MAX_RATIO,
                "m2m_dataset_crop_f32: clip %d: up / down = %d / %d out of range (1..%d)", i, c.up, c.down, M2M_INGEST_MAX_RATIO);
    M2M_REQUIRE(c.up == c.down || ig_gcd(c.up, c.down) == 1, "m2m_dataset_crop_f32: clip %d: up / down = %d / %d is not in lowest terms", i,
                c.up, c.down);
    M2M_REQUIRE(c.half == 10 * (c.up > c.down ? c.up : c.down), "m2m_dataset_crop_f32: clip %d: half = %d, the filter of %d / %d has %d", i,
                c.half, c.up, c.down, 10 * (c.up > c.down ? c.up : c.down));
    M2M_REQUIRE(c.reserved == 0, "m2m_dataset_crop_f32: clip %d: reserved = %d", i, c.reserved);
    const int64_t n_out = c.up == c.down ? c.n_frames : (c.n_frames * c.up + c.down - 1) / c.down;
    M2M_REQUIRE(n_out <= T, "m2m_dataset_crop_f32: clip %d: %lld outputs do not fit T = %lld", i, (long long)n_out, (long long)T);
    M2M_REQUIRE(ds_window(c.up, c.down) <= DS_WINDOW, "m2m_dataset_crop_f32: clip %d: a tile of %d / %d reads %d frames, the LDS window holds %d",
                i, c.up, c.down, ds_window(c.up, c.down), DS_WINDOW);
    M2M_REQUIRE(c.bytes_dev && (c.h_phase_dev || c.up == c.down), "m2m_dataset_crop_f32: clip %d: null sample bytes / filter", i);
    M2M_REQUIRE(!ig_overlap(out_dev, out_bytes, c.bytes_dev, src_bytes), "m2m_dataset_crop_f32: clip %d: the output overlaps its sample bytes", i);
    if (c.up != c.down) {
      const int64_t filter_bytes = (int64_t)c.up * (2 * c.half / c.up + 1) * (int64_t)sizeof(float);
      M2M_REQUIRE(!ig_overlap(out_dev, out_bytes, c.h_phase_dev, filter_bytes), "m2m_dataset_crop_f32: clip %d: the output overlaps its filter", i);
    }
  }
  const hipStream_t s = (hipStream_t)stream;
  M2M_CHECK_HIP(hipMemcpyAsync(table_dev, clips_host, (size_t)table_bytes, hipMemcpyHostToDevice, s));
  const dim3 grid((unsigned)((T + DS_TILE - 1) / DS_TILE), (unsigned)n_clips), block(DS_THREADS);
  hipLaunchKernelGGL(ds_crop_kernel, grid, block, 0, s, (const m2m_dataset_clip*)table_dev, out_dev, row_stride, T);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}
