// Beat tracking for gfx950: the onset envelope of log band energies, and per clip the novelty, its autocorrelation, the period, the
// penalty scale, the dynamic program and its back-tracking.  The definition is music2midi_amd/beats.py (onset_envelope_host,
// track_envelope_host) and every output here is EQUAL to its.  The only fp32 arithmetic is one subtraction, one scaling by 16 (exact)
// and one truncation per band of the envelope (nothing to contract; the pragma below says so anyway); everything else is integer
// arithmetic, and integer sums are order-free, so any reduction order equals the definition's.
//
// Envelope: one workgroup per BE_FRAMES consecutive frames of one clip.  It stages those rows of L and the one before them in LDS
// (a frame reads its predecessor across the border of its workgroup's tile), takes each row's maximum, and eight lanes per frame sum
// the clipped rises of eleven bands each.
//
// Track: ONE WORKGROUP PER CLIP, no workgroup ever waits for another, every loop is bounded by the clip's frame count.
//   novelty        one thread per frame, 25 reads of the envelope (L2); o goes to the workspace, its sum and count to LDS atomics
//   autocorrelation  tiles of BT_TILE frames of o with a 200-frame halo in LDS; thread (lag, half) owns one of the 186 lags and one
//                  half of the tile: one broadcast read, one conflict-free read and one 64-bit multiply-add per frame
//   period         86 threads score their lag, thread 0 takes the first maximum
//   dynamic program  every candidate of frame t lies at least lo = (P + 1) / 2 >= 8 frames back, so the lo frames of a block are
//                  independent: a group of 16 lanes takes one frame, lane j the candidates tau = lo + j + 16 i (at most 151, so
//                  i < 10; their penalties stay in registers), keeps its best (value, tau) in ascending tau and the group reduces
//                  with DPP moves - the larger value, on a tie the smaller tau.  ONE barrier per block.  Only C[t - hi .. t - 1] is
//                  live: a ring of 256 int64 in LDS (hi + lo <= 250, so a block never overwrites what it still reads).  back[t] is
//                  kept as the byte tau (0: no predecessor) in LDS, so the back-tracking walks LDS, not memory.
//   back-tracking  thread 0 walks a strictly decreasing index, at most F / lo + 1 steps, into an LDS list; the workgroup turns it round.
#include "common.h"

#pragma clang fp contract(off)

namespace m2m {
namespace {

constexpr int BE_BANDS = 88;
constexpr int BE_FRAMES = 32;                        // frames per workgroup
constexpr int BE_ROWS = BE_FRAMES + 1;               // and the row before them
constexpr int BE_THREADS = 256;                      // eight lanes per frame
constexpr float BE_LN20 = 0x1.7f7428p+1f;            // float32(ln 20), the bits numpy's float32(np.log(20.0)) has

constexpr int BT_THREADS = 384;                      // 6 waves: 24 groups of 16 lanes, 2 x 186 autocorrelation threads
constexpr int BT_GROUPS = BT_THREADS / 16;
constexpr int BT_LAG_TOP = 2 * M2M_BEAT_LAG_MAX;     // 200: the largest lag of the autocorrelation
constexpr int BT_NLAG = BT_LAG_TOP - M2M_BEAT_LAG_MIN + 1;       // 186
constexpr int BT_TILE = 1024;
constexpr int BT_RING = 256;                         // >= hi + lo = 200 + 50
constexpr int BT_CAND = 10;                          // candidates per lane: 16 * 10 >= 151
constexpr int BT_PEN_COLS = BT_LAG_TOP + 1;          // 201
static_assert(2 * BT_NLAG <= BT_THREADS && BT_TILE % 2 == 0, "two autocorrelation threads per lag");
static_assert(BT_RING >= 2 * M2M_BEAT_LAG_MAX + (M2M_BEAT_LAG_MAX + 1) / 2, "the ring holds a block and everything it reads");
static_assert(16 * BT_CAND >= 2 * M2M_BEAT_LAG_MAX - (M2M_BEAT_LAG_MAX + 1) / 2 + 1, "a group covers every candidate");

__global__ __launch_bounds__(BE_THREADS) void be_envelope_kernel(const float* __restrict__ L, const int32_t* __restrict__ offsets,
                                                                 int64_t total_frames, int32_t* __restrict__ env) {
  __shared__ float Ls[BE_ROWS][BE_BANDS];
  __shared__ float Ms[BE_ROWS];
  const int tid = threadIdx.x;
  int64_t f0 = offsets[blockIdx.y], f1 = offsets[blockIdx.y + 1];
  f0 = f0 < 0 ? 0 : (f0 > total_frames ? total_frames : f0);
  f1 = f1 < f0 ? f0 : (f1 > total_frames ? total_frames : f1);
  const int F = (int)(f1 - f0);
  const int t0 = (int)blockIdx.x * BE_FRAMES;
  if (t0 >= F) return;                               // uniform
  const float* Lc = L + f0 * BE_BANDS;
  for (int idx = tid; idx < BE_ROWS * BE_BANDS; idx += BE_THREADS) {
    const int r = idx / BE_BANDS, p = idx - r * BE_BANDS;
    const int t = t0 - 1 + r;
    Ls[r][p] = (t >= 0 && t < F) ? Lc[(int64_t)t * BE_BANDS + p] : 0.0f;
  }
  __syncthreads();
  if (tid >= 1 && tid < BE_ROWS) {                   // row 0 is only ever a predecessor
    float m = Ls[tid][0];
    for (int p = 1; p < BE_BANDS; ++p) m = fmaxf(m, Ls[tid][p]);
    Ms[tid] = m;
  }
  __syncthreads();
  const int fl = tid >> 3, sub = tid & 7;
  const int t = t0 + fl, r = fl + 1;
  int sum = 0;
  if (t >= 1 && t < F) {
    const float m = Ms[r];
    if (!(m <= -6.0f)) {
      const float thr = m - BE_LN20;
      for (int p = sub; p < BE_BANDS; p += 8) {
        const float v = Ls[r][p];
        const float rise = v - Ls[r - 1][p];
        const float scaled = fminf(fmaxf(rise, 0.0f) * 16.0f, 255.0f);
        sum += v >= thr ? (int)scaled : 0;
      }
    }
  }
  sum += __shfl_xor(sum, 1);                         // uniform control flow: every lane takes part
  sum += __shfl_xor(sum, 2);
  sum += __shfl_xor(sum, 4);
  if (sub == 0 && t < F) env[f0 + t] = sum;
}

// v of lane (lane ^ M) for M = 1, 2, 4, 8: the DPP moves of common.h on the bits of an int
template <int M> __device__ inline int lane_xor_i(int v) { return __builtin_bit_cast(int, lane_xor<M>(__builtin_bit_cast(float, v))); }

template <int M> __device__ inline void bt_reduce_step(int64_t& best, int& btau) {
  const int lo = lane_xor_i<M>((int)(uint32_t)(uint64_t)best);
  const int hi = lane_xor_i<M>((int)(uint32_t)((uint64_t)best >> 32));
  const int otau = lane_xor_i<M>(btau);
  const int64_t other = (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
  if (other > best || (other == best && otau < btau)) {
    best = other;
    btau = otau;
  }
}

inline int64_t bt_table_bytes(int n) { return align_up((int64_t)n * (int64_t)sizeof(m2m_beat_clip), 256); }
__host__ __device__ inline int bt_tau_bytes(int frames) { return (frames + 15) / 16 * 16; }

__global__ __launch_bounds__(BT_THREADS) void bt_track_kernel(const m2m_beat_clip* __restrict__ clips, const int32_t* __restrict__ env,
                                                              const int32_t* __restrict__ prior, const int32_t* __restrict__ penalty,
                                                              int default_period, int32_t* __restrict__ novelty, int tau_bytes,
                                                              int32_t* __restrict__ period_out, int64_t* __restrict__ score_out,
                                                              int32_t* __restrict__ beats_out, int32_t* __restrict__ n_beats_out) {
  __shared__ __align__(16) int64_t ring[BT_RING];
  __shared__ __align__(16) int64_t a_s[BT_LAG_TOP + 1];
  __shared__ __align__(16) int64_t apart[2 * BT_NLAG];
  __shared__ __align__(16) int64_t score_s[M2M_BEAT_LAG_MAX + 1];
  __shared__ __align__(16) unsigned long long sum_s;
  __shared__ int32_t tile[BT_LAG_TOP + BT_TILE];
  __shared__ int count_s, base_s, period_s, n_s;
  extern __shared__ __align__(16) unsigned char bt_dyn[];
  uint8_t* taub = bt_dyn;                            // [tau_bytes]: tau of back[t], 0 when t has no predecessor
  int32_t* list = reinterpret_cast<int32_t*>(bt_dyn + tau_bytes);   // [max_frames / 8 + 2]: the beats, last first

  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const m2m_beat_clip clip = clips[b];               // uniform
  const int F = clip.frames;
  const int32_t* e = env + clip.env_offset;

  if (tid == 0) { sum_s = 0; count_s = 0; base_s = 0; }
  for (int k = tid; k <= BT_LAG_TOP; k += BT_THREADS) a_s[k] = 0;
  __syncthreads();
  {                                                  // this clip's novelty begins after that of the clips before it
    int part = 0;
    for (int q = tid; q < b; q += BT_THREADS) part += clips[q].frames;
    if (part) atomicAdd(&base_s, part);              // all clips together hold at most 2^26 frames
  }
  __syncthreads();
  int32_t* o = novelty + base_s;

  // ---- novelty
  {
    unsigned long long part = 0;
    int cnt = 0;
    for (int t = tid; t < F; t += BT_THREADS) {
      int local = 0;
      const int k0 = t - M2M_BEAT_HALF < 0 ? 0 : t - M2M_BEAT_HALF;
      const int k1 = t + M2M_BEAT_HALF > F - 1 ? F - 1 : t + M2M_BEAT_HALF;
      for (int k = k0; k <= k1; ++k) local += e[k];  // at most 25 * 22440
      int v = (2 * M2M_BEAT_HALF + 1) * e[t] - local;
      v = v < 0 ? 0 : v;
      o[t] = v;
      part += (unsigned long long)v;
      cnt += v > 0 ? 1 : 0;
    }
    if (cnt) {
      atomicAdd(&sum_s, part);
      atomicAdd(&count_s, cnt);
    }
  }
  __threadfence_block();
  __syncthreads();                                   // o is written: the workgroup reads it from here on
  const int64_t total = (int64_t)sum_s;
  const int64_t s = total / (int64_t)(count_s > 0 ? count_s : 1);

  // ---- autocorrelation
  const int ktop = F - 1 < BT_LAG_TOP ? F - 1 : BT_LAG_TOP;
  {
    const int half = tid / BT_NLAG;                  // 0, 1; 2 for the twelve threads without a lag
    const int k = M2M_BEAT_LAG_MIN + tid - half * BT_NLAG;
    const bool mine = half < 2 && k <= ktop;
    unsigned long long acc = 0;
    if (ktop >= M2M_BEAT_LAG_MIN) {                  // uniform
      for (int t0 = 0; t0 < F; t0 += BT_TILE) {
        for (int idx = tid; idx < BT_LAG_TOP + BT_TILE; idx += BT_THREADS) {
          const int t = t0 - BT_LAG_TOP + idx;
          tile[idx] = (t >= 0 && t < F) ? o[t] : 0;
        }
        __syncthreads();
        if (mine) {
          int ta = t0 + half * (BT_TILE / 2), tb = ta + BT_TILE / 2;
          ta = ta < k ? k : ta;
          tb = tb > F ? F : tb;
          for (int t = ta; t < tb; ++t) {
            const int i = t - t0 + BT_LAG_TOP;       // i - k >= 0: k <= 200
            acc += (unsigned long long)(uint32_t)tile[i] * (unsigned long long)(uint32_t)tile[i - k];
          }
        }
        __syncthreads();
      }
    }
    if (half < 2) apart[tid] = (int64_t)acc;
  }
  __syncthreads();
  if (tid < BT_NLAG) {
    const int k = M2M_BEAT_LAG_MIN + tid;
    if (k <= ktop) a_s[k] = (apart[tid] + apart[BT_NLAG + tid]) / (int64_t)(F - k);
  }
  __syncthreads();

  // ---- period
  if (tid <= M2M_BEAT_LAG_MAX) {
    int64_t sc = 0;
    if (tid >= M2M_BEAT_LAG_MIN) sc = (a_s[tid] + a_s[2 * tid] / 2) * (int64_t)prior[tid];
    score_s[tid] = sc;
    if (score_out) score_out[(int64_t)b * (M2M_BEAT_LAG_MAX + 1) + tid] = sc;
  }
  __syncthreads();
  if (tid == 0) {
    int P = clip.period;
    if (P == 0) {
      int64_t best = 0;
      P = default_period;
      for (int l = M2M_BEAT_LAG_MIN; l <= M2M_BEAT_LAG_MAX; ++l)
        if (score_s[l] > best) { best = score_s[l]; P = l; }
    }
    P = P < M2M_BEAT_LAG_MIN ? M2M_BEAT_LAG_MIN : (P > M2M_BEAT_LAG_MAX ? M2M_BEAT_LAG_MAX : P);   // the host checked it; the ring relies on it
    period_s = P;
    period_out[b] = P;
  }
  __syncthreads();
  const int P = period_s;
  const int lo = (P + 1) / 2, hi = 2 * P;

  // ---- penalties of this lane's candidates
  const int g16 = tid & 15, group = tid >> 4;
  int64_t pen[BT_CAND];
#pragma unroll
  for (int i = 0; i < BT_CAND; ++i) {
    const int tau = lo + g16 + 16 * i;
    pen[i] = tau <= hi ? ((int64_t)penalty[P * BT_PEN_COLS + tau] * s) >> 8 : 0;
  }

  // ---- dynamic program
  for (int t = tid; t < lo && t < F; t += BT_THREADS) {
    ring[t & (BT_RING - 1)] = (int64_t)o[t];
    taub[t] = 0;
  }
  __syncthreads();
  for (int t0 = lo; t0 < F; t0 += lo) {
    for (int f = group; f < lo + group; f += BT_GROUPS) {          // f - group < lo: the same trips for every group
      const int t = t0 + f;
      const bool live = f < lo && t < F;
      const int ot = live ? o[t] : 0;
      int64_t best = INT64_MIN;
      int btau = 0x7FFFFFFF;
#pragma unroll
      for (int i = 0; i < BT_CAND; ++i) {
        const int tau = lo + g16 + 16 * i;
        if (live && tau <= hi && tau <= t) {
          const int64_t v = ring[(t - tau) & (BT_RING - 1)] - pen[i];
          if (v > best) { best = v; btau = tau; }    // ascending tau: the first of equal values stays
        }
      }
      bt_reduce_step<1>(best, btau);                 // uniform control flow: every lane takes part
      bt_reduce_step<2>(best, btau);
      bt_reduce_step<4>(best, btau);
      bt_reduce_step<8>(best, btau);
      if (live && g16 == 0) {
        ring[t & (BT_RING - 1)] = (int64_t)ot + best;
        taub[t] = (uint8_t)btau;
      }
    }
    __syncthreads();
  }

  // ---- the last beat and the chain behind it
  const int room = F / 8 + 2;
  if (tid == 0) {
    int n = 0;
    if (total > 0) {
      int t = F - P < 0 ? 0 : F - P;
      int64_t best = ring[t & (BT_RING - 1)];
      for (int u = t + 1; u < F; ++u) {
        const int64_t v = ring[u & (BT_RING - 1)];
        if (v > best) { best = v; t = u; }
      }
      while (n < room) {
        list[n++] = t;
        const int tau = taub[t];
        if (tau == 0 || tau > t) break;              // tau >= lo >= 8 otherwise: the index falls strictly
        t -= tau;
      }
    }
    n_s = n;
    n_beats_out[b] = n;
  }
  __syncthreads();
  const int n = n_s;
  for (int k = tid; k < n; k += BT_THREADS) beats_out[(int64_t)clip.beat_offset + k] = list[n - 1 - k];
}

}  // namespace
}  // namespace m2m

// ------------------------------------------------------------------ C ABI ---
using namespace m2m;

extern "C" int m2m_beat_envelope(const float* L_dev, const int32_t* frame_offsets_dev, int n_clips, int max_frames, int64_t total_frames,
                                 int32_t* env_out_dev, void* stream) {
  // every refusal is made on the arguments alone, before the first HIP call
  M2M_REQUIRE(n_clips >= 1 && n_clips <= M2M_BEAT_MAX_CLIPS, "m2m_beat_envelope: %d clips out of range (1..%d)", n_clips, M2M_BEAT_MAX_CLIPS);
  M2M_REQUIRE(total_frames >= 1 && total_frames <= M2M_BEAT_MAX_TOTAL_FRAMES, "m2m_beat_envelope: %lld frames out of range (1..%d)",
              (long long)total_frames, M2M_BEAT_MAX_TOTAL_FRAMES);
  M2M_REQUIRE(max_frames >= 1 && max_frames <= total_frames, "m2m_beat_envelope: max_frames = %d outside 1..%lld", max_frames,
              (long long)total_frames);
  M2M_REQUIRE(L_dev && frame_offsets_dev && env_out_dev, "m2m_beat_envelope: null pointer");
  M2M_REQUIRE(((uintptr_t)L_dev | (uintptr_t)frame_offsets_dev | (uintptr_t)env_out_dev) % 4 == 0,
              "m2m_beat_envelope: a pointer is not 4-byte aligned");
  const dim3 grid((unsigned)ceil_div(max_frames, BE_FRAMES), (unsigned)n_clips), block(BE_THREADS);
  hipLaunchKernelGGL(be_envelope_kernel, grid, block, 0, (hipStream_t)stream, L_dev, frame_offsets_dev, total_frames, env_out_dev);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

extern "C" int64_t m2m_beat_track_workspace_bytes(const int32_t* frames_host, int n_clips) {
  M2M_REQUIRE(frames_host, "m2m_beat_track_workspace_bytes: null sizes");
  M2M_REQUIRE(n_clips >= 1 && n_clips <= M2M_BEAT_MAX_CLIPS, "m2m_beat_track_workspace_bytes: %d clips out of range (1..%d)", n_clips,
              M2M_BEAT_MAX_CLIPS);
  int64_t frames = 0;
  for (int b = 0; b < n_clips; ++b) {
    M2M_REQUIRE(frames_host[b] >= 1 && frames_host[b] <= M2M_BEAT_MAX_FRAMES, "m2m_beat_track_workspace_bytes: clip %d has %d frames (1..%d)",
                b, frames_host[b], M2M_BEAT_MAX_FRAMES);
    frames += frames_host[b];
  }
  M2M_REQUIRE(frames <= M2M_BEAT_MAX_TOTAL_FRAMES, "m2m_beat_track_workspace_bytes: %lld frames in all, at most %d", (long long)frames,
              M2M_BEAT_MAX_TOTAL_FRAMES);
  return bt_table_bytes(n_clips) + align_up(4 * frames, 256);
}

extern "C" int m2m_beat_track(const int32_t* env_dev, int64_t env_frames, const m2m_beat_clip* clips_host, int n_clips,
                              const int32_t* prior_dev, const int32_t* penalty_dev, int default_period, void* workspace_dev,
                              int64_t workspace_bytes, int32_t* period_out_dev, int64_t* score_out_dev, int32_t* beats_out_dev,
                              int64_t beat_capacity, int32_t* n_beats_out_dev, void* stream) {
  // every refusal is made on the arguments alone, before the first HIP call
  M2M_REQUIRE(n_clips >= 1 && n_clips <= M2M_BEAT_MAX_CLIPS, "m2m_beat_track: %d clips out of range (1..%d)", n_clips, M2M_BEAT_MAX_CLIPS);
  M2M_REQUIRE(env_frames >= 1 && env_frames <= M2M_BEAT_MAX_TOTAL_FRAMES, "m2m_beat_track: %lld frames of envelope out of range (1..%d)",
              (long long)env_frames, M2M_BEAT_MAX_TOTAL_FRAMES);
  M2M_REQUIRE(default_period >= M2M_BEAT_LAG_MIN && default_period <= M2M_BEAT_LAG_MAX, "m2m_beat_track: default_period = %d outside %d..%d",
              default_period, M2M_BEAT_LAG_MIN, M2M_BEAT_LAG_MAX);
  M2M_REQUIRE(env_dev && clips_host && prior_dev && penalty_dev && workspace_dev && period_out_dev && beats_out_dev && n_beats_out_dev,
              "m2m_beat_track: null pointer");
  M2M_REQUIRE(beat_capacity >= 1 && beat_capacity <= 0x7FFFFFFFll, "m2m_beat_track: beat_capacity = %lld out of range (1..2^31 - 1)",
              (long long)beat_capacity);
  M2M_REQUIRE(((uintptr_t)env_dev | (uintptr_t)prior_dev | (uintptr_t)penalty_dev | (uintptr_t)period_out_dev | (uintptr_t)beats_out_dev |
               (uintptr_t)n_beats_out_dev) % 4 == 0 && (uintptr_t)score_out_dev % 8 == 0,
              "m2m_beat_track: a table or an output is not 4-byte (score_out_dev: 8-byte) aligned");
  M2M_REQUIRE((uintptr_t)workspace_dev % 256 == 0, "m2m_beat_track: the workspace is not 256-byte aligned");
  int64_t frames = 0, next_beat = 0;
  int max_frames = 0;
  for (int b = 0; b < n_clips; ++b) {
    const m2m_beat_clip& c = clips_host[b];
    M2M_REQUIRE(c.frames >= 1 && c.frames <= M2M_BEAT_MAX_FRAMES, "m2m_beat_track: clip %d has %d frames (1..%d)", b, c.frames,
                M2M_BEAT_MAX_FRAMES);
    M2M_REQUIRE(c.env_offset >= 0 && (int64_t)c.env_offset + c.frames <= env_frames, "m2m_beat_track: clip %d reads frames [%d, +%d) of %lld",
                b, c.env_offset, c.frames, (long long)env_frames);
    M2M_REQUIRE(c.period == 0 || (c.period >= M2M_BEAT_LAG_MIN && c.period <= M2M_BEAT_LAG_MAX),
                "m2m_beat_track: clip %d: period = %d is neither 0 nor in %d..%d", b, c.period, M2M_BEAT_LAG_MIN, M2M_BEAT_LAG_MAX);
    const int room = c.frames / 8 + 2;
    M2M_REQUIRE(c.beat_offset >= next_beat && (int64_t)c.beat_offset + room <= beat_capacity,
                "m2m_beat_track: clip %d: its beats [%d, +%d) overlap those before them or exceed beat_capacity = %lld", b, c.beat_offset, room,
                (long long)beat_capacity);
    next_beat = (int64_t)c.beat_offset + room;
    frames += c.frames;
    max_frames = c.frames > max_frames ? c.frames : max_frames;
  }
  M2M_REQUIRE(frames <= M2M_BEAT_MAX_TOTAL_FRAMES, "m2m_beat_track: %lld frames in all, at most %d", (long long)frames, M2M_BEAT_MAX_TOTAL_FRAMES);
  const int64_t need = bt_table_bytes(n_clips) + align_up(4 * frames, 256);
  if (workspace_bytes < need) {
    set_error("m2m_beat_track: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    return M2M_ERR_NOMEM;
  }
  const hipStream_t s = (hipStream_t)stream;
  M2M_CHECK_HIP(hipMemcpyAsync(workspace_dev, clips_host, (size_t)n_clips * sizeof(m2m_beat_clip), hipMemcpyHostToDevice, s));
  const m2m_beat_clip* table = (const m2m_beat_clip*)workspace_dev;
  int32_t* novelty = reinterpret_cast<int32_t*>(static_cast<unsigned char*>(workspace_dev) + bt_table_bytes(n_clips));
  const int tau_bytes = bt_tau_bytes(max_frames);
  const size_t lds = (size_t)tau_bytes + (size_t)(max_frames / 8 + 2) * sizeof(int32_t);     // at most 32 KiB + 16 KiB
  hipLaunchKernelGGL(bt_track_kernel, dim3((unsigned)n_clips), dim3(BT_THREADS), lds, s, table, env_dev, prior_dev, penalty_dev, default_period,
                     novelty, tau_bytes, period_out_dev, score_out_dev, beats_out_dev, n_beats_out_dev);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}
