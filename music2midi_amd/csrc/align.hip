// Aligning note labels to a recording for gfx950: the integer chroma / onset features of log band energies, their 5 Hz box sums, and
// batched DTW with its backtracking.  Stands in for the feature and DTW stages of ref: data/align_audio_midi.py; the definition is
// music2midi_amd/align.py (features_host, coarse, cost_matrix, dtw_host) and every output here is EQUAL to its.  The only fp32
// arithmetic is ONE subtraction before each comparison of the features (nothing to contract; the pragma below says so anyway);
// everything else is integer arithmetic.
//
// Features: one workgroup per AF_FRAMES consecutive frames of one clip.  It stages those rows of L and the six before them in LDS,
// takes each row's maximum, marks on[t][p] for the frames and the four before them, and then one thread per (frame, class) counts.
//
// DTW: ONE WORKGROUP PER PROBLEM, no workgroup ever waits for another.  The matrix is walked in strips of DT_WS columns; thread j owns
// column c0 + j and, at step s of a strip, cell (s - j, c0 + j): an anti-diagonal per step, one __syncthreads per step.  A thread
// keeps D[i-1][j] (its own last result) and D[i-1][j-1] (the value it read from its left neighbour one step ago) in registers and
// reads D[i][j-1] from the neighbour's slot of a two-entry LDS ring.  The strip's last column goes to an LDS edge array of N int32
// (128 KiB at the size limit), which the next strip's thread 0 reads IN PLACE: row s is read at step s and overwritten at step
// s + width - 1, never before.  The cell cost is computed inside the wavefront from the thread's column vector (registers, rolled by
// the shift once per strip) and the row vector (read one step ahead), WITHOUT the definition's 64-bit division:
// isqrt(X // Y) is the largest r with r r Y <= X, found from an fp32 estimate and corrected by exact 64-bit products (DESIGN.md
// section 28).  Directions: 2 bits per cell, 16 rows of a column per dword, dword (i / 16) * M + j.  Thread 0 backtracks into a scratch
// list, the workgroup turns it round into the caller's path.
#include "common.h"

#pragma clang fp contract(off)

namespace m2m {
namespace {

constexpr int AL_BANDS = 88;
constexpr int AL_LOW = 21;
constexpr int AF_FRAMES = 32;                        // frames per workgroup
constexpr int AF_HALO = 6;                           // rows of L before the first frame: on[t-4] needs L[t-6]
constexpr int AF_ROWS = AF_FRAMES + AF_HALO;
constexpr int AF_ON = AF_FRAMES + 4;                 // rows of on[]: the frames and the four before them
constexpr int AF_THREADS = 256;
constexpr float AF_LN20 = 0x1.7f7428p+1f;            // float32(ln 20), the bits numpy's float32(np.log(20.0)) has
constexpr float AF_LN4 = 0x1.62e430p+0f;             // float32(ln 4)

constexpr int DT_WS = 512;                           // columns of a strip = threads of the workgroup
constexpr int DT_INF = 0x3FFFFFFF;                   // + 4 * 512 stays inside int32; every real D is at most 2^27
constexpr int DT_S = 256;
constexpr int DT_PAD = 4;                            // words of LDS between the ring and the edge column

__global__ __launch_bounds__(AF_THREADS) void af_features_kernel(const float* __restrict__ L, const int32_t* __restrict__ offsets,
                                                                 int64_t total_frames, uint8_t* __restrict__ chroma,
                                                                 uint8_t* __restrict__ onset) {
  __shared__ float Ls[AF_ROWS][AL_BANDS];
  __shared__ float Ms[AF_ROWS];
  __shared__ uint8_t on[AF_ON][AL_BANDS];
  const int tid = threadIdx.x;
  int64_t f0 = offsets[blockIdx.y], f1 = offsets[blockIdx.y + 1];
  f0 = f0 < 0 ? 0 : (f0 > total_frames ? total_frames : f0);
  f1 = f1 < f0 ? f0 : (f1 > total_frames ? total_frames : f1);
  const int F = (int)(f1 - f0);
  const int t0 = (int)blockIdx.x * AF_FRAMES;
  if (t0 >= F) return;                               // uniform
  const float* Lc = L + f0 * AL_BANDS;
  for (int idx = tid; idx < AF_ROWS * AL_BANDS; idx += AF_THREADS) {
    const int r = idx / AL_BANDS, p = idx - r * AL_BANDS;
    const int t = t0 - AF_HALO + r;
    Ls[r][p] = (t >= 0 && t < F) ? Lc[(int64_t)t * AL_BANDS + p] : 0.0f;
  }
  __syncthreads();
  if (tid < AF_ROWS) {
    float m = Ls[tid][0];
    for (int p = 1; p < AL_BANDS; ++p) m = fmaxf(m, Ls[tid][p]);
    Ms[tid] = m;
  }
  __syncthreads();
  for (int idx = tid; idx < AF_ON * AL_BANDS; idx += AF_THREADS) {
    const int ro = idx / AL_BANDS, p = idx - ro * AL_BANDS;
    const int r = ro + 2;                            // row of Ls; r - 2 >= 0
    const int t = t0 - 4 + ro;
    bool o = false;
    if (t >= 2 && t < F) {
      const float m = Ms[r];
      const float rise = Ls[r][p] - Ls[r - 2][p];
      const float thr = m - AF_LN20;
      o = rise >= AF_LN4 && Ls[r][p] >= thr && !(m <= -6.0f);
    }
    on[ro][p] = o ? 1 : 0;
  }
  __syncthreads();
  const float dk[4] = {0x1.d52410p-1f, 0x1.9c0420p+0f, 0x1.26bb1cp+1f, AF_LN20};       // float32(ln 2.5, ln 5, ln 10, ln 20)
  for (int idx = tid; idx < AF_FRAMES * 12; idx += AF_THREADS) {
    const int fl = idx / 12, c = idx - fl * 12;
    const int t = t0 + fl;
    if (t >= F) continue;
    const int r = fl + AF_HALO;
    const float m = Ms[r];
    const int p0 = (c + 12 - AL_LOW % 12) % 12;      // the first band of class c: (21 + p0) % 12 == c
    int q = 0;
    if (!(m <= -6.0f)) {
      float thr[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) thr[k] = m - dk[k];
      for (int p = p0; p < AL_BANDS; p += 12) {
        const float v = Ls[r][p];
#pragma unroll
        for (int k = 0; k < 4; ++k) q += v >= thr[k] ? 1 : 0;
      }
    }
    int best = 0;
#pragma unroll
    for (int tau = 0; tau < 4; ++tau) {
      const int ro = fl + 4 - tau;                   // on[] row of frame t - tau; ro - 1 >= 0
      if (t - tau < 0) continue;
      int o = 0;
      for (int p = p0; p < AL_BANDS; p += 12) o += (on[ro][p] && !on[ro - 1][p]) ? 1 : 0;
      const int v = (4 - tau) * o;
      best = v > best ? v : best;
    }
    chroma[(f0 + t) * 12 + c] = (uint8_t)q;
    onset[(f0 + t) * 12 + c] = (uint8_t)best;
  }
}

__global__ __launch_bounds__(256) void af_coarse_kernel(const uint8_t* __restrict__ chroma, const int32_t* __restrict__ frame_offsets,
                                                        const int32_t* __restrict__ coarse_offsets, int64_t total_frames,
                                                        int64_t total_coarse, int W, int D, int32_t* __restrict__ out) {
  int64_t f0 = frame_offsets[blockIdx.y], f1 = frame_offsets[blockIdx.y + 1];
  f0 = f0 < 0 ? 0 : (f0 > total_frames ? total_frames : f0);
  f1 = f1 < f0 ? f0 : (f1 > total_frames ? total_frames : f1);
  int64_t c0 = coarse_offsets[blockIdx.y], c1 = coarse_offsets[blockIdx.y + 1];
  c0 = c0 < 0 ? 0 : (c0 > total_coarse ? total_coarse : c0);
  c1 = c1 < c0 ? c0 : (c1 > total_coarse ? total_coarse : c1);
  const int F = (int)(f1 - f0);
  const int idx = (int)(blockIdx.x * 256 + threadIdx.x);
  const int j = idx / 12, c = idx - j * 12;
  if (j >= (int)(c1 - c0)) return;
  const int centre = j * D, half = W / 2;
  int sum = 0;
  for (int t = centre - half; t < centre - half + W; ++t)
    if (t >= 0 && t < F) sum += chroma[(f0 + t) * 12 + c];
  out[(c0 + j) * 12 + c] = sum;
}

// ------------------------------------------------------------------ DTW
// dwords of workspace of one problem: the direction bits, then the scratch path (n + m points of two int32), rounded up to 64 dwords
__host__ __device__ inline int64_t dt_block_dwords(int n, int m) {
  const int64_t d = (int64_t)((n + 15) / 16) * m + 2 * ((int64_t)n + m);
  return (d + 63) / 64 * 64;
}
inline int64_t dt_table_bytes(int P) { return align_up((int64_t)P * (int64_t)sizeof(m2m_align_problem), 256); }

// S - isqrt(S S dot^2 // (na nb)), S for a zero vector, without the division: the root is the largest r with r r Y <= X for
// X = (S dot)^2 <= 1.93e18, Y = na nb.  r <= S by Cauchy-Schwarz, so r r Y <= X < 2^63 for every r that is tried but r + 1 = S + 1,
// which the bound r < S keeps out.  The fp32 estimate is within 1 of the root; the loops end for any estimate.
__device__ inline int dt_cost(int dot, int na, int nb) {
  const int64_t Y = (int64_t)na * (int64_t)nb;
  if (Y == 0) return DT_S;
  const int64_t sd = (int64_t)DT_S * (int64_t)dot;
  const int64_t X = sd * sd;
  int r = (int)((float)sd / sqrtf((float)Y));
  r = r < 0 ? 0 : (r > DT_S ? DT_S : r);
  while (r < DT_S && (int64_t)(r + 1) * (r + 1) * Y <= X) ++r;
  while (r > 0 && (int64_t)r * r * Y > X) --r;
  return DT_S - r;
}

template <bool COARSE> struct DtVec;                 // 12 classes of one frame: of one feature (coarse) or of two
template <> struct DtVec<true> {
  int v[12];
  __device__ inline void load(const void* f0, const void*, int64_t frame) {
    const int4* p = reinterpret_cast<const int4*>(static_cast<const int32_t*>(f0) + frame * 12);   // 48-byte rows of a 16-byte aligned array
    const int4 a = p[0], b = p[1], c = p[2];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
  }
};
template <> struct DtVec<false> {
  uint32_t w[6];                                     // chroma bytes 0..11, onset bytes 0..11
  __device__ inline void load(const void* f0, const void* f1, int64_t frame) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(f0) + frame * 12);   // 12-byte rows, 4-byte aligned
    const uint32_t* q = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(f1) + frame * 12);
    w[0] = p[0]; w[1] = p[1]; w[2] = p[2]; w[3] = q[0]; w[4] = q[1]; w[5] = q[2];
  }
  __device__ inline int get(int feature, int c) const { return (int)((w[feature * 3 + (c >> 2)] >> (8 * (c & 3))) & 0xFFu); }
};

// The column's side of the cost: its classes rolled by the shift (class c takes the unshifted class c - shift) and its norms.
template <bool COARSE> struct DtCol {
  int v[COARSE ? 12 : 24];
  int nb[COARSE ? 1 : 2];
  __device__ inline void set(const DtVec<COARSE>& x, int shift) {
    constexpr int NF = COARSE ? 1 : 2;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      int tmp[12];
#pragma unroll
      for (int c = 0; c < 12; ++c) {
        if constexpr (COARSE) tmp[c] = x.v[c];
        else tmp[c] = x.get(f, c);
      }
      int n = 0;
#pragma unroll
      for (int c = 0; c < 12; ++c) {
        int src = c - shift;                         // shift in 0..11
        src = src < 0 ? src + 12 : src;
        int val = 0;
#pragma unroll
        for (int k = 0; k < 12; ++k) val = (k == src) ? tmp[k] : val;      // a select chain: no dynamically indexed registers
        v[f * 12 + c] = val;
        n += val * val;
      }
      nb[f] = n;
    }
  }
  __device__ inline int cost(const DtVec<COARSE>& a) const {
    constexpr int NF = COARSE ? 1 : 2;
    int total = 0;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      int dot = 0, na = 0;                           // at most 12 * 672^2 = 5 419 008
#pragma unroll
      for (int c = 0; c < 12; ++c) {
        int x;
        if constexpr (COARSE) x = a.v[c];
        else x = a.get(f, c);
        dot += x * v[f * 12 + c];
        na += x * x;
      }
      total += dt_cost(dot, na, nb[f]);
    }
    return total;
  }
};

template <bool COARSE>
__global__ __launch_bounds__(DT_WS) void dt_dtw_kernel(const m2m_align_problem* __restrict__ probs, const void* __restrict__ a0,
                                                       const void* __restrict__ a1, const void* __restrict__ b0,
                                                       const void* __restrict__ b1, uint32_t* __restrict__ blocks,
                                                       int32_t* __restrict__ total_out, int32_t* __restrict__ path_out,
                                                       int64_t path_capacity, int32_t* __restrict__ len_out) {
  extern __shared__ __align__(16) int32_t dt_lds[];
  int32_t* ring = dt_lds;                            // [2][DT_WS]
  int32_t* path_len = dt_lds + 2 * DT_WS;            // [DT_PAD], one word used.  No static LDS: the kernel opts in to all 160 KiB as dynamic
  int32_t* edge = dt_lds + 2 * DT_WS + DT_PAD;       // [N]
  const int tid = threadIdx.x;
  const int p = blockIdx.x;
  const m2m_align_problem pr = probs[p];             // uniform
  const int N = pr.n, M = pr.m;
  int64_t block0 = 0;
  for (int q = 0; q < p; ++q) block0 += dt_block_dwords(probs[q].n, probs[q].m);
  uint32_t* dirs = blocks + block0;
  int32_t* scratch = reinterpret_cast<int32_t*>(dirs + (int64_t)((N + 15) / 16) * M);     // [2][N + M]

  for (int c0 = 0; c0 < M; c0 += DT_WS) {
    const int width = M - c0 < DT_WS ? M - c0 : DT_WS;
    const bool mine = tid < width;
    const int col = c0 + tid;
    DtCol<COARSE> colv;
    {
      DtVec<COARSE> x;
      x.load(b0, b1, (int64_t)pr.b_offset + (mine ? col : c0));
      colv.set(x, pr.shift);
    }
    DtVec<COARSE> cur, next;
    cur.load(a0, a1, (int64_t)pr.a_offset);          // row 0: thread 0's first row; the others take theirs from `next`
    next = cur;
    int up = DT_INF;                                 // D[i-1][col]
    int diag = (c0 == 0 && tid == 0) ? 0 : DT_INF;   // D[i-1][col-1]: the virtual origin for cell (0, 0)
    uint32_t bits = 0;
    const int steps = N + width - 1;
    for (int s = 0; s < steps; ++s) {
      const int i = s - tid;
      const int inext = i + 1;
      if (mine && inext >= 0 && inext < N) next.load(a0, a1, (int64_t)pr.a_offset + inext);
      if (mine && i >= 0 && i < N) {
        const int left = tid == 0 ? (c0 == 0 ? DT_INF : edge[i]) : ring[((s + 1) & 1) * DT_WS + tid - 1];   // D[i][col-1]
        const int c = colv.cost(cur);
        int best = diag + 4 * c, dir = 0;
        const int cu = up + 3 * c, cl = left + 3 * c;
        if (cu < best) { best = cu; dir = 1; }
        if (cl < best) { best = cl; dir = 2; }
        ring[(s & 1) * DT_WS + tid] = best;
        if (tid == width - 1) edge[i] = best;
        bits |= (uint32_t)dir << (2 * (i & 15));
        if ((i & 15) == 15 || i == N - 1) {
          dirs[(int64_t)(i >> 4) * M + col] = bits;
          bits = 0;
        }
        if (i == N - 1 && col == M - 1) total_out[p] = best;
        up = best;
        diag = left;
      }
      cur = next;
      __syncthreads();
    }
  }
  __threadfence();
  __syncthreads();
  const int room = N + M;
  if (tid == 0) {
    int i = N - 1, j = M - 1, k = 0;
    while (k < room) {
      scratch[k] = i;
      scratch[room + k] = j;
      ++k;
      if (i == 0 && j == 0) break;
      int d = (int)((dirs[(int64_t)(i >> 4) * M + j] >> (2 * (i & 15))) & 3u);
      if (i == 0) d = 2;                             // what the recurrence gives on the border; also ends the walk whatever the bits hold
      else if (j == 0) d = 1;
      if (d == 0) { --i; --j; }
      else if (d == 1) --i;
      else --j;
    }
    *path_len = k;
    len_out[p] = k;
  }
  __threadfence();
  __syncthreads();
  const int len = *path_len;
  for (int k = tid; k < len; k += DT_WS) {
    path_out[(int64_t)pr.path_offset + k] = scratch[len - 1 - k];
    path_out[path_capacity + pr.path_offset + k] = scratch[room + len - 1 - k];
  }
}

}  // namespace
}  // namespace m2m

// ------------------------------------------------------------------ C ABI ---
using namespace m2m;

extern "C" int m2m_align_features(const float* L_dev, const int32_t* frame_offsets_dev, int n_clips, int max_frames, int64_t total_frames,
                                  uint8_t* chroma_out_dev, uint8_t* onset_out_dev, void* stream) {
  // every refusal is made on the arguments alone, before the first HIP call
  M2M_REQUIRE(n_clips >= 1 && n_clips <= M2M_ALIGN_MAX_CLIPS, "m2m_align_features: %d clips out of range (1..%d)", n_clips, M2M_ALIGN_MAX_CLIPS);
  M2M_REQUIRE(total_frames >= 1 && total_frames <= M2M_ALIGN_MAX_TOTAL_FRAMES, "m2m_align_features: %lld frames out of range (1..%d)",
              (long long)total_frames, M2M_ALIGN_MAX_TOTAL_FRAMES);
  M2M_REQUIRE(max_frames >= 1 && max_frames <= total_frames, "m2m_align_features: max_frames = %d outside 1..%lld", max_frames,
              (long long)total_frames);
  M2M_REQUIRE(L_dev && frame_offsets_dev && chroma_out_dev && onset_out_dev, "m2m_align_features: null pointer");
  M2M_REQUIRE(((uintptr_t)L_dev | (uintptr_t)frame_offsets_dev) % 4 == 0, "m2m_align_features: a pointer is not 4-byte aligned");
  const dim3 grid((unsigned)ceil_div(max_frames, AF_FRAMES), (unsigned)n_clips), block(AF_THREADS);
  hipLaunchKernelGGL(af_features_kernel, grid, block, 0, (hipStream_t)stream, L_dev, frame_offsets_dev, total_frames, chroma_out_dev,
                     onset_out_dev);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

extern "C" int m2m_align_coarse(const uint8_t* chroma_dev, const int32_t* frame_offsets_dev, const int32_t* coarse_offsets_dev, int n_clips,
                                int max_coarse, int64_t total_frames, int64_t total_coarse, int W, int D, int32_t* out_dev, void* stream) {
  M2M_REQUIRE(n_clips >= 1 && n_clips <= M2M_ALIGN_MAX_CLIPS, "m2m_align_coarse: %d clips out of range (1..%d)", n_clips, M2M_ALIGN_MAX_CLIPS);
  M2M_REQUIRE(total_frames >= 1 && total_frames <= M2M_ALIGN_MAX_TOTAL_FRAMES && total_coarse >= 1 && total_coarse <= total_frames,
              "m2m_align_coarse: %lld frames, %lld coarse frames out of range", (long long)total_frames, (long long)total_coarse);
  M2M_REQUIRE(max_coarse >= 1 && max_coarse <= total_coarse, "m2m_align_coarse: max_coarse = %d outside 1..%lld", max_coarse,
              (long long)total_coarse);
  M2M_REQUIRE(W >= 1 && W <= 255 && D >= 1 && D <= 255, "m2m_align_coarse: W = %d, D = %d out of range (1..255)", W, D);   // 255 * 32 * 12 classes stay far inside int32
  M2M_REQUIRE(chroma_dev && frame_offsets_dev && coarse_offsets_dev && out_dev, "m2m_align_coarse: null pointer");
  M2M_REQUIRE(((uintptr_t)frame_offsets_dev | (uintptr_t)coarse_offsets_dev | (uintptr_t)out_dev) % 4 == 0,
              "m2m_align_coarse: a pointer is not 4-byte aligned");
  const dim3 grid((unsigned)ceil_div(max_coarse * 12, 256), (unsigned)n_clips), block(256);
  hipLaunchKernelGGL(af_coarse_kernel, grid, block, 0, (hipStream_t)stream, chroma_dev, frame_offsets_dev, coarse_offsets_dev, total_frames,
                     total_coarse, W, D, out_dev);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

extern "C" int m2m_align_dtw_strip(void) { return DT_WS; }

extern "C" int64_t m2m_align_dtw_workspace_bytes(const int32_t* rows_host, const int32_t* cols_host, int n_problems) {
  M2M_REQUIRE(rows_host && cols_host, "m2m_align_dtw_workspace_bytes: null sizes");
  M2M_REQUIRE(n_problems >= 1 && n_problems <= M2M_ALIGN_MAX_PROBLEMS, "m2m_align_dtw_workspace_bytes: %d problems out of range (1..%d)",
              n_problems, M2M_ALIGN_MAX_PROBLEMS);
  int64_t dwords = 0;
  for (int p = 0; p < n_problems; ++p) {
    M2M_REQUIRE(rows_host[p] >= 1 && rows_host[p] <= M2M_ALIGN_MAX_FRAMES && cols_host[p] >= 1 && cols_host[p] <= M2M_ALIGN_MAX_FRAMES,
                "m2m_align_dtw_workspace_bytes: problem %d is %d x %d frames, a side is 1..%d", p, rows_host[p], cols_host[p],
                M2M_ALIGN_MAX_FRAMES);
    dwords += dt_block_dwords(rows_host[p], cols_host[p]);
  }
  return dt_table_bytes(n_problems) + 4 * dwords;
}

extern "C" int m2m_align_dtw(const void* a0_dev, const void* a1_dev, int a_frames, const void* b0_dev, const void* b1_dev, int b_frames,
                             int coarse, const m2m_align_problem* problems_host, int n_problems, void* workspace_dev,
                             int64_t workspace_bytes, int32_t* total_out_dev, int32_t* path_out_dev, int64_t path_capacity,
                             int32_t* path_len_out_dev, void* stream) {
  // every refusal is made on the arguments alone, before the first HIP call
  M2M_REQUIRE(n_problems >= 1 && n_problems <= M2M_ALIGN_MAX_PROBLEMS, "m2m_align_dtw: %d problems out of range (1..%d)", n_problems,
              M2M_ALIGN_MAX_PROBLEMS);
  M2M_REQUIRE(coarse == 0 || coarse == 1, "m2m_align_dtw: coarse = %d", coarse);
  M2M_REQUIRE(a_frames >= 1 && b_frames >= 1, "m2m_align_dtw: %d / %d frames of features", a_frames, b_frames);
  M2M_REQUIRE(problems_host && a0_dev && a1_dev && b0_dev && b1_dev && workspace_dev && total_out_dev && path_out_dev && path_len_out_dev,
              "m2m_align_dtw: null pointer");
  M2M_REQUIRE(path_capacity >= 1 && path_capacity <= 0x7FFFFFFFll, "m2m_align_dtw: path_capacity = %lld out of range (1..2^31 - 1)",
              (long long)path_capacity);
  const uintptr_t feat = (uintptr_t)a0_dev | (uintptr_t)a1_dev | (uintptr_t)b0_dev | (uintptr_t)b1_dev;
  M2M_REQUIRE(feat % (coarse ? 16 : 4) == 0, "m2m_align_dtw: a feature array is not %d-byte aligned", coarse ? 16 : 4);
  M2M_REQUIRE(((uintptr_t)workspace_dev % 256) == 0 && ((uintptr_t)total_out_dev | (uintptr_t)path_out_dev | (uintptr_t)path_len_out_dev) % 4 == 0,
              "m2m_align_dtw: the workspace is not 256-byte aligned or an output not 4-byte aligned");
  int64_t dwords = 0, next_path = 0;
  int max_n = 0;
  for (int p = 0; p < n_problems; ++p) {
    const m2m_align_problem& q = problems_host[p];
    M2M_REQUIRE(q.n >= 1 && q.n <= M2M_ALIGN_MAX_FRAMES && q.m >= 1 && q.m <= M2M_ALIGN_MAX_FRAMES,
                "m2m_align_dtw: problem %d is %d x %d frames, a side is 1..%d", p, q.n, q.m, M2M_ALIGN_MAX_FRAMES);
    M2M_REQUIRE(q.a_offset >= 0 && (int64_t)q.a_offset + q.n <= a_frames && q.b_offset >= 0 && (int64_t)q.b_offset + q.m <= b_frames,
                "m2m_align_dtw: problem %d reads frames [%d, +%d) of %d and [%d, +%d) of %d", p, q.a_offset, q.n, a_frames, q.b_offset, q.m,
                b_frames);
    M2M_REQUIRE(q.shift >= 0 && q.shift <= 11, "m2m_align_dtw: problem %d: shift = %d outside 0..11", p, q.shift);
    M2M_REQUIRE(q.path_offset >= next_path && (int64_t)q.path_offset + q.n + q.m - 1 <= path_capacity,
                "m2m_align_dtw: problem %d: its path [%d, +%d) overlaps the one before it or exceeds path_capacity = %lld", p, q.path_offset,
                q.n + q.m - 1, (long long)path_capacity);
    next_path = (int64_t)q.path_offset + q.n + q.m - 1;
    dwords += dt_block_dwords(q.n, q.m);
    max_n = q.n > max_n ? q.n : max_n;
  }
  const int64_t need = dt_table_bytes(n_problems) + 4 * dwords;
  if (workspace_bytes < need) {
    set_error("m2m_align_dtw: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
    return M2M_ERR_NOMEM;
  }
  const hipStream_t s = (hipStream_t)stream;
  M2M_CHECK_HIP(hipMemcpyAsync(workspace_dev, problems_host, (size_t)n_problems * sizeof(m2m_align_problem), hipMemcpyHostToDevice, s));
  const m2m_align_problem* table = (const m2m_align_problem*)workspace_dev;
  uint32_t* blocks = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(workspace_dev) + dt_table_bytes(n_problems));
  const size_t lds = (size_t)(2 * DT_WS + DT_PAD + max_n) * sizeof(int32_t);       // at most 4 KiB + 128 KiB
  if (coarse) {
    M2M_OPT_IN_LDS(dt_dtw_kernel<true>, 160 * 1024);
    hipLaunchKernelGGL(dt_dtw_kernel<true>, dim3((unsigned)n_problems), dim3(DT_WS), lds, s, table, a0_dev, a1_dev, b0_dev, b1_dev, blocks,
                       total_out_dev, path_out_dev, path_capacity, path_len_out_dev);
  } else {
    M2M_OPT_IN_LDS(dt_dtw_kernel<false>, 160 * 1024);
    hipLaunchKernelGGL(dt_dtw_kernel<false>, dim3((unsigned)n_problems), dim3(DT_WS), lds, s, table, a0_dev, a1_dev, b0_dev, b1_dev, blocks,
                       total_out_dev, path_out_dev, path_capacity, path_len_out_dev);
  }
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}
