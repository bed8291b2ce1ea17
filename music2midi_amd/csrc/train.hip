// Training-step kernels: what `loss.backward()` + `Adafactor.step()` run for
// ref: music2midi/model.py:27-43 (training_step -> T5Transformer.forward with labels, ref transformer.py:28-39;
// optimizer = transformers Adafactor(warmup_init=True) + AdafactorSchedule), written for gfx950.
// (The Adafactor kernels and their launcher are in adafactor.hip; the plan they run on is built here, build_optimizer.  The strided
// and the weight-gradient GEMMs, the transposes and the per-step weight copies are in train_gemm.hip, behind the launchers of train.h.)
//
// Layout rules of the training path (train_api.hip drives these kernels):
//   * every activation is a plain row-major [rows, features] matrix — fp32 for the residual stream, its
//     gradient and the logits, storage type T (bf16, or fp32 in the parity mode) for every GEMM input;
//   * attention is done with MATERIALISED probabilities: training sequences are short (S = 190..261 encoder
//     positions, <= ~360 labels), so P [B,H,Sq,Sk] is a few MB per layer and the backward is four batched
//     GEMMs + one row kernel instead of a second flash kernel;
//   * ONE strided/batched MFMA GEMM (`bgemm_kernel`) serves every product of the forward and the backward:
//     either operand may be stored k-major ("transposed"), so dX = dY . W and dW = dY^T . X read the same
//     buffers the forward wrote — no transposed copies of weights or activations exist;
//   * every reduction has a fixed order (per-block partials + a second pass, never float atomics), so a
//     training step is bit-reproducible run to run.
#include "carver.h"
#include "mma.h"
#include "t5.h"
#include "train.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <functional>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

namespace m2m {

// ============================================================ element / row kernels ====
template <typename T>
__global__ void cvt_kernel(const float* __restrict__ src, T* __restrict__ dst, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = from_f32<T>(src[i]);
}
// four consecutive elements of the storage type <-> four floats (8- / 16-byte accesses)
template <typename T> __device__ inline void st_store4(T* p, float a, float b, float c, float d);
template <> __device__ inline void st_store4<bf16_t>(bf16_t* p, float a, float b, float c, float d) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack2_bf16(a, b), pack2_bf16(c, d));
}
template <> __device__ inline void st_store4<float>(float* p, float a, float b, float c, float d) { *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d); }
template <typename T> __device__ inline float4 st_load4(const T* p);
template <> __device__ inline float4 st_load4<bf16_t>(const bf16_t* p) {
  const uint2 v = *reinterpret_cast<const uint2*>(p);
  return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xFFFF0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xFFFF0000u));
}
template <> __device__ inline float4 st_load4<float>(const float* p) { return *reinterpret_cast<const float4*>(p); }
// dst = T(keep(i) * scale * src)  (the gradient entering a dropped branch)
template <typename T>
__global__ void cvt_drop_kernel(const float* __restrict__ src, T* __restrict__ dst, int64_t n, DropKey dk, uint32_t thresh, float scale) {
  const uint64_t key = thresh ? drop_site_key(dk) : 0ull;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = from_f32<T>(drop_keep(key, i, thresh) ? src[i] * scale : 0.f);
}
static inline int grid_1d(int64_t n, int per_block = 256) {
  int64_t g = (n + per_block - 1) / per_block;
  return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}
int launch_cvt(int precision, const float* src, void* dst, int64_t n, hipStream_t st) {
  if (precision == M2M_PREC_BF16) hipLaunchKernelGGL(cvt_kernel<bf16_t>, dim3(grid_1d(n)), dim3(256), 0, st, src, (bf16_t*)dst, n);
  else hipLaunchKernelGGL(cvt_kernel<float>, dim3(grid_1d(n)), dim3(256), 0, st, src, (float*)dst, n);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

// ---- attention probabilities: P = softmax(scores + bias) row by row (hf: modeling_t5.py:159-170: no 1/sqrt(d)) ----
// scores fp32 [BH][Sq][ldp]; bias_tab [H][tab_stride] by (key - query) + tab_center, or null; causal: keys > query masked.
// One wave per row; P is written in T with the padding columns [Sk, ldp) zeroed (they are GEMM operand columns).
// With dropout (hf: modeling_t5.py "attn_weights = dropout(attn_weights)") the kept-and-scaled copy Pd feeds the P.V product;
// P itself is what the softmax backward needs.
constexpr int SM_NR = 8;      // row elements per lane kept in registers (rows up to 512 keys)
template <typename T>
__global__ __launch_bounds__(256) void softmax_fwd_kernel(const float* __restrict__ sc, T* __restrict__ P, int rows_total, int H,
                                                          int Sq, int Sk, int ldp, const float* __restrict__ bias_tab,
                                                          int tab_stride, int tab_center, int causal, T* __restrict__ Pd,
                                                          DropKey dk, uint32_t thresh, float scale) {
  const uint64_t key = (Pd && thresh) ? drop_site_key(dk) : 0ull;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows_total) return;
  const int q = row % Sq, bh = row / Sq, hh = bh % H;
  const float* s = sc + (int64_t)row * ldp;
  T* p = P + (int64_t)row * ldp;
  const int kend = causal ? min(Sk, q + 1) : Sk;
  const float* bt = bias_tab ? bias_tab + (int64_t)hh * tab_stride + tab_center - q : nullptr;
  if (ldp <= 64 * SM_NR) {
    // rows of up to 512 keys (every shape of the model): the row lives in registers between the three passes — one read of
    // the scores and one exponential per element instead of three reads and two exponentials; same values, same summation order
    float v[SM_NR];
    float mx = -1e30f;
#pragma unroll
    for (int u = 0; u < SM_NR; ++u) {
      const int k = lane + 64 * u;
      v[u] = k < kend ? s[k] + (bt ? bt[k] : 0.f) : -1e30f;
      if (k < kend) mx = fmaxf(mx, v[u]);
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < SM_NR; ++u) {
      const int k = lane + 64 * u;
      v[u] = k < kend ? expf(v[u] - mx) : 0.f;
      if (k < kend) sum += v[u];
    }
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int u = 0; u < SM_NR; ++u) {
      const int k = lane + 64 * u;
      if (k < ldp) {
        const T pt = from_f32<T>(v[u] * inv);
        p[k] = pt;
        if (Pd) Pd[(int64_t)row * ldp + k] = drop_keep(key, (int64_t)row * ldp + k, thresh) ? from_f32<T>(to_f32(pt) * scale) : from_f32<T>(0.f);
      }
    }
    return;
  }
  float mx = -1e30f;
  for (int k = lane; k < kend; k += 64) mx = fmaxf(mx, s[k] + (bt ? bt[k] : 0.f));
  mx = wave_max(mx);
  float sum = 0.f;
  for (int k = lane; k < kend; k += 64) sum += expf(s[k] + (bt ? bt[k] : 0.f) - mx);
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  for (int k = lane; k < ldp; k += 64) {
    const float pv = k < kend ? expf(s[k] + (bt ? bt[k] : 0.f) - mx) * inv : 0.f;
    const T pt = from_f32<T>(pv);
    p[k] = pt;
    if (Pd) Pd[(int64_t)row * ldp + k] = drop_keep(key, (int64_t)row * ldp + k, thresh) ? from_f32<T>(to_f32(pt) * scale) : from_f32<T>(0.f);
  }
}
// K and V of every (clip, head) transposed for the fused products of the stripe kernels: src element (b, s, h, d) at
// src + (b*S + s)*ld + which*wstride + h*64 + d  ->  dst[which][(b*H + h)*64 + d][s], row pitch Sp (a multiple of 32), zero in [S, Sp).
template <typename T>
__global__ __launch_bounds__(256) void kv_transpose_kernel(const T* __restrict__ src, int64_t ld, int64_t wstride, T* __restrict__ dst, int S, int Sp, int H,
                                                           int64_t dst_wstride) {
  // register transposes only (tr_col): a thread takes an E x E block — E rows of s, 16 bytes of d each — and writes E rows of d,
  // 16 bytes of s each; for a fixed register the lanes of a wave cover whole 128-byte lines on both sides (the LDS form with
  // 2-byte accesses took 9.3 us per launch)
  constexpr int E = 16 / sizeof(T), DB = DK / E;              // d blocks per row: 8 (bf16) / 16 (fp32)
  const int bh = blockIdx.y, which = blockIdx.z, b = bh / H, hh = bh - b * H;
  const int blk = blockIdx.x * 256 + threadIdx.x;             // block id: d block fastest on the load side
  const int sb = blk / DB, db = blk - sb * DB;
  const int s0 = sb * E;
  if (s0 >= Sp) return;
  const T* sp = src + (int64_t)b * S * ld + which * wstride + hh * DK + db * E;
  uint4 rg[E];
#pragma unroll
  for (int k = 0; k < E; ++k) rg[k] = (s0 + k < S) ? *reinterpret_cast<const uint4*>(sp + (int64_t)(s0 + k) * ld) : make_uint4(0, 0, 0, 0);
  T* dp = dst + which * dst_wstride + ((int64_t)bh * DK + db * E) * Sp + s0;
#pragma unroll
  for (int jj = 0; jj < E; ++jj) *reinterpret_cast<uint4*>(dp + (int64_t)jj * Sp) = tr_col<T, E>(rg, jj);
}

// ---- attention stripes: scores -> probabilities (forward) and dP -> dS (backward) WITHOUT the fp32 [Sq, Sk] image ----
// Training sequences are short (S, L <= 320 here), so one wave can hold a whole stripe of 32 queries x all keys in MFMA
// accumulators: T^T = X . Y^T with the KEYS as tile rows (X = K or V, [Sk, 64]) and the QUERIES as tile columns
// (Y = Q or dO), so a lane owns ONE query (column l & 31) and its row reductions are in-lane plus one exchange with lane ^ 32
// (the orientation of the inference flash kernel).  Forward: + T5 bias (per-head row of the (key - query) table, staged in
// LDS), causal mask, softmax, P written in T (its dropped copy stays in LDS, the operand of the fused P~ . V).
// Backward: dP = V . dO^T, dS = P o (dP~ - sum P o dP~) with dP~ the dropout-masked dP.  Replaces a batched GEMM that wrote the fp32 image + a row kernel that read it back
// (35 MB each way per call at 16 clips): 15.6 + 25.7 us -> one launch (forward), 15.6 + 18 us -> one launch (backward).
#ifdef M2M_ST_STAMP      // diagnostic builds only: phase times of one workgroup of the stripe kernel (100 MHz s_memrealtime)
__device__ unsigned long long g_st_stamp[4][12];
#define ST_STAMP(i) do { if (threadIdx.x == 0 && bh == 5 && sx == 4) g_st_stamp[(BWD ? 2 : 0) + (BIAS ? 1 : 0)][i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define ST_WAITLOADS() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define ST_STAMP(i) do {} while (0)
#define ST_WAITLOADS() do {} while (0)
#endif
struct StripeArgs {
  const void *X, *Y;                 // (key, d) at X + b*sX1 + h*sX2 + key*ldx + d;  (query, d) at Y + b*sY1 + h*sY2 + q*ldy + d
  int64_t ldx, sX1, sX2, ldy, sY1, sY2;
  void* P;                           // [nB*H][Sq][ldp] T: forward out / backward in
  void* Pd;                          // backward with dropout: the dropped P again, out (the dV product's operand)
  void* dS;                          // backward out
  float* diag_part;                  // backward, self-attention with bias: [nB*H][stripes][Sk + 31] diagonal sums of dS per stripe, or null
  // the fused product with the rows this workgroup has just formed: forward O = P~ . V, backward dQ = dS . K.  Xt is the
  // second operand TRANSPOSED ([nB*H][64][xt_ld], zero beyond Sk: kv_transpose_kernel), (query, d) of the result at
  // O + b*sO1 + h*sO2 + q*ldo + d
  const void* Xt;
  int64_t xt_ld;
  void* O;
  int64_t ldo, sO1, sO2;
  const float* bias_tab;             // forward, self-attention: [H][tab_stride] by (key - query + tab_center); null: no bias
  int tab_stride, tab_center;
  int H, Sq, Sk, ldp, causal;
  DropKey dk;
  uint32_t thresh;
  float scale;
  int n_stripes, xcd_total;          // set by launch_attn_stripe: stripes per (clip, head); > 0: 1-D launch in XCD-contiguous order
};
constexpr int ST_NT = 16;            // key tiles per stripe: Sk <= 512 (the X operand of a (clip, head) is staged in LDS)
// the LDS of a workgroup at the largest stripe: the 32-row block of P / dS in fp32 (32 x 516 x 4 B) + the longest bias row + 1 KB static
static_assert((size_t)32 * (ST_NT * 32 + 4) * 4 + (2 * ST_NT * 32 + 31) * 4 + 16 + 1024 < 158 * 1024, "a stripe's rows and bias row must fit the LDS");
// softmax exponential: accurate in the fp32 (parity) mode; multiply + v_exp_f32 where the result is rounded to bf16
template <typename T> __device__ inline float m2m_exp_t(float x) {
  if constexpr (sizeof(T) == 2) return __builtin_amdgcn_exp2f(x * 1.4426950408889634f);
  else return expf(x);
}


// SLIM: the operand fragments are NOT kept across the two passes (reloaded, as the fp32 form always does): ~95 registers, FIVE
// workgroups per CU.  Chosen by the launch when the grid has more workgroups than the 1 024 that four per CU hold but not more
// than 1 280: the encoder's 9 stripes x 128 (clip, head) = 1 152 ran as a full round plus a round of 128 — twice one
// workgroup's time (stamps: 17.6 us of the launch's 38) — and now run as one.
template <typename T, bool BWD, bool DROP, bool BIAS, bool SLIM = false>
__global__ __launch_bounds__(256, SLIM ? 5 : 4) void attn_stripe_kernel(StripeArgs a) {
  // A workgroup = 32 queries of one (clip, head); its four waves split the key tiles (wave w: tiles w, w + 4, ...), so the
  // dependent chain of a wave is at most ST_NT / 4 tiles per pass and a 16-clip launch has > 1 000 workgroups.  Operand
  // fragments come straight from memory, all of a wave's loads in flight at once (bf16: kept in registers for both passes);
  // LDS holds only this head's bias row and the per-wave row statistics.  (First forms: all tiles' accumulators alive in
  // one wave — 368 registers, 37 us per launch; K / V staged in LDS for 128 queries per workgroup — 25 us.)
  extern __shared__ __align__(16) unsigned char st_smem[];
  constexpr int TPW = ST_NT / 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h2 = lane >> 5;
  // XCD-contiguous order (workgroup id % 8 picks the XCD): the stripes of one (clip, head) — which all read its K, V, K^T / V^T —
  // run side by side on one XCD instead of on all eight (PMC: 113 MB fetched per backward launch with the launch order)
  int sx = blockIdx.x, bh = blockIdx.y;
  const int n_stripes = a.n_stripes;
  if (a.xcd_total > 0) {
    const int per = (a.xcd_total + 7) >> 3, l = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (l >= a.xcd_total || (int)(blockIdx.x >> 3) >= per) return;       // padding workgroups (uniform, before any barrier)
    sx = l % n_stripes; bh = l / n_stripes;
  }
  const int b = bh / a.H, hh = bh - b * a.H;
  const int q0 = sx * 32;
  __shared__ float red_a[4][32], red_b[4][32];       // per-wave partial row statistics
  constexpr bool has_bias = !BWD && BIAS;
  float* st_bias = reinterpret_cast<float*>(st_smem);
  const int nt = (a.Sk + 31) >> 5;
  // row staging: the 32 x ldp block of P / dS this workgroup produces (or consumes) goes through LDS, so memory sees whole
  // rows in 16-byte chunks instead of 8-byte pieces of 32 different rows per store (forward 18.7 -> us, backward 25.3 -> us)
  const int LP = nt * 32 + 16 / (int)sizeof(T);                                   // row pitch, elements
  T* pl = reinterpret_cast<T*>(st_smem + (has_bias ? ((size_t)(a.tab_stride + 32) * 4 + 15) / 16 * 16 : 0));
  const int q = q0 + r, qc = min(q, a.Sq - 1);
  const T* X = reinterpret_cast<const T*>(a.X) + b * a.sX1 + hh * a.sX2;
  const T* Y = reinterpret_cast<const T*>(a.Y) + b * a.sY1 + hh * a.sY2;
  Frag<T> yf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) yf[s] = load_frag(Y + (int64_t)qc * a.ldy + 16 * s + 8 * h2);
  constexpr bool KEEP = sizeof(T) == 2 && !SLIM;     // fp32 fragments are twice the registers: reloaded per pass instead
  Frag<T> xf[KEEP ? TPW : 1][4];
  if constexpr (KEEP) {
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const T* xr = X + (int64_t)min((wave + 4 * j) * 32 + r, a.Sk - 1) * a.ldx + 8 * h2;      // clamped: keys >= Sk are masked below
#pragma unroll
      for (int s = 0; s < 4; ++s) xf[j][s] = load_frag(xr + 16 * s);
    }
  }
  ST_STAMP(0);
  ST_WAITLOADS();
  ST_STAMP(1);
  constexpr int EC = 16 / sizeof(T);
  const int cpr = a.ldp / EC;                        // 16-byte chunks per row (ldp is a multiple of 8)
  const int64_t blk = ((int64_t)bh * a.Sq + q0) * a.ldp;
  const uint64_t key = DROP ? drop_site_key(a.dk) : 0ull;
  if constexpr (BWD) {                               // P rows -> LDS (read twice below), coalesced
    const T* src = reinterpret_cast<const T*>(a.P) + blk;
    const int cpl = nt * 32 / EC;                      // the WHOLE LDS row: a causal stripe never rewrites the tiles above its diagonal,
                                                       // and the fused product reads them (uninitialised LDS x 0 is not 0)
    // all of a thread's chunks requested before the first is stored: ONE round trip instead of one per loop iteration (stamps: 4.6 us
    // of the workgroup's 17.6 with the plain loop).  32 rows x at most ST_NT * 32 elements = at most 8 (bf16) / 16 (fp32) chunks per thread.
    constexpr int PCH = ST_NT * 32 / EC * 32 / 256 / 2;       // in two batches: a single one spills next to the kept operand fragments
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (half * PCH * 256 >= 32 * cpl) break;                 // (uniform)
      uint4 pv[PCH];
#pragma unroll
      for (int u = 0; u < PCH; ++u) {
        const int c = threadIdx.x + 256 * (half * PCH + u), row = c / cpl, col = (c - row * cpl) * EC;
        pv[u] = (c < 32 * cpl && q0 + row < a.Sq && col < a.ldp) ? *reinterpret_cast<const uint4*>(src + (int64_t)row * a.ldp + col) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int u = 0; u < PCH; ++u) {
        const int c = threadIdx.x + 256 * (half * PCH + u), row = c / cpl, col = (c - row * cpl) * EC;
        if (c < 32 * cpl) *reinterpret_cast<uint4*>(pl + row * LP + col) = pv[u];
      }
    }
    __syncthreads();
    if constexpr (DROP) {
      // The dropped probabilities again (the dV product's operand; a scratch buffer in the forward pass) — what drop_copy_kernel
      // produced in a launch of its own, 18 launches / 0.28 ms of a step: masked straight from the staged P rows into memory, chunk by
      // chunk, before the passes overwrite them.  No second row block, so the five-per-CU variant stays available with dropout on.
      // (a.Pd is set exactly when DROP, so the test below never decides; it stays because without it this compiler allots the bf16
      //  instantiations more registers: 20 -> 44 bytes of scratch at four workgroups per CU, 71 -> 73 VGPRs in the SLIM form)
      if (a.Pd) {
        T* dst2 = reinterpret_cast<T*>(a.Pd) + blk;
        for (int c = threadIdx.x; c < 32 * cpr; c += 256) {
          const int row = c / cpr, col = (c - row * cpr) * EC;
          if (q0 + row >= a.Sq) continue;
          const int64_t at = ((int64_t)bh * a.Sq + q0 + row) * a.ldp + col;
#pragma unroll
          for (int g4 = 0; g4 < EC / 4; ++g4) {
            const float4 v = st_load4<T>(pl + row * LP + col + 4 * g4);
            const uint32_t kb = drop_keep4(key, at + 4 * g4, a.thresh);
            st_store4<T>(dst2 + (int64_t)row * a.ldp + col + 4 * g4, (kb & 1u) ? v.x * a.scale : 0.f, (kb & 2u) ? v.y * a.scale : 0.f,
                         (kb & 4u) ? v.z * a.scale : 0.f, (kb & 8u) ? v.w * a.scale : 0.f);
          }
        }
      }
    }
  }
  if (has_bias) {
    for (int i = threadIdx.x; i < a.tab_stride + 32; i += 256) st_bias[i] = i < a.tab_stride ? a.bias_tab[(int64_t)hh * a.tab_stride + i] : 0.f;
    __syncthreads();
  }
  ST_STAMP(2);
  // element i of a tile: key 32 kt + (i & 3) + 8 (i >> 2) + 4 h2, query q (this lane's column); the tile product is
  // RECOMPUTED in the second pass (4 MFMAs) instead of being kept
  auto tile = [&](int j) {
    f32x16 acc = zero_acc();
    if constexpr (KEEP) {
#pragma unroll
      for (int s = 0; s < 4; ++s) mma16(acc, xf[j][s], yf[s]);
    } else {
      const T* xr = X + (int64_t)min((wave + 4 * j) * 32 + r, a.Sk - 1) * a.ldx + 8 * h2;
#pragma unroll
      for (int s = 0; s < 4; ++s) mma16(acc, load_frag(xr + 16 * s), yf[s]);
    }
    return acc;
  };
  // fused product rows . Xt^T (see StripeArgs): waves 0 and 1 take the two 32-wide halves of d, 8 k-steps' fragments in flight at a time
  auto rows_times_xt = [&](const T* rows) {
    if (wave >= 2) return;
    const T* xt = reinterpret_cast<const T*>(a.Xt) + ((int64_t)bh * DK + wave * 32 + r) * a.xt_ld + 8 * h2;
    f32x16 acc = zero_acc();
    const int nks = nt * 2;                           // k-steps of 16 keys
    for (int k8 = 0; k8 < nks; k8 += 8) {
      Frag<T> bf[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) bf[u] = load_frag(xt + 16 * min(k8 + u, nks - 1));
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k8 + u < nks) mma16(acc, load_frag(rows + r * LP + 16 * (k8 + u) + 8 * h2), bf[u]);
    }
    T* o = reinterpret_cast<T*>(a.O) + b * a.sO1 + hh * a.sO2 + wave * 32 + r;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int qq = q0 + acc_row(i, lane);
      if (qq < a.Sq) o[(int64_t)qq * a.ldo] = from_f32<T>(acc[i]);
    }
  };
  const int kend = BWD ? a.Sk : (a.causal ? min(a.Sk, q + 1) : a.Sk);
  const int64_t prow = ((int64_t)bh * a.Sq + qc) * a.ldp;
  if constexpr (!BWD) {
    const float* bt = st_bias + a.tab_center - qc;
    // pass 1: running (max, sum) of this lane's half of the keys
    float m = -1e30f, l = 0.f;
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const int kt = wave + 4 * j;
      if (kt >= nt) break;                             // wave-uniform
      if (a.causal && kt * 32 > q0 + 31) break;        // causal: this and every later tile of the wave lie above the stripe's diagonal
      f32x16 acc = tile(j);
      float tm = -1e30f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int k = kt * 32 + (i & 3) + 8 * (i >> 2) + 4 * h2;
        float v = acc[i];
        if (has_bias) v += bt[k];                      // the LDS row is padded by 32 entries: no clamp
        v = k < kend ? v : -1e30f;
        acc[i] = v;
        tm = fmaxf(tm, v);
      }
      const float mn = fmaxf(m, tm);
      float ts = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) ts += m2m_exp_t<T>(acc[i] - mn);      // masked entries are -1e30: exp gives exactly 0, no branch
      l = l * m2m_exp_t<T>(m - mn) + ts;
      m = mn;
    }
    {
      const float mo = lane_xor<32>(m), lo = lane_xor<32>(l);
      const float mt = fmaxf(m, mo);
      l = l * m2m_exp_t<T>(m - mt) + lo * m2m_exp_t<T>(mo - mt);
      m = mt;
    }
    ST_STAMP(3);
    if (h2 == 0) { red_a[wave][r] = m; red_b[wave][r] = l; }
    __syncthreads();
    ST_STAMP(4);
    {                                                // the four waves' (max, sum) of this query, fixed order
      const float m0 = red_a[0][r], m1 = red_a[1][r], m2 = red_a[2][r], m3 = red_a[3][r];
      m = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
      l = red_b[0][r] * m2m_exp_t<T>(m0 - m) + red_b[1][r] * m2m_exp_t<T>(m1 - m) + red_b[2][r] * m2m_exp_t<T>(m2 - m) + red_b[3][r] * m2m_exp_t<T>(m3 - m);
    }
    const float inv = 1.0f / l;
    // pass 2: probabilities
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const int kt = wave + 4 * j;
      if (kt >= nt) break;                             // wave-uniform
      if (a.causal && kt * 32 > q0 + 31) {             // fully masked tile: zeros, no product, no exponentials
#pragma unroll
        for (int g = 0; g < 4; ++g) st_store4<T>(pl + r * LP + kt * 32 + 8 * g + 4 * h2, 0.f, 0.f, 0.f, 0.f);
        continue;
      }
      const f32x16 acc = tile(j);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = kt * 32 + 8 * g + 4 * h2;
        float pv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = k0 + e;
          float v = acc[4 * g + e];
          if (has_bias) v += bt[k];
          v = k < kend ? v : -1e30f;
          pv[e] = to_f32(from_f32<T>(m2m_exp_t<T>(v - m) * inv));
        }
        st_store4<T>(pl + r * LP + k0, pv[0], pv[1], pv[2], pv[3]);          // keys >= kend are zeros
      }
    }
    ST_STAMP(5);
    __syncthreads();
    ST_STAMP(6);
    {
      T* dst = reinterpret_cast<T*>(a.P) + blk;
      for (int c = threadIdx.x; c < 32 * cpr; c += 256) {
        const int row = c / cpr, col = (c - row * cpr) * EC;
        if (q0 + row < a.Sq) *reinterpret_cast<uint4*>(dst + (int64_t)row * a.ldp + col) = *reinterpret_cast<const uint4*>(pl + row * LP + col);
      }
    }
    if constexpr (DROP) {
      // The dropped probabilities are only the operand of the fused product (the backward pass re-forms them): no second row block —
      // half the LDS, four (or five) workgroups per CU instead of three — the rows are masked IN PLACE once they have been copied out,
      // every lane rewriting the elements it wrote
      __syncthreads();
#pragma unroll
      for (int j = 0; j < TPW; ++j) {
        const int kt = wave + 4 * j;
        if (kt >= nt) break;                             // wave-uniform
        if (a.causal && kt * 32 > q0 + 31) continue;     // zeros stay zeros
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int k0 = kt * 32 + 8 * g + 4 * h2;
          const float4 pv = st_load4<T>(pl + r * LP + k0);
          const float pe[4] = {pv.x, pv.y, pv.z, pv.w};
          const uint32_t kb4 = drop_keep4(key, prow + k0, a.thresh);
          float dv[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) dv[e] = ((kb4 >> e) & 1u) ? pe[e] * a.scale : 0.f;
          st_store4<T>(pl + r * LP + k0, dv[0], dv[1], dv[2], dv[3]);
        }
      }
      __syncthreads();
    }
    ST_STAMP(7);
    rows_times_xt(pl);                               // O = P~ . V
    ST_STAMP(9);
  } else {
    T* prd = pl + r * LP;                            // this lane's query row of P, in LDS
    // dP arrives for the DROPPED probabilities: through the mask first.  The keep bits of a lane's 16 elements per tile are hashed
    // ONCE (pass 1) and kept as a bit mask for pass 2 and for the dropped copy (three hashes per element before: 22 -> 36 us per launch)
    uint32_t kbits[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) kbits[j] = 0u;
    auto masked = [&](float dp, int k, bool keep) {
      if constexpr (DROP) dp = keep ? dp * a.scale : 0.f;
      return k < a.Sk ? dp : 0.f;
    };
    // pass 1: t = sum_k P dP~
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const int kt = wave + 4 * j;
      if (kt >= nt) break;                             // wave-uniform
      if (a.causal && kt * 32 > q0 + 31) break;        // causal: P is zero there
      const f32x16 acc = tile(j);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = kt * 32 + 8 * g + 4 * h2;
        const float4 pv = st_load4<T>(prd + k0);
        const float pe[4] = {pv.x, pv.y, pv.z, pv.w};
        uint32_t kb = 0xFu;
        if constexpr (DROP) { kb = drop_keep4(key, prow + k0, a.thresh); kbits[j] |= kb << (4 * g); }
#pragma unroll
        for (int e = 0; e < 4; ++e) t += (k0 + e < a.Sk ? pe[e] : 0.f) * masked(acc[4 * g + e], k0 + e, (kb >> e) & 1u);
      }
    }
    t += lane_xor<32>(t);
    ST_STAMP(3);
    if (h2 == 0) red_a[wave][r] = t;
    __syncthreads();
    ST_STAMP(4);
    t = (red_a[0][r] + red_a[1][r]) + (red_a[2][r] + red_a[3][r]);
    // pass 2: dS = P (dP~ - t)
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
      const int kt = wave + 4 * j;
      if (kt >= nt) break;                             // wave-uniform
      if (a.causal && kt * 32 > q0 + 31) {             // dS = P (...) = 0: the staged P rows already hold zeros there
        continue;
      }
      const f32x16 acc = tile(j);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int k0 = kt * 32 + 8 * g + 4 * h2;
        const float4 pv = st_load4<T>(prd + k0);
        const float pe[4] = {pv.x, pv.y, pv.z, pv.w};
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (k0 + e < a.Sk) ? pe[e] * (masked(acc[4 * g + e], k0 + e, (kbits[j] >> (4 * g + e)) & 1u) - t) : 0.f;
        st_store4<T>(prd + k0, o[0], o[1], o[2], o[3]);                        // in place: the same lane read these four
      }
    }
    ST_STAMP(5);
    __syncthreads();
    ST_STAMP(6);
    {
      T* dst = reinterpret_cast<T*>(a.dS) + blk;
      for (int c = threadIdx.x; c < 32 * cpr; c += 256) {
        const int row = c / cpr, col = (c - row * cpr) * EC;
        if (q0 + row < a.Sq) *reinterpret_cast<uint4*>(dst + (int64_t)row * a.ldp + col) = *reinterpret_cast<const uint4*>(pl + row * LP + col);
      }
    }
    // relative-position-bias gradient, stage 1 (replaces bias_diag_kernel's pass over dS in memory): the sums of this stripe's
    // dS along the diagonals key - row = i - 31, i in [0, Sk + 31), rows in fixed order; bias_bucket2_kernel adds the stripes
    ST_STAMP(7);
    if (a.diag_part) {
      const int dl = a.Sk + 31, rows = min(32, a.Sq - q0);
      float* out = a.diag_part + ((int64_t)bh * n_stripes + sx) * dl;
      for (int i = threadIdx.x; i < dl; i += 256) {
        float acc = 0.f;
        for (int r8 = 0; r8 < 32; r8 += 8) {          // eight LDS reads in flight, added in row order (the sum is what the plain loop gave)
          float v[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int rr = r8 + u, k = i - 31 + rr;
            v[u] = (rr < rows && k >= 0 && k < a.Sk) ? to_f32(pl[rr * LP + k]) : 0.f;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) acc += v[u];
        }
        out[i] = acc;
      }
    }
    ST_STAMP(8);
    rows_times_xt(pl);                               // dQ = dS . K
    ST_STAMP(9);
  }
}

template <typename T>
static int launch_attn_stripe(bool bwd, const StripeArgs& a_in, int nB, hipStream_t st, const TrainSwitches& sw) {
  StripeArgs a = a_in;
  dim3 grid((unsigned)ceil_div(a.Sq, 32), (unsigned)(nB * a.H));
  a.n_stripes = (int)grid.x;
  if (sw.xcd_order && grid.x * grid.y >= 64) {
    a.xcd_total = (int)(grid.x * grid.y);
    grid = dim3((unsigned)(8 * ceil_div(a.xcd_total, 8)));
  }
  const bool drop = a.thresh != 0, bias = !bwd && a.bias_tab != nullptr;
  const size_t bias_bytes = bias ? ((size_t)(a.tab_stride + 32) * 4 + 15) / 16 * 16 : 0;
  const size_t row_bytes = (size_t)32 * (ceil_div(a.Sk, 32) * 32 + 16 / sizeof(T)) * sizeof(T);
  const size_t smem = bias_bytes + row_bytes;
  // five workgroups per CU when that turns two rounds into one (and their LDS fits): see SLIM above
  const int64_t n_wgs = (int64_t)a.n_stripes * nB * a.H;
  const bool slim = sw.st_slim && sizeof(T) == 2 && n_wgs > 4 * 256 && n_wgs <= 5 * 256 && 5 * (smem + 1024) <= 160 * 1024;
#define M2M_ST_LAUNCH(B_, D_, I_)                                                                              \
  do {                                                                                                         \
    if (slim) {                                                                                                \
      if constexpr (sizeof(T) == 2) {                                                                          \
        M2M_OPT_IN_LDS((attn_stripe_kernel<T, B_, D_, I_, true>), 158 * 1024);                                    \
        hipLaunchKernelGGL((attn_stripe_kernel<T, B_, D_, I_, true>), grid, dim3(256), smem, st, a);           \
      }                                                                                                        \
    } else {                                                                                                   \
      M2M_OPT_IN_LDS((attn_stripe_kernel<T, B_, D_, I_>), 158 * 1024);      /* + 1 KB of static LDS */            \
      hipLaunchKernelGGL((attn_stripe_kernel<T, B_, D_, I_>), grid, dim3(256), smem, st, a);                   \
    }                                                                                                          \
  } while (0)
  if (bwd) {
    if (drop) M2M_ST_LAUNCH(true, true, false); else M2M_ST_LAUNCH(true, false, false);
  } else if (bias) {
    if (drop) M2M_ST_LAUNCH(false, true, true); else M2M_ST_LAUNCH(false, false, true);
  } else {
    if (drop) M2M_ST_LAUNCH(false, true, false); else M2M_ST_LAUNCH(false, false, false);
  }
#undef M2M_ST_LAUNCH
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

// Pd = dropout(P) again (backward: the dV product needs it, it was a scratch buffer in the forward)
template <typename T>
__global__ void drop_copy_kernel(const T* __restrict__ P, T* __restrict__ Pd, int64_t n, DropKey dk, uint32_t thresh, float scale) {
  const uint64_t key = thresh ? drop_site_key(dk) : 0ull;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) Pd[i] = drop_keep(key, i, thresh) ? from_f32<T>(to_f32(P[i]) * scale) : from_f32<T>(0.f);
}

// dS = P o (dP - rowsum(P o dP))   (softmax backward; P in T as the forward stored it, dP fp32), dS in T, padding zeroed
template <typename T>
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const T* __restrict__ P, const float* __restrict__ dP, T* __restrict__ dS,
                                                          int rows_total, int Sk, int ldp, DropKey dk, uint32_t thresh, float scale) {
  const uint64_t key = thresh ? drop_site_key(dk) : 0ull;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows_total) return;
  const T* p = P + (int64_t)row * ldp;
  const float* dp = dP + (int64_t)row * ldp;
  T* ds = dS + (int64_t)row * ldp;
  // dP arrives for the DROPPED probabilities: through the mask first (thresh == 0: identity)
  auto dpe = [&](int k) { return thresh ? (drop_keep(key, (int64_t)row * ldp + k, thresh) ? dp[k] * scale : 0.f) : dp[k]; };
  if (ldp <= 64 * SM_NR) {                 // P and dP of the row stay in registers between the two passes
    float pv[SM_NR], dv[SM_NR];
    float t = 0.f;
#pragma unroll
    for (int u = 0; u < SM_NR; ++u) {
      const int k = lane + 64 * u;
      pv[u] = k < Sk ? to_f32(p[k]) : 0.f;
      dv[u] = k < Sk ? dpe(k) : 0.f;
      if (k < Sk) t += pv[u] * dv[u];
    }
    t = wave_sum(t);
#pragma unroll
    for (int u = 0; u < SM_NR; ++u) {
      const int k = lane + 64 * u;
      if (k < ldp) ds[k] = from_f32<T>(k < Sk ? pv[u] * (dv[u] - t) : 0.f);
    }
    return;
  }
  float t = 0.f;
  for (int k = lane; k < Sk; k += 64) t += to_f32(p[k]) * dpe(k);
  t = wave_sum(t);
  for (int k = lane; k < ldp; k += 64) ds[k] = from_f32<T>(k < Sk ? to_f32(p[k]) * (dpe(k) - t) : 0.f);
}


// relative-position-bias gradient.  Stage 1: one block per (clip, head): part[b][h][rel] = sum over the diagonal
// key - query = rel - (Sq-1) of dS[b,h,q,k]; consecutive threads take consecutive diagonals, so every pass over q reads
// consecutive addresses.  Stage 2 sums the clips and the diagonals of each bucket.  Fixed order throughout.
template <typename T>
__global__ __launch_bounds__(256) void bias_diag_kernel(const T* __restrict__ dS, float* __restrict__ part, int H, int Sq, int Sk, int ldp) {
  // block = (clip-head, 64 consecutive diagonals); thread = (quarter of the queries, diagonal): consecutive threads read
  // consecutive addresses; the four partial sums of a diagonal are added in a fixed order through LDS
  __shared__ float sred[4][64];
  const int nrel = Sq + Sk - 1;
  const int bh = blockIdx.x, rl = threadIdx.x & 63, qg = threadIdx.x >> 6;
  const int rel = blockIdx.y * 64 + rl;
  const T* base = dS + (int64_t)bh * Sq * ldp;
  float acc = 0.f;
  if (rel < nrel) {
    const int off = rel - (Sq - 1);                              // key - query
    const int q_lo = max(0, -off), q_hi = min(Sq, Sk - off);     // q with 0 <= q + off < Sk
    const int per = (Sq + 3) / 4;
    const int a0 = max(q_lo, qg * per), a1 = min(q_hi, (qg + 1) * per);
    for (int q = a0; q < a1; ++q) acc += to_f32(base[(int64_t)q * ldp + q + off]);
  }
  sred[qg][rl] = acc;
  __syncthreads();
  if (qg == 0 && rel < nrel) part[(int64_t)bh * nrel + rel] = (sred[0][rl] + sred[1][rl]) + (sred[2][rl] + sred[3][rl]);
}
// stage 2: one block per (bucket, head): dtable[bucket][h] (+)= sum over clips b and the rels of that bucket of part[b][h][rel]
__global__ __launch_bounds__(256) void bias_bucket_kernel(const float* __restrict__ part, const int* __restrict__ bucket_of_rel,
                                                          float* __restrict__ dtable, int B, int H, int nrel, int accumulate) {
  __shared__ float sred[256];
  const int bk = blockIdx.x / H, hh = blockIdx.x - bk * H;
  float acc = 0.f;
  for (int rel = threadIdx.x; rel < nrel; rel += 256)
    if (bucket_of_rel[rel] == bk)
      for (int b = 0; b < B; ++b) acc += part[((int64_t)b * H + hh) * nrel + rel];
  sred[threadIdx.x] = acc;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) { if (threadIdx.x < st) sred[threadIdx.x] += sred[threadIdx.x + st]; __syncthreads(); }
  if (threadIdx.x == 0) dtable[blockIdx.x] = accumulate ? dtable[blockIdx.x] + sred[0] : sred[0];
}

// stage 1b for the per-stripe diagonal sums of attn_stripe_kernel: part2 [B*H][stripes][Sk + 31] -> tmp [H][nrel], summed over
// clips and stripes in a fixed order; the diagonal with global index rel (= key - query + Sq - 1) is entry
// rel + 31 + 32 s - (Sq - 1) of stripe s.  Block = (head, 64 consecutive rels) x 16 clip groups; bias_bucket_kernel (B = 1) follows.
__global__ __launch_bounds__(1024) void bias_stripes_sum_kernel(const float* __restrict__ part2_all, float* __restrict__ tmp_all, int B, int H, int stripes,
                                                                int Sq, int Sk, int64_t layer_stride) {
  const float* part2 = part2_all + (int64_t)blockIdx.z * layer_stride;        // blockIdx.z: layer (grouped mode: all layers of a stack in one launch)
  float* tmp = tmp_all + (int64_t)blockIdx.z * H * (Sq + Sk - 1);
  __shared__ float sred[16][64];
  const int nrel = Sq + Sk - 1, dl = Sk + 31;
  const int hh = blockIdx.x, rl = threadIdx.x & 63, bg = threadIdx.x >> 6;     // sixteen clip groups: at 16 clips one clip x all stripes per thread,
  const int rel = blockIdx.y * 64 + rl;                                        // loads unconditional (clamped) so that they are all in flight at once
  float acc = 0.f;
  if (rel < nrel) {
    const int per = (B + 15) / 16;
    for (int b = bg * per; b < min(B, (bg + 1) * per); ++b) {
      const float* pb = part2 + ((int64_t)b * H + hh) * stripes * dl;
#pragma unroll 3
      for (int sidx = 0; sidx < stripes; ++sidx) {
        const int loc = rel + 31 + 32 * sidx - (Sq - 1);
        const float v = pb[(int64_t)sidx * dl + min(max(loc, 0), dl - 1)];
        acc += (loc >= 0 && loc < dl) ? v : 0.f;
      }
    }
  }
  sred[bg][rl] = acc;
  __syncthreads();
  if (bg == 0 && rel < nrel) {
    float sum = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) sum += sred[g][rl];
    tmp[(int64_t)hh * nrel + rel] = sum;
  }
}

// ---- gated GELU (hf: modeling_t5.py T5DenseGatedActDense: gelu_new(wi_0 x) * (wi_1 x)); ab = [a | b], [M, 2*dff] ----
// four consecutive columns per thread (8- / 16-byte accesses; the first form moved 2-byte elements: 11.4 / 16.5 us per launch)
template <typename T>
__global__ void gated_fwd_kernel(const T* __restrict__ ab, T* __restrict__ mid, int64_t M, int dff, DropKey dk, uint32_t thresh, float scale) {
  const uint64_t key = thresh ? drop_site_key(dk) : 0ull;
  int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int q = dff >> 2;
  const int64_t n4 = M * q, stride = (int64_t)gridDim.x * blockDim.x;
  for (; i4 < n4; i4 += stride) {
    const int64_t row = i4 / q;
    const int c = (int)(i4 - row * q) * 4;
    const float4 a = st_load4<T>(ab + row * 2 * dff + c), b = st_load4<T>(ab + row * 2 * dff + dff + c);
    float v[4] = {gelu_new_t<T>(a.x) * b.x, gelu_new_t<T>(a.y) * b.y, gelu_new_t<T>(a.z) * b.z, gelu_new_t<T>(a.w) * b.w};      // (as the fused epilogue)
    if (thresh) {                                                       // hf: T5DenseGatedActDense dropout before wo
      const uint32_t kb = drop_keep4(key, row * dff + c, thresh);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = ((kb >> e) & 1u) ? v[e] * scale : 0.f;
    }
    st_store4<T>(mid + row * dff + c, v[0], v[1], v[2], v[3]);
  }
}
template <typename T>
__global__ void gated_bwd_kernel(const T* __restrict__ ab, const T* __restrict__ dmid, T* __restrict__ dab, int64_t M, int dff, DropKey dk,
                                 uint32_t thresh, float scale) {
  const uint64_t key = thresh ? drop_site_key(dk) : 0ull;
  int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int q = dff >> 2;
  const int64_t n4 = M * q, stride = (int64_t)gridDim.x * blockDim.x;
  for (; i4 < n4; i4 += stride) {
    const int64_t row = i4 / q;
    const int c = (int)(i4 - row * q) * 4;
    const float4 a4 = st_load4<T>(ab + row * 2 * dff + c), b4 = st_load4<T>(ab + row * 2 * dff + dff + c), d4 = st_load4<T>(dmid + row * dff + c);
    const float a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
    float dm[4] = {d4.x, d4.y, d4.z, d4.w}, da[4], db[4];
    const uint32_t kb = thresh ? drop_keep4(key, row * dff + c, thresh) : 0xFu;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (thresh) dm[e] = ((kb >> e) & 1u) ? dm[e] * scale : 0.f;
      float g, dg;
      gelu_new_both_t<T>(a[e], &g, &dg);                    // (as the fused epilogue: bit-identical either way)
      da[e] = dm[e] * b[e] * dg;
      db[e] = dm[e] * g;
    }
    st_store4<T>(dab + row * 2 * dff + c, da[0], da[1], da[2], da[3]);
    st_store4<T>(dab + row * 2 * dff + dff + c, db[0], db[1], db[2], db[3]);
  }
}

// ---- RMSNorm backward (forward: y = w * x * r, r = rsqrt(mean(x^2) + eps), hf: modeling_t5.py:59-72) ----
// dx_out[row] = dx_res[row] (gradient arriving over the residual connection, may be null)
//             + r * (w o dy) - x * r^3 * mean(w o dy o x);   dw partial per block (fixed order), reduced by colsum_kernel.
constexpr int RN_BLOCKS = 512;      // (256 until round 3: four rows per wave at 16 clips, one memory round trip each — two now, both in flight from the start)
// out_t (optional): the gradient again in the GEMM-input type, through the dropout mask of the branch that consumes it next
// (what cvt_kernel / cvt_drop_kernel would produce in a launch of its own)
template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                          const float* __restrict__ dy, const float* __restrict__ dx_res,
                                                          float* __restrict__ dx_out, float* __restrict__ dw_part, int M, int d, float eps,
                                                          T* __restrict__ out_t, DropKey dk, uint32_t thresh, float scale,
                                                          DropKey dk_in, uint32_t thresh_in) {
  // thresh_in != 0: dy arrives through the dropout that follows THIS norm in the forward pass (the final norm of a stack): masked
  // as it is loaded — a drop_inplace launch over the whole buffer before
  const uint64_t key = (out_t && thresh) ? drop_site_key(dk) : 0ull;
  const uint64_t key_in = thresh_in ? drop_site_key(dk_in) : 0ull;
  extern __shared__ float red[];          // [4][d]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float dwacc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) dwacc[j] = 0.f;
  // d <= 512: a lane's (at most two) 4-column pieces of x, dy and the weight stay in registers between the statistics
  // and the output pass (the first form read them twice, two dependent round trips per row)
  float4 gv[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) gv[j] = (lane * 4 + 256 * j < d) ? *reinterpret_cast<const float4*>(w + lane * 4 + 256 * j) : make_float4(0, 0, 0, 0);
  // A wave walks its rows (4 at M = 4 176) with the NEXT row's loads in flight while it reduces the current one: the first form
  // paid a dependent load -> reduce -> store chain per row (10 us per launch, 32 launches per step).
  const int stride = gridDim.x * 4;
  float4 xv[2], dv[2], rv[2], xn[2], dn[2], rn[2];
  const float* const res_src = dx_res ? dx_res : x;     // (never predicated: clamped addresses, unconditional loads, then a select)
  auto load_row = [&](int row, float4 (&xa)[2], float4 (&da)[2], float4 (&ra)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = lane * 4 + 256 * j;
      const bool in = col < d && row < M;
      const int64_t at = (int64_t)min(row, M - 1) * d + min(col, d - 4);
      const float4 a = *reinterpret_cast<const float4*>(x + at), b = *reinterpret_cast<const float4*>(dy + at),
                   c4 = *reinterpret_cast<const float4*>(res_src + at);
      const float4 z = make_float4(0, 0, 0, 0);
      xa[j] = in ? a : z;
      float4 bm = b;
      if (thresh_in) {
        const uint32_t kb = drop_keep4(key_in, at, thresh_in);
        bm = make_float4((kb & 1u) ? b.x * scale : 0.f, (kb & 2u) ? b.y * scale : 0.f, (kb & 4u) ? b.z * scale : 0.f, (kb & 8u) ? b.w * scale : 0.f);
      }
      da[j] = in ? bm : z;
      ra[j] = (in && dx_res) ? c4 : z;
    }
  };
  int row = blockIdx.x * 4 + wave;
  if (row < M) load_row(row, xv, dv, rv);
  for (; row < M; row += stride) {
    load_row(row + stride, xn, dn, rn);                 // (past the end: no loads, zeros)
    float ss = 0.f, c = 0.f;
#pragma unroll
    for (int j = 0; j < 2; ++j) {       // same association as the two-pass form: per piece, then pieces in order
      ss += xv[j].x * xv[j].x + xv[j].y * xv[j].y + xv[j].z * xv[j].z + xv[j].w * xv[j].w;
      c += gv[j].x * dv[j].x * xv[j].x + gv[j].y * dv[j].y * xv[j].y + gv[j].z * dv[j].z * xv[j].z + gv[j].w * dv[j].w * xv[j].w;
    }
    ss = wave_sum(ss);
    c = wave_sum(c);
    const float r = rsqrtf(ss / (float)d + eps);
    const float k2 = r * r * r * c / (float)d;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = lane * 4 + 256 * j;
      if (col < d) {
        float4 o = make_float4(r * gv[j].x * dv[j].x - xv[j].x * k2, r * gv[j].y * dv[j].y - xv[j].y * k2, r * gv[j].z * dv[j].z - xv[j].z * k2,
                               r * gv[j].w * dv[j].w - xv[j].w * k2);
        if (dx_res) { o.x += rv[j].x; o.y += rv[j].y; o.z += rv[j].z; o.w += rv[j].w; }
        *reinterpret_cast<float4*>(dx_out + (int64_t)row * d + col) = o;
        if (out_t) {
          const int64_t at = (int64_t)row * d + col;
          float v[4] = {o.x, o.y, o.z, o.w};
          if (thresh) {
            const uint32_t kb = drop_keep4(key, at, thresh);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = ((kb >> e) & 1u) ? v[e] * scale : 0.f;
          }
          st_store4<T>(out_t + at, v[0], v[1], v[2], v[3]);
        }
        dwacc[4 * j + 0] += dv[j].x * xv[j].x * r; dwacc[4 * j + 1] += dv[j].y * xv[j].y * r;
        dwacc[4 * j + 2] += dv[j].z * xv[j].z * r; dwacc[4 * j + 3] += dv[j].w * xv[j].w * r;
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) { xv[j] = xn[j]; dv[j] = dn[j]; rv[j] = rn[j]; }
  }
  int j = 0;
  for (int col = lane * 4; col < d; col += 256, ++j) {
    red[wave * d + col + 0] = dwacc[4 * j + 0]; red[wave * d + col + 1] = dwacc[4 * j + 1];
    red[wave * d + col + 2] = dwacc[4 * j + 2]; red[wave * d + col + 3] = dwacc[4 * j + 3];
  }
  __syncthreads();
  for (int col = threadIdx.x; col < d; col += 256)
    dw_part[(int64_t)blockIdx.x * d + col] = red[col] + red[d + col] + red[2 * d + col] + red[3 * d + col];
}
// out[col] (+)= sum over `parts` rows of part[p][col]   (second pass of every column reduction): 32 columns per block,
// 8 row groups per column, each walking its rows 8 at a time (independent loads: the first form issued one dependent
// round trip per row, 64 in a row = 16.7 us per launch), summed through LDS in a fixed order
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ part, float* __restrict__ out, int parts, int d, int accumulate) {
  __shared__ float sred[8][32];
  const int cx = threadIdx.x & 31, py = threadIdx.x >> 5;
  const int col = blockIdx.x * 32 + cx;
  float acc = 0.f;
  if (col < d) {
    int p = py;
    for (; p + 56 < parts; p += 64) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = part[(int64_t)(p + 8 * u) * d + col];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; p < parts; p += 8) acc += part[(int64_t)p * d + col];
  }
  sred[py][cx] = acc;
  __syncthreads();
  if (py == 0 && col < d) {
    float v = sred[0][cx];
#pragma unroll
    for (int u = 1; u < 8; ++u) v += sred[u][cx];
    out[col] = accumulate ? out[col] + v : v;
  }
}

// every RMSNorm weight gradient of a step in one launch: partial image j ([parts][d]) -> (accumulate: added to) out_base + off[j]
__global__ __launch_bounds__(256) void colsum_group_kernel(const float* __restrict__ part_all, const int64_t* __restrict__ offs, float* __restrict__ out_base,
                                                           int parts, int d, int accumulate) {
  // block = 64 columns (16 lanes x 16 bytes: 256-byte row pieces) x 16 row groups, eight rows in flight per thread; the first form read
  // 128-byte pieces one 4-byte element per lane (54 us for the step's 17 MB of partial rows)
  __shared__ float4 sred[16][16];
  const int j = blockIdx.y;
  const float* part = part_all + (int64_t)j * parts * d;
  const int cx = threadIdx.x & 15, py = threadIdx.x >> 4;
  const int col = blockIdx.x * 64 + 4 * cx;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (col < d) {
    for (int p = py; p < parts; p += 128) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(part + (int64_t)min(p + 16 * u, parts - 1) * d + col);
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (p + 16 * u < parts) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
    }
  }
  sred[py][cx] = acc;
  __syncthreads();
  if (py == 0 && col < d) {
    float4 v = sred[0][cx];
#pragma unroll
    for (int u = 1; u < 16; ++u) { const float4 o = sred[u][cx]; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
    float* out = out_base + offs[j] + col;
    if (accumulate) { v.x += out[0]; v.y += out[1]; v.z += out[2]; v.w += out[3]; }
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
  }
}

// ---- cross entropy (mean over labels != -100, hf: modeling_t5.py:1049-1054) + gradient of the logits ----
// one wave per row: row_loss[row] = logsumexp - logit[label] (0 if ignored); dlogits (T) = (softmax - onehot) / n_valid
template <typename T>
__global__ __launch_bounds__(256) void ce_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                 const float* __restrict__ inv_n, float* __restrict__ row_loss, T* __restrict__ dlogits,
                                                 int M, int V, int ldd) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* lg = logits + (int64_t)row * V;
  const int64_t lab = labels[row];
  const bool valid = lab >= 0 && lab < V;          // -100 (and anything out of range) is ignored, as torch's ignore_index
  float mx = -1e30f;
  for (int v = lane; v < V; v += 64) mx = fmaxf(mx, lg[v]);
  mx = wave_max(mx);
  float sum = 0.f;
  for (int v = lane; v < V; v += 64) sum += expf(lg[v] - mx);
  sum = wave_sum(sum);
  const float lse = mx + logf(sum), scale = inv_n[0];
  if (lane == 0) row_loss[row] = valid ? lse - lg[lab] : 0.f;
  T* dl = dlogits + (int64_t)row * ldd;
  for (int v = lane; v < ldd; v += 64) {
    float gval = 0.f;
    if (valid && v < V) gval = (expf(lg[v] - lse) - (v == (int)lab ? 1.f : 0.f)) * scale;
    dl[v] = from_f32<T>(gval);
  }
}
// loss = inv_n * sum(row_loss)  (single block, fixed order)
__global__ void loss_reduce_kernel(const float* __restrict__ row_loss, int M, const float* __restrict__ inv_n, float* __restrict__ loss) {
  __shared__ float part[256];
  float acc = 0.f;
  for (int i = threadIdx.x; i < M; i += 256) acc += row_loss[i];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = part[0] * inv_n[0];
}

// ---- embeddings ----
// conditioning rows of the encoder input: x[b, i, :] = table_i[idx[b, i], :]   (ref: music2midi/input.py:57-59)
__global__ void cond_gather_kernel(const float* __restrict__ params, const int64_t* __restrict__ tab_off, const int* __restrict__ tab_rows,
                                   int n_tab, const int64_t* __restrict__ idx, float* __restrict__ x, int S, int d) {
  const int b = blockIdx.x / n_tab, i = blockIdx.x - b * n_tab;
  int64_t id = idx[(int64_t)b * n_tab + i];
  if (id < 0 || id >= tab_rows[i]) id = 0;
  const float* src = params + tab_off[i] + id * d;
  float* dst = x + ((int64_t)b * S + i) * d;
  for (int c = threadIdx.x; c < d; c += blockDim.x) dst[c] = src[c];
}
// gradient of an embedding table: one block per table row v, G[v] = sum of dx[row] over the activation rows whose id is v, in a fixed
// order.  Pass 1 scans the ids 256 at a time and lists the matching rows in LDS (ballot + prefix counts keep them in order); pass 2
// gives every fourth listed row to one wave, eight rows in flight per wave (a lane reads 16 bytes of each), and the four waves' partial
// rows meet in LDS in wave order.  (Round 2 walked the matches one after another inside the scan: a hot row — the pad / start token of
// every clip's ragged tail, ~700 activation rows at 16 clips — paid one memory latency per match, 140 us of the step.)
// ids[i * id_stride + id_off] is the id of activation row (i * x_row_stride + x_row_off).
// thresh != 0: dx arrives through the dropout on the embeddings (hf: T5Stack dropout(inputs_embeds)); only the rows that are READ
// here are masked, as they are read.
// NW waves per block: 16 for the shared embedding (round 4: the hot row's ~700 matches are 6 batches of loads per wave instead of 22;
// the launch's time IS that row), 4 for the small conditioning tables.
constexpr int EMB_ROWS_IN_FLIGHT = 8;
template <int NW>
__global__ __launch_bounds__(64 * NW) void embed_bwd_kernel(const int64_t* __restrict__ ids, int n_ids, int id_stride, int id_off,
                                                        const float* __restrict__ dx, int64_t x_row_stride, int64_t x_row_off,
                                                        float* __restrict__ gtab, int d, int pad_to_zero_id, int V, DropKey dk, uint32_t thresh,
                                                        float scale, int accumulate) {
  extern __shared__ __align__(16) int emb_smem[];
  int* list = emb_smem;                                          // [round_up_4(n_ids)]
  float* part = reinterpret_cast<float*>(list + ((n_ids + 3) & ~3));      // [NW][256]: one column block of the waves' sums
  __shared__ int wave_cnt[NW];
  const uint64_t dkey = thresh ? drop_site_key(dk) : 0ull;
  const int v = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cnt = 0;
  for (int i0 = 0; i0 < n_ids; i0 += 64 * NW) {
    const int i = i0 + threadIdx.x;
    bool match = false;
    if (i < n_ids) {
      int64_t id = ids[(int64_t)i * id_stride + id_off];
      if (id < 0 || id >= V) id = pad_to_zero_id;
      match = id == v;
    }
    const unsigned long long m = __ballot(match);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int base = cnt, all = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { const int c = wave_cnt[w]; if (w < wave) base += c; all += c; }
    if (match) list[base + __popcll(m & ((1ull << lane) - 1ull))] = i;
    cnt += all;
    __syncthreads();
  }
  for (int c0 = 0; c0 < d; c0 += 256) {                          // column blocks of 256: lane -> columns c0 + 4 lane .. + 3
    const int c = c0 + 4 * lane;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < d) {
      for (int k0 = wave; k0 < cnt; k0 += NW * EMB_ROWS_IN_FLIGHT) {
        float4 rows[EMB_ROWS_IN_FLIGHT];
        uint32_t keep[EMB_ROWS_IN_FLIGHT];
#pragma unroll
        for (int rr = 0; rr < EMB_ROWS_IN_FLIGHT; ++rr) {
          const int k = k0 + NW * rr;
          rows[rr] = make_float4(0.f, 0.f, 0.f, 0.f);
          keep[rr] = 0xFu;
          if (k < cnt) {
            const int64_t roff = ((int64_t)list[k] * x_row_stride + x_row_off) * d + c;
            rows[rr] = *reinterpret_cast<const float4*>(dx + roff);
            if (thresh) keep[rr] = drop_keep4(dkey, roff, thresh);
          }
        }
#pragma unroll
        for (int rr = 0; rr < EMB_ROWS_IN_FLIGHT; ++rr) {
          const float sc = thresh ? scale : 1.0f;
          acc.x += (keep[rr] & 1u) ? rows[rr].x * sc : 0.f;
          acc.y += (keep[rr] & 2u) ? rows[rr].y * sc : 0.f;
          acc.z += (keep[rr] & 4u) ? rows[rr].z * sc : 0.f;
          acc.w += (keep[rr] & 8u) ? rows[rr].w * sc : 0.f;
        }
      }
    }
    *reinterpret_cast<float4*>(part + wave * 256 + 4 * lane) = acc;
    __syncthreads();
    const int cc = c0 + threadIdx.x;
    if (threadIdx.x < 256 && cc < d) {                           // the waves' partial rows in wave order: a fixed order of additions
      float sum = part[threadIdx.x];
#pragma unroll
      for (int w = 1; w < NW; ++w) sum += part[256 * w + threadIdx.x];
      float* gp = gtab + (int64_t)v * d + cc;
      *gp = accumulate ? *gp + sum : sum;
    }
    __syncthreads();
  }
}
constexpr int EMB_NW_SHARED = 16;      // waves per block of the shared-embedding launch
static size_t embed_bwd_smem(int n_ids, int nw = EMB_NW_SHARED) { return (size_t)((n_ids + 3) & ~3) * 4 + (size_t)nw * 256 * 4; }
// Final norm of a stack with the dropout that follows it (hf: T5Stack dropout(final_layer_norm(x))): y = T(x * rstd * w), then the
// mask on the ROUNDED value, as the separate in-place pass did — one wave per row, one launch instead of two.
template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_drop_kernel(const float* __restrict__ x, const float* __restrict__ w, T* __restrict__ out, int M, int d,
                                                           float eps, DropKey dk, uint32_t thresh, float scale) {
  const uint64_t key = thresh ? drop_site_key(dk) : 0ull;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + (int64_t)row * d;
  float ss = 0.f;
  for (int c = lane * 4; c < d; c += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + c);
    ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  }
  ss = wave_sum(ss);
  const float rstd = rsqrtf(ss / (float)d + eps);
  for (int c = lane * 4; c < d; c += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + c);
    const float4 gw = *reinterpret_cast<const float4*>(w + c);
    float y[4] = {to_f32(from_f32<T>(gw.x * (v.x * rstd))), to_f32(from_f32<T>(gw.y * (v.y * rstd))), to_f32(from_f32<T>(gw.z * (v.z * rstd))),
                  to_f32(from_f32<T>(gw.w * (v.w * rstd)))};
    const int64_t at = (int64_t)row * d + c;
    const uint32_t kb = drop_keep4(key, at, thresh);
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = ((kb >> e) & 1u) ? y[e] * scale : 0.f;
    st_store4<T>(out + at, y[0], y[1], y[2], y[3]);
  }
}
// Encoder input of a pass in place: rows [0, n_tab) of every clip from the conditioning tables (ref: music2midi/input.py:57-59), then
// the dropout on the embeddings over ALL rows (cond_gather_kernel + drop_inplace_kernel before).
__global__ __launch_bounds__(256) void enc_input_kernel(const float* __restrict__ params, const int64_t* __restrict__ tab_off, const int* __restrict__ tab_rows,
                                                        int n_tab, const int64_t* __restrict__ idx, float* __restrict__ x, int B, int S, int d, DropKey dk,
                                                        uint32_t thresh, float scale) {
  const uint64_t key = thresh ? drop_site_key(dk) : 0ull;
  const int q = d >> 2;
  const int64_t n4 = (int64_t)B * S * q, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i4 < n4; i4 += stride) {
    const int64_t row = i4 / q;
    const int c = (int)(i4 - row * q) * 4, b = (int)(row / S), s = (int)(row - (int64_t)b * S);
    float4 v;
    if (s < n_tab) {
      int64_t id = idx[(int64_t)b * n_tab + s];
      if (id < 0 || id >= tab_rows[s]) id = 0;
      v = *reinterpret_cast<const float4*>(params + tab_off[s] + id * d + c);
    } else {
      if (!thresh) continue;                                 // nothing to do for a feature row
      v = *reinterpret_cast<const float4*>(x + row * d + c);
    }
    if (thresh) {
      const uint32_t kb = drop_keep4(key, row * d + c, thresh);
      v = make_float4((kb & 1u) ? v.x * scale : 0.f, (kb & 2u) ? v.y * scale : 0.f, (kb & 4u) ? v.z * scale : 0.f, (kb & 8u) ? v.w * scale : 0.f);
    }
    *reinterpret_cast<float4*>(x + row * d + c) = v;
  }
}
// Decoder input embedding of the teacher-forced pass with its dropout: x[row] = dropout(table[ids[row]])
__global__ __launch_bounds__(256) void embed_rows_drop_kernel(const int64_t* __restrict__ ids, const float* __restrict__ table, float* __restrict__ x, int M,
                                                              int d, int V, int pad_id, DropKey dk, uint32_t thresh, float scale) {
  const uint64_t key = thresh ? drop_site_key(dk) : 0ull;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  int tok = (int)ids[row];
  if (tok < 0 || tok >= V) tok = pad_id;
  for (int c = lane * 4; c < d; c += 256) {
    float4 v = *reinterpret_cast<const float4*>(table + (int64_t)tok * d + c);
    const uint32_t kb = drop_keep4(key, (int64_t)row * d + c, thresh);
    v = make_float4((kb & 1u) ? v.x * scale : 0.f, (kb & 2u) ? v.y * scale : 0.f, (kb & 4u) ? v.z * scale : 0.f, (kb & 8u) ? v.w * scale : 0.f);
    *reinterpret_cast<float4*>(x + (int64_t)row * d + c) = v;
  }
}

// the three inputs of a pass into the trainer's own buffers (what a captured graph reads): x as 16-byte pieces, labels, conditioning indices
__global__ void stage_inputs_kernel(const float4* __restrict__ x, float4* __restrict__ x_dst, int64_t n4, const int64_t* __restrict__ lab,
                                    int64_t* __restrict__ lab_dst, int64_t nl, const int64_t* __restrict__ cond, int64_t* __restrict__ cond_dst, int64_t nc,
                                    float* __restrict__ gscale_dst, float gscale) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, n = n4 + nl + nc;
  if (gscale_dst && blockIdx.x == 0 && threadIdx.x == 0) *gscale_dst = gscale;      // the gradient factor of a scaled pass
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (i < n4) x_dst[i] = x[i];
    else if (i < n4 + nl) lab_dst[i - n4] = lab[i - n4];
    else cond_dst[i - n4 - nl] = cond[i - n4 - nl];
  }
}

// fp32 c = a + b (either may be null -> treated as 0)
__global__ void add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ c, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) c[i] = (a ? a[i] : 0.f) + (b ? b[i] : 0.f);
}


// declared in enc_kernels.hip (the forward RMSNorm is the inference kernel)
int launch_rmsnorm(int precision, const float* x, const float* w, void* out, int M, int d, float eps, hipStream_t st);
int launch_embed_rows(const int64_t* ids, const float* table, float* x, int M, int d, int V, int pad_id, hipStream_t st);

}  // namespace m2m

// ============================================================ trainer ====
using namespace m2m;

namespace {

struct TensorDesc {
  std::string name;        // state-dict key under `model.` of the reference's LightningModule
  int64_t off;             // floats into the flat buffers
  int rows, cols;          // 1-D tensors: rows = length, cols = 0
};

// A sub-layer: the offsets of its weights (floats into the flat buffers, build_layout) next to what its forward pass keeps for the
// backward pass (pointers into the arena, build_arena): h = the normed input, then the projections' outputs, P = the probabilities
// (whole-head kernels: their dropout keep words), ao = the attention output rows, kt = K and V transposed, [2][B*H][64][Sp]
// (kv_transpose_kernel, for the fused stripe products), lse = the row log-sum-exp [B*H][queries] of the whole-head kernels.
struct SelfAttn { int64_t ln, qkv, o; void *h, *qkv_out, *P, *ao, *kt; float* lse; };
struct CrossAttn { int64_t ln, q, kv, o; void *h, *q_out, *kv_out, *P, *ao, *kt; float* lse; };
struct FeedFwd { int64_t ln, wi, wo; void *h, *ab, *mid; };
struct EncLayer { SelfAttn self; FeedFwd ff; };
struct DecLayer { SelfAttn self; CrossAttn cross; FeedFwd ff; };
struct ProjMat { int64_t off; int N, K; };      // a fused projection group as one matrix [N][K] at parameter offset `off`

// build the relative-position tables for one (Sq, Sk) geometry: bucket of every (key - query) offset
std::vector<int> bucket_table(const m2m_t5_geometry& g, int Sq, int Sk, bool bidirectional) {
  std::vector<int> t((size_t)Sq + Sk - 1);
  for (int i = 0; i < Sq + Sk - 1; ++i) t[i] = m2m_rel_bucket(i - (Sq - 1), bidirectional ? 1 : 0, g.num_buckets, g.max_distance);
  return t;
}

}  // namespace

struct m2m_trainer {
  m2m_t5_geometry g;
  int precision, inner, n_cond;
  size_t es;
  int max_batch, max_enc, max_dec;
  std::vector<int> cond_rows;
  std::vector<TensorDesc> tensors;
  int64_t n_floats = 0;
  // offsets
  int64_t o_shared, o_lm, o_erb, o_drb, o_eln, o_dln;
  std::vector<EncLayer> enc;             // per layer: weight offsets and activation buffers (sized by build_layout, never resized after)
  std::vector<DecLayer> dec;
  std::vector<ProjMat> proj;             // every projection matrix (fused groups), encoder layers then decoder layers, without lm_head
  std::vector<int64_t> o_cond;
  // device memory owned by the trainer
  unsigned char* arena = nullptr;
  int64_t arena_bytes = 0;
  void* Wc = nullptr;                    // T copy of the parameters (bf16 mode; fp32 mode reads the master buffer)
  void* Wil = nullptr;                   // bf16 mode: the gate-pair matrices again, rows interleaved (same offsets; see weights_transpose_kernel)
  void* WT = nullptr;                    // every weight matrix TRANSPOSED, in T, at the same offsets (dX = dY . W as an NT product)
  void *tA = nullptr, *tB = nullptr;     // transposed activations of the current dW product: [features][Mp]
  float* kpart = nullptr;                // split-K partial tiles
  int64_t kpart_floats = 0;
  void* wt_blocks = nullptr;             // WtBlock table on the device
  int n_wt_blocks = 0;
  // activations (pointers into the arena)
  std::vector<float*> xe, xd;            // residual streams: 2*Le + 1 and 3*Ld + 1 buffers (a sub-layer's buffers: enc / dec above)
  void *hE = nullptr, *hD = nullptr;
  float *logits = nullptr, *sc = nullptr, *dxa = nullptr, *dxb = nullptr, *dh = nullptr, *dhE = nullptr, *dw_part = nullptr,
        *row_loss = nullptr, *inv_n = nullptr, *drel = nullptr, *etab = nullptr, *dtab = nullptr;
  void *dlog = nullptr, *dxT = nullptr, *dmid = nullptr, *dab = nullptr, *dO = nullptr, *dqkv = nullptr, *dS = nullptr, *dcq = nullptr,
       *dckv = nullptr;
  int64_t* dec_in = nullptr;
  int *ebucket = nullptr, *dbucket = nullptr;
  int64_t* cond_off_dev = nullptr;
  int* cond_rows_dev = nullptr;
  int64_t* pads_dev = nullptr;           // (offset, count) of the alignment gaps of the flat layout
  int n_pads = 0;
  int tab_S = -1, tab_L = -1;            // geometry the bucket tables on the device were built for
  // fp8 mode (M2M_PREC_FP8): storage type stays bf16, the projection products run on MXFP8 (mx8.hip)
  bool fp8 = false;
  // sw.fp8.fwd / fp8_dx / fp8_dw: which projection products run on MXFP8 (M2M_FP8_PARTS = subset of fwd,dx,dw).  Default: forward
  // and dX; the weight gradients take the grouped bf16 launch — on fp8 they need two transposing quantiser launches + a split-K
  // product + a reduce EACH (16 clips: 8.9 ms per step against 7.5 ms), for the least accuracy-critical third of the products
  TrainSwitches sw;                      // every environment switch of the trainer, latched by m2m_trainer_create
  EncSwitches enc_sw;                    // ... and those of the encoder-side kernels its passes launch (put in scope by m2m_train_forward_backward)
  using LinW = W8Lin;
  std::vector<LinW> lin;                // every projection matrix (fused groups), by parameter offset
  uint8_t* w8 = nullptr;                 // fp8 weights, both layouts, + scales
  void* w8_tiles = nullptr;
  int n_w8_tiles = 0;
  uint8_t *q8a = nullptr, *s8a = nullptr, *q8ta = nullptr, *s8ta = nullptr, *q8tb = nullptr, *s8tb = nullptr;
  // dropout (hf T5Config.dropout_rate; the reference trains in model.train() mode, ref train.py:33): off unless set
  float drop_scale = 1.f;
  uint32_t drop_thresh = 0;
  uint64_t drop_seed = 0;
  uint64_t *step_key_dev = nullptr, *step_ctr_dev = nullptr;   // key of the current pass / passes since set_dropout (device words:
                                                               // a captured graph advances them itself, see train_prologue_kernel)
  // gradient accumulation (m2m_train_forward_backward_acc, for the duration of one call): GM_SCALED = dlogits carry the factor
  // `gscale` (d (loss * gscale)); GM_ACC = the gradient writers add to the flat buffer.  The factor itself is not baked into a
  // graph: a staged pass reads it from the device word inv_n[3] (gscale_src), written by stage_inputs_kernel before every replay.
  enum { GM_SCALED = 1, GM_ACC = 2 };
  int gmode = 0;
  float gscale = 1.f;
  const float* gscale_src = nullptr;
  // The operands the weight-gradient products read (dxT, dab, dqkv, dcq, dckv) live in per-sub-layer buffers (rings, one
  // entry per use in a pass): the products of a whole step are issued as ONE grouped launch after the backward pass
  // (or, in fp8 mode, on the side stream while the main stream moves on), so nothing may be overwritten before.
  enum { K_DXT = 0, K_DAB, K_DQKV, K_DCQ, K_DCKV, K_KINDS };
  std::vector<void*> ring[K_KINDS];
  void* dw_probs_dev = nullptr;          // DwProb tables on the device: [N_SLOTS + 1 table slots][2 phases][128 entries] (see GraphSlot)
  int64_t drel_slot_floats = 0;          // one self-attention layer's per-stripe diagonal sums (t->drel holds Le + Ld of them, then the scratch)
  int64_t* norm_offs_dev = nullptr;      // parameter offsets of the RMSNorm weights, in the order the backward pass meets them: [N_SLOTS + 1][2][32]
  // data-parallel overlap (m2m_trainer_set_sync_stream): the backward pass is issued in two parts — decoder side, then encoder side —
  // and `sync_stream` is released (ev_mid) as soon as the decoder-side gradients are final, so their all-reduce runs beside the
  // encoder backward.  The layout keeps them in two flat ranges: [0, o_erb) (shared embedding, lm_head) and the decoder blocks.
  hipStream_t sync_stream = nullptr;
  hipEvent_t ev_mid = nullptr;
  int64_t dec_begin = 0, dec_end = 0;
  // streams / graph of the step (trainer-owned: the caller's stream may be the legacy default stream, which cannot capture)
  hipStream_t s_main = nullptr, s_side = nullptr;
  hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_ready = nullptr, ev_free[2] = {nullptr, nullptr};
  int64_t* labels_buf = nullptr;
  int64_t* cond_buf = nullptr;
  float* loss_dev = nullptr;
  struct GraphKey {
    const float* P = nullptr; float* G = nullptr; int B = 0, S = 0, L = 0; uint32_t thresh = 0; uint64_t seed = 0; bool split = false; int gmode = 0;
    bool operator==(const GraphKey& o) const {
      return P == o.P && G == o.G && B == o.B && S == o.S && L == o.L && thresh == o.thresh && seed == o.seed && split == o.split && gmode == o.gmode;
    }
  };
  // One captured graph PER SHAPE.  The grouped weight-gradient launch and the norm column sums read device-resident tables
  // (operand pointers, reduction lengths, tile counts) that depend on (B, S, L); a graph bakes the table's ADDRESS in, so every
  // cached shape owns a table slot of its own and a pass with another shape can never rewrite the table a kept graph replays
  // (training batches are padded to their longest label sequence, ref: music2midi/tokenizer.py:86-96, so L changes from batch
  // to batch and comes back).  The first call with a key runs directly and uploads the slot's tables, the second captures, later
  // ones replay; the least recently used slot is recycled (its graphs destroyed first).  Slot N_SLOTS serves the passes issued on
  // the caller's stream (no graph).
  static constexpr int N_SLOTS = 8;
  struct GraphSlot {
    GraphKey key;
    bool valid = false;
    int calls = 0;
    uint64_t last_use = 0;
    hipGraphExec_t gexec = nullptr, gexec2 = nullptr;      // gexec2: second half of a split pass
    int nodes = 0;                                         // nodes of the captured graph(s): launches per step
    std::vector<unsigned char> dw_probs_host[2];           // host images of the slot's device tables (re-uploaded only when they change);
    std::vector<int64_t> norm_offs_host[2];                // [1]: the second half of a split pass
  };
  GraphSlot slots[N_SLOTS + 1];
  int cur_slot = N_SLOTS;                // the table slot the pass being issued uses
  uint64_t tick = 0;
  // optimizer
  AfPlan af;
  unsigned char* af_mem = nullptr;
  int step = 0;
  int clip_mode = AF_CLIP_OFF;           // m2m_trainer_set_grad_clip: applied by every m2m_adafactor_step
  float clip_value = 0.f;                // norm: max_norm;  value: the clamp
};

namespace {

int64_t add_tensor(m2m_trainer* t, const std::string& name, int rows, int cols, int64_t& off) {
  const int64_t o = off;
  t->tensors.push_back({name, o, rows, cols});
  off = align_up(off + (int64_t)rows * (cols ? cols : 1), 64);
  return o;
}

void build_layout(m2m_trainer* t) {
  const m2m_t5_geometry& g = t->g;
  const int d = g.d_model, dff = g.d_ff, inner = t->inner, V = g.vocab_size, H = g.num_heads;
  int64_t off = 0;
  const std::string T5 = "transformer.";
  t->o_shared = add_tensor(t, T5 + "shared.weight", V, d, off);
  t->o_lm = add_tensor(t, T5 + "lm_head.weight", V, d, off);
  t->o_erb = add_tensor(t, T5 + "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", g.num_buckets, H, off);
  t->o_drb = add_tensor(t, T5 + "decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", g.num_buckets, H, off);
  t->o_eln = add_tensor(t, T5 + "encoder.final_layer_norm.weight", d, 0, off);
  t->o_dln = add_tensor(t, T5 + "decoder.final_layer_norm.weight", d, 0, off);
  // a projection group: the matrices `names` back to back WITHOUT padding, one fused [n * rows, cols] matrix to the products
  // (q|k|v, wi_0|wi_1, cross k|v; a single name: the matrix alone).  Recorded in t->proj: the one list of projection matrices.
  auto group = [&](const std::string& p, std::initializer_list<const char*> names, int rows, int cols) {
    const int64_t first = off;
    for (const char* n : names) {
      t->tensors.push_back({p + n + ".weight", off, rows, cols});
      off += (int64_t)rows * cols;
    }
    off = align_up(off, 64);
    t->proj.push_back({first, (int)names.size() * rows, cols});
    return first;
  };
  auto self_attn = [&](const std::string& p, SelfAttn& a) {
    a.ln = add_tensor(t, p + "layer_norm.weight", d, 0, off);
    a.qkv = group(p + "SelfAttention.", {"q", "k", "v"}, inner, d);
    a.o = group(p + "SelfAttention.", {"o"}, d, inner);
  };
  auto feed_fwd = [&](const std::string& p, FeedFwd& f) {
    f.ln = add_tensor(t, p + "layer_norm.weight", d, 0, off);
    f.wi = group(p + "DenseReluDense.", {"wi_0", "wi_1"}, dff, d);
    f.wo = group(p + "DenseReluDense.", {"wo"}, d, dff);
  };
  t->enc.resize(g.num_layers);
  for (int l = 0; l < g.num_layers; ++l) {
    const std::string p = T5 + "encoder.block." + std::to_string(l) + ".layer.";
    self_attn(p + "0.", t->enc[l].self);
    feed_fwd(p + "1.", t->enc[l].ff);
  }
  t->dec.resize(g.num_decoder_layers);
  t->dec_begin = off;
  for (int l = 0; l < g.num_decoder_layers; ++l) {
    const std::string p = T5 + "decoder.block." + std::to_string(l) + ".layer.";
    self_attn(p + "0.", t->dec[l].self);
    CrossAttn& c = t->dec[l].cross;
    c.ln = add_tensor(t, p + "1.layer_norm.weight", d, 0, off);
    c.q = group(p + "1.EncDecAttention.", {"q"}, inner, d);
    c.kv = group(p + "1.EncDecAttention.", {"k", "v"}, inner, d);
    c.o = group(p + "1.EncDecAttention.", {"o"}, d, inner);
    feed_fwd(p + "2.", t->dec[l].ff);
  }
  t->dec_end = off;
  t->o_cond.resize(t->n_cond);
  for (int i = 0; i < t->n_cond; ++i)
    t->o_cond[i] = add_tensor(t, "conditioning.embeds." + std::to_string(i) + ".weight", t->cond_rows[i], d, off);
  t->n_floats = off;
}

// -------------------------------------------------------------- arena
// One device allocation; every buffer is declared once on a Carver (carver.h), and the order of the declarations is the layout.
int build_optimizer(m2m_trainer* t) {
  std::vector<AfTensor> at;
  std::vector<AfBlock> ab;
  int row_off = 0, cfac_off = 0;
  int64_t col_off = 0, state_off = 0;
  for (const TensorDesc& td : t->tensors) {
    AfTensor a{};
    a.offset = td.off;
    a.rows = td.cols ? td.rows : 1;
    a.cols = td.cols ? td.cols : td.rows;
    a.row_off = row_off; a.cfac_off = cfac_off; a.col_off = col_off; a.state_off = state_off;
    a.block0 = (int)ab.size();
    a.nblocks = ceil_div(a.rows, AF_ROWS);
    for (int b = 0; b < a.nblocks; ++b) ab.push_back({(int)at.size(), b * AF_ROWS, col_off + (int64_t)b * a.cols});
    row_off += a.rows; cfac_off += a.cols; col_off += (int64_t)a.nblocks * a.cols;
    state_off += (a.rows > 1 ? a.rows : 0) + a.cols;
    at.push_back(a);
  }
  AfPlan& p = t->af;
  p.n_tensors = (int)at.size(); p.n_blocks = (int)ab.size(); p.state_floats = state_off;
  Carver c;
  c.take(p.tensors, (int64_t)at.size() * sizeof(AfTensor));
  c.take(p.blocks, (int64_t)ab.size() * sizeof(AfBlock));
  c.take(p.rowsum, (int64_t)row_off * 4);
  c.take(p.colpart, col_off * 4);
  c.take(p.blk_a, (int64_t)ab.size() * 4);
  c.take(p.blk_b, (int64_t)ab.size() * 4);
  c.take(p.state, state_off * 4);
  c.take(p.rfac, (int64_t)row_off * 4);
  c.take(p.cfac, (int64_t)cfac_off * 4);
  c.take(p.tstat, (int64_t)at.size() * 2 * 4);
  c.take(p.blk_g, (int64_t)ab.size() * 4);
  c.take(p.gn_words, 4 * 4);
  M2M_CHECK_HIP(hipMalloc((void**)&t->af_mem, (size_t)c.off));
  M2M_CHECK_HIP(hipMemset(t->af_mem, 0, (size_t)c.off));
  c.bind(t->af_mem);
  M2M_CHECK_HIP(hipMemcpy(p.tensors, at.data(), at.size() * sizeof(AfTensor), hipMemcpyHostToDevice));
  M2M_CHECK_HIP(hipMemcpy(p.blocks, ab.data(), ab.size() * sizeof(AfBlock), hipMemcpyHostToDevice));
  return M2M_OK;
}

int build_arena(m2m_trainer* t) {
  const m2m_t5_geometry& g = t->g;
  const int64_t es = (int64_t)t->es, d = g.d_model, dff = g.d_ff, inner = t->inner, V = g.vocab_size, H = g.num_heads;
  const int64_t B = t->max_batch, S = t->max_enc, L = t->max_dec;
  const int64_t Me = B * S, Md = B * L, Mx = Me > Md ? Me : Md;
  const int64_t lps = align_up(S, 8), lpl = align_up(L, 8), lpm = lps > lpl ? lps : lpl, Sm = S > L ? S : L;
  const int Le = g.num_layers, Ld = g.num_decoder_layers;
  using Tr = m2m_trainer;
  Carver c;
  auto T = [&](auto*& member, int64_t elems) { c.take(member, elems * es); };
  auto F = [&](float*& member, int64_t elems) { c.take(member, elems * 4); };
  // a layer's probability buffer [B*H][Sq][ldp]; the whole-head attention path keeps only its dropout keep words there ([B*H][ceil(Sk/32)][round_up_32(Sq)] x 4 bytes)
  auto PB = [&](int64_t Sq, int64_t Sk, int64_t ldp) { return std::max<int64_t>(B * H * Sq * ldp, B * H * ((Sk + 31) / 32) * align_up(Sq, 32) * 2); };
  // the containers the carver points into get their final size first (t->enc / t->dec have theirs from build_layout)
  t->xe.resize(2 * Le + 1);
  t->xd.resize(3 * Ld + 1);
  const int ring_len[Tr::K_KINDS] = {2 * Le + 3 * Ld, Le + Ld, Le + Ld, Ld, Ld};      // one entry per use in a pass
  for (int k = 0; k < Tr::K_KINDS; ++k) t->ring[k].resize(std::max(ring_len[k], 1));
  // ---- the layout: every declaration below is one buffer, in arena order
  for (float*& x : t->xe) F(x, Me * d);
  for (float*& x : t->xd) F(x, Md * d);
  for (EncLayer& e : t->enc) {
    T(e.self.h, Me * d); T(e.ff.h, Me * d); T(e.self.qkv_out, Me * 3 * inner); T(e.self.P, PB(S, S, lps)); T(e.self.ao, Me * inner);
    T(e.ff.ab, Me * 2 * dff); T(e.ff.mid, Me * dff);
  }
  for (DecLayer& e : t->dec) {
    T(e.self.h, Md * d); T(e.cross.h, Md * d); T(e.ff.h, Md * d); T(e.self.qkv_out, Md * 3 * inner); T(e.self.P, PB(L, L, lpl));
    T(e.self.ao, Md * inner); T(e.cross.q_out, Md * inner); T(e.cross.kv_out, Me * 2 * inner); T(e.cross.P, PB(L, S, lps));
    T(e.cross.ao, Md * inner); T(e.ff.ab, Md * 2 * dff); T(e.ff.mid, Md * dff);
  }
  for (EncLayer& e : t->enc) F(e.self.lse, B * H * Sm);
  for (DecLayer& e : t->dec) { F(e.self.lse, B * H * Sm); F(e.cross.lse, B * H * Sm); }
  const int64_t Sp32 = align_up(S, 32), Lp32 = align_up(L, 32);
  for (EncLayer& e : t->enc) T(e.self.kt, 2 * B * H * 64 * Sp32);
  for (DecLayer& e : t->dec) { T(e.self.kt, 2 * B * H * 64 * Lp32); T(e.cross.kt, 2 * B * H * 64 * Sp32); }
  T(t->hE, Me * d); T(t->hD, Md * d);
  F(t->logits, Md * V); F(t->sc, B * H * Sm * lpm);
  F(t->dxa, Mx * d); F(t->dxb, Mx * d); F(t->dh, Mx * d); F(t->dhE, Me * d);
  F(t->dw_part, (int64_t)RN_BLOCKS * d * (2 * Le + 3 * Ld + 2));
  c.take(t->norm_offs_dev, (int64_t)(Tr::N_SLOTS + 1) * 64 * 8);
  F(t->row_loss, Md); F(t->inv_n, 64);
  // per self-attention layer a slot of per-stripe diagonal sums, then the stacks' reduction scratch, then bias_grad's own
  t->drel_slot_floats = B * H * std::max<int64_t>(2 * Sm, ((Sm + 31) / 32) * (Sm + 32));
  F(t->drel, (int64_t)(Le + Ld) * t->drel_slot_floats + (int64_t)std::max(Le, Ld) * H * 2 * Sm + B * H * 2 * Sm);
  F(t->etab, H * (2 * S)); F(t->dtab, H * (2 * L));
  T(t->dlog, Md * align_up(V, 8));
  T(t->dxT, Mx * d); T(t->dmid, Mx * dff); T(t->dab, Mx * 2 * dff); T(t->dO, Mx * inner); T(t->dqkv, Mx * 3 * inner);
  T(t->dS, B * H * Sm * lpm); T(t->dcq, Md * inner); T(t->dckv, Me * 2 * inner);
  c.take(t->labels_buf, Md * 8); c.take(t->cond_buf, B * 8 * 8);
  c.take(t->step_key_dev, 256);          // its words: [0] the key, [1] step_ctr_dev, [4] loss_dev (set behind the bind)
  c.take(t->dec_in, Md * 8);
  c.take(t->ebucket, 2 * S * 4); c.take(t->dbucket, 2 * L * 4);
  c.take(t->cond_off_dev, 64 * 8); c.take(t->cond_rows_dev, 64 * 4);
  c.take(256);                           // reserved (a counter that is gone): keeps every offset behind it where it was
  if (t->precision == M2M_PREC_BF16) { T(t->Wc, t->n_floats); T(t->Wil, t->n_floats); }
  T(t->WT, t->n_floats);
  // ring entry 0 of a kind is the buffer declared above (set behind the bind), the others follow here
  for (int i = 1; i < ring_len[Tr::K_DXT]; ++i) T(t->ring[Tr::K_DXT][i], Mx * d);
  for (int i = 1; i < ring_len[Tr::K_DAB]; ++i) { T(t->ring[Tr::K_DAB][i], Mx * 2 * dff); T(t->ring[Tr::K_DQKV][i], Mx * 3 * inner); }
  for (int i = 1; i < ring_len[Tr::K_DCQ]; ++i) { T(t->ring[Tr::K_DCQ][i], Md * inner); T(t->ring[Tr::K_DCKV][i], Me * 2 * inner); }
  c.take(t->dw_probs_dev, (int64_t)(Tr::N_SLOTS + 1) * 256 * (int64_t)sizeof(DwProb));
  const int64_t Mxp = align_up(Mx, 8), fmax = std::max<int64_t>(std::max<int64_t>(3 * inner, 2 * dff), align_up(V, 8));
  const int64_t fmin = std::max<int64_t>(std::max<int64_t>(dff, inner), d);
  T(t->tA, fmax * Mxp); T(t->tB, fmin * Mxp);
  t->kpart_floats = std::max<int64_t>((int64_t)8 << 20, fmax * std::max<int64_t>(dff, d) + 64);
  F(t->kpart, t->kpart_floats);
  // weight-transpose table: lm_head, then every projection group as one matrix [N][K], in 64 x 64 tiles
  std::vector<WtBlock> wtb;
  auto wt_add = [&](const ProjMat& m) {
    const int il = (m.N == 2 * (int)dff && m.K == (int)d && dff % 32 == 0) ? (int)dff : 0;      // the gate pairs
    for (int tn = 0; tn < ceil_div(m.N, 64); ++tn)
      for (int tk = 0; tk < ceil_div(m.K, 64); ++tk) wtb.push_back({m.off, m.N, m.K, tn, tk, il});
  };
  wt_add({t->o_lm, (int)V, (int)d});
  for (const ProjMat& m : t->proj) wt_add(m);
  t->n_wt_blocks = (int)wtb.size();
  c.take(t->wt_blocks, (int64_t)wtb.size() * sizeof(WtBlock));
  std::vector<int64_t> pads;             // gaps between consecutive tensors of the flat layout (and behind the last one)
  {
    std::vector<std::pair<int64_t, int64_t>> spans;
    for (const TensorDesc& td : t->tensors) spans.push_back({td.off, (int64_t)td.rows * (td.cols ? td.cols : 1)});
    std::sort(spans.begin(), spans.end());
    int64_t pos = 0;
    for (const auto& sp : spans) {
      if (sp.first > pos) { pads.push_back(pos); pads.push_back(sp.first - pos); }
      pos = std::max(pos, sp.first + sp.second);
    }
    if (t->n_floats > pos) { pads.push_back(pos); pads.push_back(t->n_floats - pos); }
  }
  t->n_pads = (int)(pads.size() / 2);
  c.take(t->pads_dev, (int64_t)std::max<size_t>(pads.size(), 2) * 8);
  // fp8 mode: MXFP8 copies of every projection matrix (lm_head stays bf16) + quantised-activation scratch
  std::vector<W8Tile> w8t;
  if (t->fp8) {
    int64_t w8_bytes = 0;
    for (const ProjMat& m : t->proj) t->lin.push_back(w8_add_matrix(m.off, m.N, m.K, w8_bytes, w8t));
    t->n_w8_tiles = (int)w8t.size();
    const int64_t Mp128 = align_up(Mx, 128), f8 = align_up(fmax, 128), f8b = align_up(fmin, 128);
    c.take(t->w8, w8_bytes); c.take(t->w8_tiles, (int64_t)w8t.size() * sizeof(W8Tile));
    c.take(t->q8a, Mx * f8); c.take(t->s8a, Mx * (f8 / 32));
    c.take(t->q8ta, f8 * Mp128); c.take(t->s8ta, f8 * (Mp128 / 32));
    c.take(t->q8tb, f8b * Mp128); c.take(t->s8tb, f8b * (Mp128 / 32));
  }
  t->arena_bytes = c.off;
  hipError_t e = hipMalloc((void**)&t->arena, (size_t)c.off);
  if (e != hipSuccess) { set_error("m2m_trainer_create: hipMalloc(%lld) failed: %s", (long long)c.off, hipGetErrorString(e)); return M2M_ERR_NOMEM; }
  M2M_CHECK_HIP(hipMemset(t->arena, 0, (size_t)c.off));
  c.bind(t->arena);
  t->step_ctr_dev = t->step_key_dev + 1; t->loss_dev = (float*)(t->step_key_dev + 4);
  void* const first[Tr::K_KINDS] = {t->dxT, t->dab, t->dqkv, t->dcq, t->dckv};
  for (int k = 0; k < Tr::K_KINDS; ++k) t->ring[k][0] = first[k];
  M2M_CHECK_HIP(hipMemcpy(t->wt_blocks, wtb.data(), wtb.size() * sizeof(WtBlock), hipMemcpyHostToDevice));
  if (!pads.empty()) M2M_CHECK_HIP(hipMemcpy(t->pads_dev, pads.data(), pads.size() * 8, hipMemcpyHostToDevice));
  if (t->fp8) M2M_CHECK_HIP(hipMemcpy(t->w8_tiles, w8t.data(), w8t.size() * sizeof(W8Tile), hipMemcpyHostToDevice));
  M2M_CHECK_HIP(hipMemcpy(t->cond_off_dev, t->o_cond.data(), t->o_cond.size() * 8, hipMemcpyHostToDevice));
  M2M_CHECK_HIP(hipMemcpy(t->cond_rows_dev, t->cond_rows.data(), t->cond_rows.size() * 4, hipMemcpyHostToDevice));
  return M2M_OK;
}

// ------------------------------------------------------------ operand views of the attention products
// A matrix per (clip b, head h): element (row, col) at p + b * sb + h * sh + row * ld + col, in elements of its own type.  An activation
// split into heads ({p, ld, sb}: HeadAttnArgs' convention) has its heads DK columns apart.  km: stored k-major, a product reads it transposed.
struct Mat {
  const void* p;
  int64_t ld, sb, sh = DK;
  int km = 0;
  Mat t() const { Mat m = *this; m.km = 1; return m; }
};
struct MatProd { Mat A, B, C; };      // C = A . B^T
// What the attention core of a layer works on (attn_core_fwd / attn_core_bwd)
struct AttnDesc {
  Mat q, k, v;                 // V sits `inner` columns behind K
  int Sq, Sk, causal, site;    // site: the dropout site of the probabilities
  const float* tab;            // bias table, or null
  void *Pm, *kt, *ao;          // the layer's P (whole-head kernels: its keep words), its K^T | V^T image, its output rows [nB * Sq, inner]
  float* lse;
  // backward only
  const void* dO;              // layout of ao
  Mat dq, dk, dv;
  const int* buckets;          // bias gradient (null: none): bucket table, destination, and `accumulate` as bias_grad* take it
  float* Gbias;
  int bias_accumulate;
};

// ------------------------------------------------------------ typed helpers
template <typename T>
struct Ops {
  m2m_trainer* t;
  hipStream_t st;
  const float* P;      // master parameters (fp32)
  const T* W(int64_t off) const { return (t->precision == M2M_PREC_BF16 ? reinterpret_cast<const T*>(t->Wc) : reinterpret_cast<const T*>(P)) + off; }

  // fp8 mode: the projection matrix that starts at parameter offset `off`, or null (lm_head, non-projection operands)
  const m2m_trainer::LinW* lin8(int64_t off) const {
    if (!t->fp8) return nullptr;
    for (const auto& w : t->lin) if (w.off == off) return &w;
    return nullptr;
  }
  float* Gbase = nullptr;     // flat gradient buffer of this call (dW recognises its weight by the output offset)
  // accumulate mode (m2m_train_forward_backward_acc): every writer of the flat gradient buffer adds its result to what the
  // buffer holds instead of overwriting it.  (Not the bias reductions' `accumulate` argument: that one sums the layers of a
  // stack into their shared table within ONE pass.)
  int gacc = 0;

  // dropout sites: one key per (layer, place); site < 0 or p == 0: no dropout
  bool dropping(int site) const { return site >= 0 && t->drop_thresh != 0; }
  DropKey key(int site) const { return DropKey{t->step_key_dev, (uint64_t)site * 0x9E3779B97F4A7C15ull}; }
  // what a kernel with dropout in it takes for a site: (key, thresh, scale), the key null and thresh 0 where the site does not drop
  struct Drop { DropKey key; uint32_t thresh; float scale; };
  Drop drop(int site) const { return dropping(site) ? Drop{key(site), t->drop_thresh, t->drop_scale} : Drop{DropKey{nullptr, 0}, 0u, t->drop_scale}; }
  // ... and the same as the dropout fields of a product's arguments (BGemmArgs, GemmArgs), left zero where the site does not drop
  template <typename Args>
  void drop_fields(Args& a, int site) const {
    if (!dropping(site)) return;
    a.drop_thresh = t->drop_thresh; a.drop_scale = t->drop_scale; a.drop_key = key(site).salt; a.drop_step = t->step_key_dev;
  }

  // ---- weight-gradient products.  A backward sub-layer brackets itself with begin_sub(kinds) / end_sub(): begin_sub
  // points t->dxT ... at fresh ring entries, dW() calls in between are queued.  Grouped mode: the queue becomes ONE launch
  // after the backward pass (flush_group).  Side-stream mode (fp8): end_sub() hands the queue to the side stream behind
  // everything the main stream has issued so far.
  hipStream_t st2 = nullptr;
  bool group = false;
  mutable std::vector<std::function<int(hipStream_t)>> pending;
  mutable std::vector<DwProb> probs;
  mutable std::vector<int64_t> norm_offs;
  struct BiasJob { const int* buckets; float* Gtab; int nB, Sq, Sk, first_slot, layers; };
  mutable std::vector<BiasJob> bias_jobs;          // grouped mode: per stack, the self-attention layers whose diagonal sums wait in t->drel slots
  mutable int drel_slots = 0;
  // grouped mode: the RMSNorm backward of a sub-layer also emits its dx in the GEMM-input type for the sub-layer that runs next
  // (site = that sub-layer's branch-output dropout site; -2: nobody), straight into that sub-layer's dxT ring entry
  mutable int after_site = -2;
  struct PreCvt { const float* src = nullptr; const void* dst = nullptr; int site = -2; };
  mutable PreCvt pre;
  mutable int pos[m2m_trainer::K_KINDS] = {0, 0, 0, 0, 0};
  mutable int sub = 0;
  mutable bool used[2] = {false, false};
  int begin_sub(unsigned kinds) const {
    void** dst[m2m_trainer::K_KINDS] = {&t->dxT, &t->dab, &t->dqkv, &t->dcq, &t->dckv};
    if (group) {                           // a ring entry per use: nothing is overwritten before the grouped launch
      for (int k = 0; k < m2m_trainer::K_KINDS; ++k)
        if (kinds & (1u << k)) { *dst[k] = t->ring[k][pos[k] % t->ring[k].size()]; pos[k] += 1; }
      return M2M_OK;
    }
    // side-stream / single-stream mode: two alternating sets (they stay in the Infinity Cache; fresh buffers per
    // sub-layer measured 10.9 vs 10.0 ms per fp8 step); a set is rewritten only after the side stream has read it
    const int slot = sub & 1;
    if (st2 && used[slot]) M2M_CHECK_HIP(hipStreamWaitEvent(st, t->ev_free[slot], 0));
    for (int k = 0; k < m2m_trainer::K_KINDS; ++k)
      if (kinds & (1u << k)) *dst[k] = t->ring[k][slot];
    return M2M_OK;
  }
  int end_sub() const {
    if (group) return M2M_OK;
    const int slot = sub & 1;
    sub += 1;
    if (!st2 || pending.empty()) return M2M_OK;
    M2M_CHECK_HIP(hipEventRecord(t->ev_ready, st));
    M2M_CHECK_HIP(hipStreamWaitEvent(st2, t->ev_ready, 0));
    for (auto& f : pending) { const int rc = f(st2); if (rc != M2M_OK) { pending.clear(); return rc; } }
    pending.clear();
    M2M_CHECK_HIP(hipEventRecord(t->ev_free[slot], st2));
    used[slot] = true;
    return M2M_OK;
  }
  int join_side() const {                  // the main stream continues only after every queued product has finished
    if (!st2) return M2M_OK;
    for (int p = 0; p < 2; ++p)
      if (used[p]) M2M_CHECK_HIP(hipStreamWaitEvent(st, t->ev_free[p], 0));
    return M2M_OK;
  }
  // A split pass (t->sync_stream) flushes twice: `phase` picks the half of the device tables (and the host image) a flush uses,
  // so both halves stay constant from step to step and a captured graph never sees a table change.
  mutable int phase = 0;
  mutable int norm_slot_base = 0;          // partial images already handed to an earlier flush of this pass keep their slices
  int flush_norms() const {
    if (!group || norm_offs.empty()) return M2M_OK;
    M2M_REQUIRE(norm_offs.size() <= 32 && (int)norm_offs.size() <= 2 * t->g.num_layers + 3 * t->g.num_decoder_layers + 2, "training: too many norms");
    int64_t* const offs_dev = t->norm_offs_dev + 64 * t->cur_slot + 32 * phase;
    std::vector<int64_t>& offs_host = t->slots[t->cur_slot].norm_offs_host[phase];
    if (offs_host != norm_offs) {
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      (void)hipStreamIsCapturing(st, &cs);
      M2M_REQUIRE(cs == hipStreamCaptureStatusNone, "training: the norm table changed inside a graph capture");
      M2M_CHECK_HIP(hipStreamSynchronize(st));
      M2M_CHECK_HIP(hipMemcpy(offs_dev, norm_offs.data(), norm_offs.size() * 8, hipMemcpyHostToDevice));
      offs_host = norm_offs;
    }
    const int d = t->g.d_model;
    hipLaunchKernelGGL(colsum_group_kernel, dim3(ceil_div(d, 64), (unsigned)norm_offs.size()), dim3(256), 0, st,
                       t->dw_part + (int64_t)norm_slot_base * RN_BLOCKS * d, offs_dev, Gbase, RN_BLOCKS, d, gacc);
    M2M_CHECK_HIP(hipGetLastError());
    norm_slot_base += (int)norm_offs.size();
    norm_offs.clear();
    return M2M_OK;
  }
  int flush_group() const {
    if (!group || probs.empty()) return M2M_OK;
    M2M_REQUIRE(probs.size() <= 128, "training: %zu weight-gradient products exceed the table", probs.size());
    unsigned char* const tab_dev = reinterpret_cast<unsigned char*>(t->dw_probs_dev) + (size_t)(2 * t->cur_slot + phase) * 128 * sizeof(DwProb);
    std::vector<unsigned char>& tab_host = t->slots[t->cur_slot].dw_probs_host[phase];
    int tiles = 0;
    for (DwProb& p : probs) { p.tn2 = ceil_div(p.g.N2, 128); p.tile0 = tiles; tiles += ceil_div(p.g.N1, 128) * p.tn2; }
    const size_t bytes = probs.size() * sizeof(DwProb);
    if (tab_host.size() != bytes || memcmp(tab_host.data(), probs.data(), bytes) != 0) {
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      (void)hipStreamIsCapturing(st, &cs);
      M2M_REQUIRE(cs == hipStreamCaptureStatusNone, "training: the weight-gradient table changed inside a graph capture");
      M2M_CHECK_HIP(hipStreamSynchronize(st));                 // nothing in flight still reads the old table
      M2M_CHECK_HIP(hipMemcpy(tab_dev, probs.data(), bytes, hipMemcpyHostToDevice));
      tab_host.assign(reinterpret_cast<const unsigned char*>(probs.data()), reinterpret_cast<const unsigned char*>(probs.data()) + bytes);
    }
    const int rc = launch_dw_group(t->precision, (const DwProb*)tab_dev, (int)probs.size(), tiles, st, t->sw);
    probs.clear();
    return rc;
  }
  int mm(int epi, const void* A, int64_t lda, int akm, const void* B, int64_t ldb, int bkm, void* C, int64_t ldc, int M, int N, int K,
         const float* R = nullptr, int drop_site = -1) const {
    BGemmArgs g{};
    g.A = A; g.B = B; g.C = C; g.R = R; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc; g.a_kmajor = akm; g.b_kmajor = bkm;
    g.nb1 = 1; g.nb2 = 1; g.alpha = 1.0f;
    drop_fields(g, drop_site);
    if (!akm && !bkm && t->fp8 && t->sw.fp8.fwd) {          // a forward projection Y = X . W^T on MXFP8 operands
      const int64_t off = reinterpret_cast<const T*>(B) - W(0);
      if (const m2m_trainer::LinW* w = lin8(off))
        return mx8_fwd(epi, A, lda, t->w8 + w->q, t->w8 + w->qs, t->q8a, t->s8a, C, ldc, R, M, N, K,
                       MxDrop{g.drop_thresh, g.drop_scale, g.drop_key, g.drop_step}, t->sw, st);
    }
    // dense NT products with K % 64 == 0 go through the inference path's tuned kernel (128x128 tiles, register-prefetched
    // staging, XCD-aware tile order): every forward projection and every dX product qualifies
    if (!akm && !bkm && K % 64 == 0 && lda == K && ldb == K && t->sw.tuned_gemm) {
      GemmArgs a{};
      a.A = A; a.W = B; a.M = M; a.N = N; a.K = K; a.out = C; a.ldo = (int)ldc; a.vt_which = -1;
      if (epi == TG_STORE_T) return launch_gemm(t->precision, EPI_STORE, a, st);
      if (epi == TG_STORE_F32) return launch_gemm(t->precision, EPI_STORE_F32, a, st);
      if (epi == TG_ACC_F32) return launch_gemm(t->precision, EPI_RESID, a, st);
      a.resid = R;
      drop_fields(a, drop_site);
      return launch_gemm(t->precision, EPI_RESID, a, st);
    }
    return launch_bgemm(t->precision, epi, g, st, t->sw);
  }
  // gradient entering a (possibly dropped) branch, in the GEMM-input type
  int cvt_branch(const float* src, void* dst, int64_t n, int site) const {
    if (pre.src == src && pre.dst == dst && pre.site == site) { pre = PreCvt{}; return M2M_OK; }      // the producing norm already wrote it
    pre = PreCvt{};
    if (!dropping(site)) return launch_cvt(t->precision, src, dst, n, st);
    hipLaunchKernelGGL(cvt_drop_kernel<T>, dim3(grid_1d(n)), dim3(256), 0, st, src, (T*)dst, n, key(site), t->drop_thresh, t->drop_scale);
    M2M_CHECK_HIP(hipGetLastError());
    return M2M_OK;
  }
  // the layouts only this trainer knows: P / dS / the fp32 scores [nB][H][Sq][ldp] with ldp = align_up(Sk, 8), and the activations
  Mat pmat(const void* p, int Sq, int Sk) const { const int64_t ldp = align_up(Sk, 8); return Mat{p, ldp, t->g.num_heads * Sq * ldp, Sq * ldp}; }
  // column group i of n in a projection's output [rows, n * inner] with Sx rows per clip (q | k | v: n = 3; k | v: n = 2; ao, dO, cq: n = 1)
  Mat part(const void* p, int n, int i, int Sx) const { return Mat{(const T*)p + i * t->inner, n * t->inner, (int64_t)Sx * n * t->inner}; }
  // C[M,N] (epi)= A[M,K] . B[N,K]^T batched over (clip, head); m2 (BGemmArgs pair mode): a second product of the same shape in the same
  // launch, whose A and C share pitch, strides and orientation with the first
  int mmbh(int epi, const MatProd& m, int nB, int M, int N, int K, const MatProd* m2 = nullptr) const {
    BGemmArgs g{};
    g.A = m.A.p; g.B = m.B.p; g.C = const_cast<void*>(m.C.p); g.R = nullptr; g.M = M; g.N = N; g.K = K; g.lda = m.A.ld; g.ldb = m.B.ld; g.ldc = m.C.ld;
    g.a_kmajor = m.A.km; g.b_kmajor = m.B.km;
    g.nb1 = nB; g.nb2 = t->g.num_heads; g.sA1 = m.A.sb; g.sA2 = m.A.sh; g.sB1 = m.B.sb; g.sB2 = m.B.sh; g.sC1 = m.C.sb; g.sC2 = m.C.sh; g.alpha = 1.0f;
    if (m2) { g.A2 = m2->A.p; g.B2 = m2->B.p; g.C2 = const_cast<void*>(m2->C.p); g.ldb2 = m2->B.ld; g.sB1_2 = m2->B.sb; g.sB2_2 = m2->B.sh; }
    return launch_bgemm(t->precision, epi, g, st, t->sw);
  }
  int mmbh2(int epi, const MatProd& m, const MatProd& m2, int nB, int M, int N, int K) const { return mmbh(epi, m, nB, M, N, K, &m2); }
  // dX[M, Kw] (epi) = dY[M, Nw] . W   for a weight stored [Nw][Kw]: an NT product against the transposed copy WT [Kw][Nw]
  int dX(int epi, const void* dY, int64_t ldy, int64_t w_off, int Nw, int Kw, void* C, int64_t ldc, int M) const {
    if (const m2m_trainer::LinW* w = t->sw.fp8.dx ? lin8(w_off) : nullptr)      // fp8 mode: dY in the gradient format, W^T in e4m3
      return mx8_dx(epi, dY, ldy, Nw, Kw, t->w8 + w->qt, t->w8 + w->qts, w->Np, t->q8a, t->s8a, C, ldc, nullptr, M, MxDrop{}, t->sw, st);
    return mm(epi, dY, ldy, 0, reinterpret_cast<const T*>(t->WT) + w_off, Nw, 0, C, ldc, M, Kw, Nw);
  }
  // G[Ny, Kx] = dY[M, Ny]^T . X[M, Kx]: both operands are transposed once (coalesced, through LDS) into [features][Mp]
  // scratch, then it is a plain NT product with the M rows as the reduction, split over k so that the few output tiles
  // of a weight gradient still fill the chip; the k-slices are summed in a fixed order.
  int dW(const void* dY, int64_t ldy, int Ny, const void* X, int64_t ldx, int Kx, float* Gout, int M) const {
    if (group) {
      const int Ea = t->precision == M2M_PREC_BF16 ? 8 : 4;
      if (Ny % Ea == 0 && Kx % Ea == 0 && ldy % Ea == 0 && ldx % Ea == 0 && (reinterpret_cast<uintptr_t>(dY) & 15) == 0 &&
          (reinterpret_cast<uintptr_t>(X) & 15) == 0) {
        DwProb p;
        memset(&p, 0, sizeof(p));                     // the table is compared bytewise: no uninitialised padding
        p.g.A = dY; p.g.B = X; p.g.C = Gout; p.g.N1 = Ny; p.g.N2 = Kx; p.g.K = M; p.g.lda = ldy; p.g.ldb = ldx; p.g.ldc = Kx; p.g.ksplit = 1; p.g.kchunk = M;
        p.g.accum = gacc;
        probs.push_back(p);
        return M2M_OK;
      }
      return dW_on(st, dY, ldy, Ny, X, ldx, Kx, Gout, M);
    }
    if (!st2) return dW_on(st, dY, ldy, Ny, X, ldx, Kx, Gout, M);
    pending.push_back([=](hipStream_t s) { return dW_on(s, dY, ldy, Ny, X, ldx, Kx, Gout, M); });
    return M2M_OK;
  }
  int dW_on(hipStream_t st, const void* dY, int64_t ldy, int Ny, const void* X, int64_t ldx, int Kx, float* Gout, int M) const {
    if (Gbase && t->sw.fp8.dw && lin8(Gout - Gbase))        // fp8 mode: dY^T (gradient format) . X^T (e4m3), blocks along the M rows
      return mx8_dw(dY, ldy, Ny, X, ldx, Kx, t->q8ta, t->s8ta, t->q8tb, t->s8tb, t->kpart, t->kpart_floats, Gout, gacc, M, t->sw, st);
    // (the generic kernel's k-major staging — 2-byte LDS scatters — and the transpose-then-NT route it replaced cost
    //  ~30 us per weight gradient at 16 clips; M2M_TRAIN_DW_OLD=1 keeps them for comparison)
    const int Ealign = t->precision == M2M_PREC_BF16 ? 8 : 4;
    if (!t->sw.dw_old && Ny % Ealign == 0 && Kx % Ealign == 0 && ldy % Ealign == 0 && ldx % Ealign == 0)
      return launch_dw_gemm(t->precision, dY, ldy, Ny, X, ldx, Kx, M, Gout, Kx, t->kpart, t->kpart_floats, st, gacc, t->sw);
    const int Mp = (int)align_up(M, 8);
    BGemmArgs g{};
    g.C = Gout; g.M = Ny; g.N = Kx; g.K = M; g.ldc = Kx; g.nb1 = 1; g.nb2 = 1; g.alpha = 1.0f;
    if (t->sw.dw_kmajor == 1 || (t->sw.dw_kmajor < 0 && M < 8192)) {
      g.A = dY; g.B = X; g.lda = ldy; g.ldb = ldx; g.a_kmajor = 1; g.b_kmajor = 1;
    } else {
      const int rc = launch_transpose_pair(t->precision, dY, ldy, Ny, X, ldx, Kx, t->tA, t->tB, M, Mp, st);
      if (rc != M2M_OK) return rc;
      g.A = t->tA; g.B = t->tB; g.lda = Mp; g.ldb = Mp;
    }
    const int tiles = ceil_div(Ny, TG_BM) * ceil_div(Kx, TG_BN);
    int ks = 1024 / tiles;
    if (ks > 32) ks = 32;
    while (ks > 1 && ((int64_t)ks * Ny * Kx > t->kpart_floats || ceil_div(M, ks) < 64)) --ks;
    if (ks > 1) { g.ksplit = ks; g.kchunk = (int)align_up(ceil_div(M, ks), TG_BK_MAX); g.ksplit = ceil_div(M, g.kchunk); g.Cpart = t->kpart; }
    return launch_bgemm(t->precision, gacc ? TG_ACC_F32 : TG_STORE_F32, g, st, t->sw);
  }
  int cvt(const float* src, void* dst, int64_t n) const { return launch_cvt(t->precision, src, dst, n, st); }
  // (A row-complete residual product that carries the next sub-layer's RMSNorm in its epilogue — 32 whole rows per workgroup, the
  //  weight matrix streamed through every one of the 131 workgroups by DMA — was built and measured in round 3 (commit 0a97748,
  //  tools/shared_stream.hip for the streaming ceiling): 13.4 us at K = 512 and 23.9 us at K = 1 152 against 9.6 + 5.2 and 13.9 + 5.2 us
  //  for the product and the norm as two launches.  Per 64-deep step a workgroup moves 52 KB into LDS and reads 64 KB of fragments
  //  back: ~0.6 us of LDS and L2-to-CU time per step on HALF the CUs, where the tiled product spreads the same 54 MB over all of them.)
  int mm_resid(const void* A, int64_t w_off, float* x_out, int M, int N, int K, const float* x_in, int site) const {
    return mm(TG_RESID_F32, A, K, 0, W(w_off), K, 0, x_out, N, M, N, K, x_in, site);
  }
  int norm(const float* x, int64_t w_off, void* out, int M) const { return launch_rmsnorm(t->precision, x, P + w_off, out, M, t->g.d_model, t->g.layer_norm_eps, st); }
  int norm_drop(const float* x, int64_t w_off, void* out, int M, int site) const {
    if (!dropping(site)) return norm(x, w_off, out, M);
    hipLaunchKernelGGL(rmsnorm_drop_kernel<T>, dim3(ceil_div(M, 4)), dim3(256), 0, st, x, P + w_off, (T*)out, M, t->g.d_model, t->g.layer_norm_eps, key(site),
                       t->drop_thresh, t->drop_scale);
    M2M_CHECK_HIP(hipGetLastError());
    return M2M_OK;
  }
  int norm_bwd(const float* x, int64_t w_off, const float* dy, const float* dx_res, float* dx_out, float* G, int M, int dy_site = -1) const {
    const int d = t->g.d_model;
    // (summing the partials in the last block to finish, behind a __threadfence() + counter, was measured: the agent-scope
    //  fence of 256 blocks costs ~100 us per launch on this machine — 8.7 -> 12.3 ms per step; the second launch stays)
    // grouped mode: the partial image of every norm goes to a slice of its own and ONE launch sums them all after the backward
    // pass (flush_norms); otherwise the column sum follows right away
    const int slot = group ? norm_slot_base + (int)norm_offs.size() : 0;
    float* part = t->dw_part + (int64_t)slot * RN_BLOCKS * d;
    T* out_t = nullptr;
    const bool emits = group && after_site != -2;
    if (emits) {
      out_t = (T*)t->ring[m2m_trainer::K_DXT][pos[m2m_trainer::K_DXT] % t->ring[m2m_trainer::K_DXT].size()];      // what the next begin_sub() selects
      pre.src = dx_out; pre.dst = out_t; pre.site = after_site;
    }
    const Drop after = drop(emits ? after_site : -1), din = drop(dy_site);
    hipLaunchKernelGGL(rmsnorm_bwd_kernel<T>, dim3(RN_BLOCKS), dim3(256), (size_t)4 * d * sizeof(float), st, x, P + w_off, dy, dx_res, dx_out,
                       part, M, d, t->g.layer_norm_eps, out_t, after.key, after.thresh, after.scale, din.key, din.thresh);
    if (group) norm_offs.push_back(w_off);
    else hipLaunchKernelGGL(colsum_kernel, dim3(ceil_div(d, 32)), dim3(256), 0, st, part, G + w_off, RN_BLOCKS, d, gacc);
    M2M_CHECK_HIP(hipGetLastError());
    return M2M_OK;
  }
  // Whole-head attention kernels (attn_train.hip): bf16 storage, both lengths within an LDS image.  M2M_TRAIN_ATTN=stripes keeps round 2's path.
  bool head_ok(int Sq, int Sk) const { return sizeof(T) == 2 && t->sw.attn_head && t->sw.tuned_gemm && Sq <= AH_MAX_S && Sk <= AH_MAX_S; }
  HeadAttnArgs head_args(const AttnDesc& d, bool bwd) const {
    HeadAttnArgs a{};
    const int Sq = d.Sq, Sk = d.Sk;
    a.Q = (const bf16_t*)d.q.p; a.K = (const bf16_t*)d.k.p; a.V = (const bf16_t*)d.v.p; a.ldq = d.q.ld; a.ldk = d.k.ld; a.ldv = d.v.ld;
    a.sQb = d.q.sb; a.sKb = d.k.sb; a.sVb = d.v.sb;
    a.O = (bf16_t*)d.ao; a.ldo = t->inner; a.sOb = (int64_t)Sq * t->inner; a.lse = d.lse;
    a.bias_tab = d.tab; a.tab_stride = Sq + Sk - 1; a.tab_center = Sq - 1;
    a.H = t->g.num_heads; a.Sq = Sq; a.Sk = Sk; a.causal = d.causal; a.ldp = (int)align_up(Sk, 8);
    const Drop dr = drop(d.site);
    a.dk = dr.key; a.thresh = dr.thresh; a.scale = dr.scale;
    a.keep_bits = (uint32_t*)d.Pm;           // (the layer's probability buffer, unused on this path: B*H*Sq*Sk/8 bytes of its B*H*Sq*ldp*2)
    if (bwd) {
      a.dO = (const bf16_t*)d.dO; a.dQ = (bf16_t*)d.dq.p; a.dK = (bf16_t*)d.dk.p; a.dV = (bf16_t*)d.dv.p;
      a.lddq = d.dq.ld; a.lddk = d.dk.ld; a.lddv = d.dv.ld; a.sdQb = d.dq.sb; a.sdKb = d.dk.sb; a.sdVb = d.dv.sb;
      a.diag_part = d.buckets ? drel_slot() : nullptr;
    }
    return a;
  }
  // Fused scores + softmax (attn_stripe_kernel) when a wave can hold all keys; K = (key, d) operand, Q = (query, d) operand.
  bool stripe_ok(int Sk) const { return t->sw.stripes && Sk <= 32 * ST_NT; }      // (the LDS bound: at ST_NT)
  // K | V of a layer (V `inner` columns behind K) -> kt [2][nB*H][64][Sp]
  int kv_transpose(const Mat& k, void* kt, int nB, int S) const {
    const int H = t->g.num_heads, Sp = (int)align_up(S, 32);
    constexpr int Et = 16 / sizeof(T);
    hipLaunchKernelGGL(kv_transpose_kernel<T>, dim3(ceil_div((Sp / Et) * (DK / Et), 256), nB * H, 2), dim3(256), 0, st, (const T*)k.p, k.ld, (int64_t)t->inner, (T*)kt, S, Sp,
                       H, (int64_t)nB * H * DK * Sp);
    M2M_CHECK_HIP(hipGetLastError());
    return M2M_OK;
  }
  // what the two stripe launches of a layer share: X = (key, d) operand, Y = (query, d) operand, the probabilities, the dropout key, and the
  // fused product of the rows a workgroup has just formed: Xt its transposed second operand, `out` its result
  StripeArgs stripe_args(const AttnDesc& d, const Mat& X, const Mat& Y, const T* Xt, const Mat& out) const {
    const Drop dr = drop(d.site);
    StripeArgs a{};
    a.X = X.p; a.ldx = X.ld; a.sX1 = X.sb; a.sX2 = X.sh; a.Y = Y.p; a.ldy = Y.ld; a.sY1 = Y.sb; a.sY2 = Y.sh;
    a.P = d.Pm; a.H = t->g.num_heads; a.Sq = d.Sq; a.Sk = d.Sk; a.ldp = (int)align_up(d.Sk, 8); a.causal = d.causal;
    a.dk = dr.key; a.thresh = dr.thresh; a.scale = dr.scale;
    a.Xt = Xt; a.xt_ld = align_up(d.Sk, 32); a.O = const_cast<void*>(out.p); a.ldo = out.ld; a.sO1 = out.sb; a.sO2 = out.sh;
    return a;
  }
  // Fused scores + softmax (K, Q) -> P, and O = P~ . V into ao against the transposed V (the dropped P~ never leaves the kernel)
  int attn_probs(const AttnDesc& d, int nB, const T* vt) const {
    StripeArgs a = stripe_args(d, d.k, d.q, vt, part(d.ao, 1, 0, d.Sq));
    a.bias_tab = d.tab; a.tab_stride = d.Sq + d.Sk - 1; a.tab_center = d.Sq - 1;
    return launch_attn_stripe<T>(false, a, nB, st, t->sw);
  }
  // Fused dP + softmax backward (V, dO) -> dS (t->dS), dQ = dS . K against the transposed K, the diagonal sums of the bias gradient
  // and, with dropout, the dropped probabilities again into the fp32 score scratch (t->sc, unused on this tier: they survive dS, so
  // dV shares a launch with dK).  (causal only lets the kernel skip key tiles above the diagonal: P is zero there anyway)
  int dscores(const AttnDesc& d, int nB, const T* kt) const {
    StripeArgs a = stripe_args(d, d.v, part(d.dO, 1, 0, d.Sq), kt, d.dq);
    a.Pd = dropping(d.site) ? t->sc : nullptr;
    a.dS = t->dS;
    a.diag_part = d.buckets ? drel_slot() : nullptr;
    return launch_attn_stripe<T>(true, a, nB, st, t->sw);
  }
  // P (kept for the backward) and, with dropout, the dropped copy the P.V product reads (scratch: t->dS); returns it through *Puse
  int softmax(const AttnDesc& d, int nB, const T** Puse) const {
    const int H = t->g.num_heads, Sq = d.Sq, Sk = d.Sk, rows = nB * H * Sq;
    const Drop dr = drop(d.site);
    T* const Pd = dr.thresh ? (T*)t->dS : (T*)nullptr;
    hipLaunchKernelGGL(softmax_fwd_kernel<T>, dim3(ceil_div(rows, 4)), dim3(256), 0, st, t->sc, (T*)d.Pm, rows, H, Sq, Sk, (int)align_up(Sk, 8), d.tab, Sq + Sk - 1,
                       Sq - 1, d.causal, Pd, dr.key, dr.thresh, dr.scale);
    M2M_CHECK_HIP(hipGetLastError());
    *Puse = Pd ? Pd : (const T*)d.Pm;
    return M2M_OK;
  }
  // backward: the dropped probabilities again (into t->dS, consumed by the dV product before dS overwrites it)
  int redrop(const void* Pm, int64_t n, int site, const T** Puse) const {
    if (!dropping(site)) { *Puse = (const T*)Pm; return M2M_OK; }
    hipLaunchKernelGGL(drop_copy_kernel<T>, dim3(grid_1d(n)), dim3(256), 0, st, (const T*)Pm, (T*)t->dS, n, key(site), t->drop_thresh, t->drop_scale);
    M2M_CHECK_HIP(hipGetLastError());
    *Puse = (const T*)t->dS;
    return M2M_OK;
  }
  int softmax_bwd(const AttnDesc& d, int nB) const {      // dS (t->dS) from P and dPd (t->sc)
    const Drop dr = drop(d.site);
    hipLaunchKernelGGL(softmax_bwd_kernel<T>, dim3(ceil_div(nB * t->g.num_heads * d.Sq, 4)), dim3(256), 0, st, (const T*)d.Pm, t->sc, (T*)t->dS,
                       nB * t->g.num_heads * d.Sq, d.Sk, (int)align_up(d.Sk, 8), dr.key, dr.thresh, dr.scale);
    M2M_CHECK_HIP(hipGetLastError());
    return M2M_OK;
  }
  int gated(const void* ab, void* mid, int64_t M, int site) const {
    const Drop dr = drop(site);
    hipLaunchKernelGGL(gated_fwd_kernel<T>, dim3(grid_1d(M * t->g.d_ff / 4)), dim3(256), 0, st, (const T*)ab, (T*)mid, M, t->g.d_ff, dr.key, dr.thresh, dr.scale);
    M2M_CHECK_HIP(hipGetLastError());
    return M2M_OK;
  }
  int gated_bwd(const void* ab, const void* dmid, void* dab, int64_t M, int site) const {
    const Drop dr = drop(site);
    hipLaunchKernelGGL(gated_bwd_kernel<T>, dim3(grid_1d(M * t->g.d_ff / 4)), dim3(256), 0, st, (const T*)ab, (const T*)dmid, (T*)dab, M, t->g.d_ff,
                       dr.key, dr.thresh, dr.scale);
    M2M_CHECK_HIP(hipGetLastError());
    return M2M_OK;
  }
  // bias gradient from the per-stripe diagonal sums the backward stripe kernel left in t->drel
  float* drel_slot() const { return t->drel + (int64_t)(group ? drel_slots : 0) * t->drel_slot_floats; }      // where the next stripe launch leaves its sums
  int bias_reduce(const BiasJob& j, int accumulate) const {
    const int H = t->g.num_heads, nrel = j.Sq + j.Sk - 1, stripes = ceil_div(j.Sq, 32);
    float* tmp = t->drel + (int64_t)(t->g.num_layers + t->g.num_decoder_layers) * t->drel_slot_floats;
    hipLaunchKernelGGL(bias_stripes_sum_kernel, dim3(H, ceil_div(nrel, 64), j.layers), dim3(1024), 0, st, t->drel + (int64_t)j.first_slot * t->drel_slot_floats,
                       tmp, j.nB, H, stripes, j.Sq, j.Sk, t->drel_slot_floats);
    hipLaunchKernelGGL(bias_bucket_kernel, dim3(t->g.num_buckets * H), dim3(256), 0, st, tmp, j.buckets, j.Gtab, j.layers, H, nrel, accumulate | gacc);
    M2M_CHECK_HIP(hipGetLastError());
    return M2M_OK;
  }
  // grouped mode: the layers of a stack share one table, so their sums are reduced together after the backward pass (two
  // launches per stack instead of two per layer); otherwise right away
  int bias_grad_stripes(const int* buckets, float* Gtab, int nB, int Sq, int Sk, int accumulate) const {
    if (!group) return bias_reduce(BiasJob{buckets, Gtab, nB, Sq, Sk, 0, 1}, accumulate);
    if (!bias_jobs.empty() && bias_jobs.back().buckets == buckets && bias_jobs.back().Gtab == Gtab) bias_jobs.back().layers += 1;
    else bias_jobs.push_back(BiasJob{buckets, Gtab, nB, Sq, Sk, drel_slots, 1});
    drel_slots += 1;
    return M2M_OK;
  }
  int flush_bias() const {
    for (const BiasJob& j : bias_jobs) { const int rc = bias_reduce(j, 0); if (rc != M2M_OK) return rc; }
    bias_jobs.clear();
    return M2M_OK;
  }
  int bias_grad(const void* dS, const int* buckets, float* Gtab, int nB, int Sq, int Sk, int ldp, int accumulate) const {
    const int H = t->g.num_heads, nrel = Sq + Sk - 1;
    // scratch of its own, behind the stripe kernels' slots and their reduction scratch: those may hold other layers' sums
    // that wait for the end of the pass (a model whose encoder is past the stripe kernels' reach and whose decoder is not)
    float* part = t->drel + (int64_t)(t->g.num_layers + t->g.num_decoder_layers) * t->drel_slot_floats +
                  (int64_t)std::max(t->g.num_layers, t->g.num_decoder_layers) * H * 2 * std::max(t->max_enc, t->max_dec);
    hipLaunchKernelGGL(bias_diag_kernel<T>, dim3(nB * H, ceil_div(nrel, 64)), dim3(256), 0, st, (const T*)dS, part, H, Sq, Sk, ldp);
    hipLaunchKernelGGL(bias_bucket_kernel, dim3(t->g.num_buckets * H), dim3(256), 0, st, part, buckets, Gtab, nB, H, nrel, accumulate | gacc);
    M2M_CHECK_HIP(hipGetLastError());
    return M2M_OK;
  }
};

#define RC(expr) do { if ((rc = (expr)) != M2M_OK) return rc; } while (0)

// dropout sites (hf: modeling_t5.py — T5Stack dropout on the embeddings and after the final norm, T5Attention on the
// probabilities, T5LayerSelfAttention / CrossAttention / FF on the branch output, T5DenseGatedActDense before wo).
// site = stack base + 16 * layer + place; oracle/train.py uses the same numbering.
enum { SITE_ENC = 0, SITE_DEC = 1000, SITE_EMB = 900, SITE_FIN = 901,
       PL_PROBS_SELF = 1, PL_SELF_OUT = 2, PL_PROBS_CROSS = 3, PL_CROSS_OUT = 4, PL_MID = 5, PL_FF_OUT = 6 };

// The attention of one layer between its projections, self or cross: q / k / v -> ao.  The ONE place that chooses among the
// whole-head kernels (attn_train.hip), the fused stripe kernels and the unfused product + softmax path past 512 keys: three
// straight-line bodies per direction, the same choice in both.
template <typename T>
int attn_core_fwd(const Ops<T>& o, const AttnDesc& a, int nB) {
  m2m_trainer* t = o.t;
  const int Sq = a.Sq, Sk = a.Sk;
  int rc;
  if (o.head_ok(Sq, Sk))                                            // whole-head kernel: no P, no K^T | V^T, only O and the row log-sum-exp
    return launch_attn_head_fwd(o.head_args(a, false), nB, o.st, t->sw);
  if (o.stripe_ok(Sk)) {                                            // stripe kernel: P, and O = P~ . V against the transposed V
    // (K^T | V^T from the projection's own epilogue was built twice in round 3 — the tile staged through LDS, then the transpose taken
    //  from the matrix core with the operands swapped — and both cost the projection as much as this launch takes: 64-byte row
    //  pieces instead of whole lines; removed again)
    RC(o.kv_transpose(a.k, a.kt, nB, Sk));                          // (its K^T half serves dQ = dS . K in the backward pass)
    return o.attn_probs(a, nB, (const T*)a.kt + (int64_t)nB * t->g.num_heads * DK * align_up(Sk, 32));
  }
  const T* Pu;                                                      // unfused: scores -> softmax (+ the dropped copy) -> P~ . V
  RC(o.mmbh(TG_STORE_F32, {a.q, a.k, o.pmat(t->sc, Sq, Sk)}, nB, Sq, Sk, DK));
  RC(o.softmax(a, nB, &Pu));
  RC(o.mmbh(TG_STORE_T, {o.pmat(Pu, Sq, Sk), a.v.t(), o.part(a.ao, 1, 0, Sq)}, nB, Sq, DK, Sk));
  return M2M_OK;
}

// ... and backward: a.dO -> a.dq | a.dk | a.dv, and the bias gradient where the layer has one
template <typename T>
int attn_core_bwd(const Ops<T>& o, const AttnDesc& a, int nB) {
  m2m_trainer* t = o.t;
  const int Sq = a.Sq, Sk = a.Sk;
  int rc;
  if (o.head_ok(Sq, Sk)) {                                          // whole-head kernel: dQ | dK | dV (and the bias gradient's diagonal sums) in one launch
    RC(launch_attn_head_bwd(o.head_args(a, true), nB, o.st, t->sw));
    if (a.buckets) RC(o.bias_grad_stripes(a.buckets, a.Gbias, nB, Sq, Sk, a.bias_accumulate));
    return M2M_OK;
  }
  const Mat dO = o.part(a.dO, 1, 0, Sq), dS = o.pmat(t->dS, Sq, Sk);
  if (o.stripe_ok(Sk)) {                                            // stripe kernel: dS, dQ, the dropped P again; then dV | dK as one launch
    RC(o.dscores(a, nB, (const T*)a.kt));
    if (a.buckets) RC(o.bias_grad_stripes(a.buckets, a.Gbias, nB, Sq, Sk, a.bias_accumulate));
    const Mat Pd = o.pmat(o.dropping(a.site) ? (const void*)t->sc : a.Pm, Sq, Sk);
    RC(o.mmbh2(TG_STORE_T, {Pd.t(), dO.t(), a.dv}, {dS.t(), a.q.t(), a.dk}, nB, Sk, DK, Sq));      // dV = Pd^T dO | dK = dS^T Q
    return M2M_OK;
  }
  const T* Pu;                                                      // unfused: every product and row kernel a launch of its own
  RC(o.redrop(a.Pm, nB * dS.sb, a.site, &Pu));
  RC(o.mmbh(TG_STORE_T, {o.pmat(Pu, Sq, Sk).t(), dO.t(), a.dv}, nB, Sk, DK, Sq));                 // dV = Pd^T dO (before dS overwrites Pd)
  RC(o.mmbh(TG_STORE_F32, {dO, a.v, o.pmat(t->sc, Sq, Sk)}, nB, Sq, Sk, DK));                     // dPd = dO V^T
  RC(o.softmax_bwd(a, nB));
  if (a.buckets) RC(o.bias_grad(t->dS, a.buckets, a.Gbias, nB, Sq, Sk, (int)dS.ld, a.bias_accumulate));
  RC(o.mmbh(TG_STORE_T, {dS, a.k.t(), a.dq}, nB, Sq, DK, Sk));                                    // dQ = dS K
  RC(o.mmbh(TG_STORE_T, {dS.t(), a.q.t(), a.dk}, nB, Sk, DK, Sq));                                // dK = dS^T Q
  return M2M_OK;
}

// What the layers of one stack share in a pass (forward_backward_t builds one per stack).  The backward pass walks a stack from its
// LAST layer down: that layer starts the sums the layers of a stack share (the bias table's gradient, dhE), the others add to them.
struct Stack {
  int S, Sx;               // rows per clip; Sx: of the encoder output the decoder's cross-attention reads
  int layers;
  const float* tab;        // self-attention: the relative-position bias table [H][2 S - 1], ...
  const int* buckets;      // ... its bucket table, and where the bias weights sit in the flat buffers
  int64_t bias_off;
  int causal;
  int site0;               // SITE_ENC / SITE_DEC
  int site(int l) const { return site0 + 16 * l; }
  bool last(int l) const { return l == layers - 1; }
};

// the descriptor of a self-attention layer: q | k | v from the layer's one projection, dq | dk | dv into its gradient (t->dqkv)
template <typename T>
AttnDesc self_desc(const Ops<T>& o, const SelfAttn& w, const Stack& s, int l) {
  AttnDesc a{};
  a.q = o.part(w.qkv_out, 3, 0, s.S); a.k = o.part(w.qkv_out, 3, 1, s.S); a.v = o.part(w.qkv_out, 3, 2, s.S);
  a.dq = o.part(o.t->dqkv, 3, 0, s.S); a.dk = o.part(o.t->dqkv, 3, 1, s.S); a.dv = o.part(o.t->dqkv, 3, 2, s.S);
  a.Sq = a.Sk = s.S; a.tab = s.tab; a.causal = s.causal; a.site = s.site(l) + PL_PROBS_SELF;
  a.Pm = w.P; a.kt = w.kt; a.lse = w.lse; a.ao = w.ao;
  return a;
}

// self-attention block of layer l, forward: x_in -> x_out = x_in + Attn(norm(x_in))
template <typename T>
int attn_self_fwd(const Ops<T>& o, const SelfAttn& w, const Stack& s, int l, int nB, const float* x_in, float* x_out) {
  m2m_trainer* t = o.t;
  const int d = t->g.d_model, inner = t->inner, M = nB * s.S;
  int rc;
  RC(o.norm(x_in, w.ln, w.h, M));
  RC(o.mm(TG_STORE_T, w.h, d, 0, o.W(w.qkv), d, 0, w.qkv_out, 3 * inner, M, 3 * inner, d));
  RC(attn_core_fwd<T>(o, self_desc<T>(o, w, s, l), nB));
  RC(o.mm_resid(w.ao, w.o, x_out, M, d, inner, x_in, s.site(l) + PL_SELF_OUT));
  return M2M_OK;
}

// ... and backward: dx_out (fp32, gradient wrt x_out) -> dx_in; weight gradients into G
template <typename T>
int attn_self_bwd(const Ops<T>& o, const SelfAttn& w, const Stack& s, int l, int nB, const float* x_in, const float* dx_out, float* dx_in, float* G) {
  m2m_trainer* t = o.t;
  const int d = t->g.d_model, inner = t->inner, M = nB * s.S;
  int rc;
  RC(o.begin_sub(1u << m2m_trainer::K_DXT | 1u << m2m_trainer::K_DQKV));
  RC(o.cvt_branch(dx_out, t->dxT, (int64_t)M * d, s.site(l) + PL_SELF_OUT));
  RC(o.dW(t->dxT, d, d, w.ao, inner, inner, G + w.o, M));                                         // dWo = dx^T . ao
  RC(o.dX(TG_STORE_T, t->dxT, d, w.o, d, inner, t->dO, inner, M));                                // dO = dx . Wo
  AttnDesc a = self_desc<T>(o, w, s, l);
  a.dO = t->dO; a.buckets = s.buckets; a.Gbias = G + s.bias_off; a.bias_accumulate = s.last(l) ? 0 : 1;
  RC(attn_core_bwd<T>(o, a, nB));
  RC(o.dW(t->dqkv, 3 * inner, 3 * inner, w.h, d, d, G + w.qkv, M));                               // dWqkv = dqkv^T . h
  RC(o.dX(TG_STORE_F32, t->dqkv, 3 * inner, w.qkv, 3 * inner, d, t->dh, d, M));                   // dh = dqkv . Wqkv
  RC(o.norm_bwd(x_in, w.ln, t->dh, dx_out, dx_in, G, M));
  RC(o.end_sub());
  return M2M_OK;
}

// the descriptor of decoder layer l's cross-attention (hf: modeling_t5.py:319-342: K/V from the encoder output, zero bias, no mask)
template <typename T>
AttnDesc cross_desc(const Ops<T>& o, const CrossAttn& w, const Stack& s, int l) {
  m2m_trainer* t = o.t;
  AttnDesc a{};
  a.q = o.part(w.q_out, 1, 0, s.S); a.k = o.part(w.kv_out, 2, 0, s.Sx); a.v = o.part(w.kv_out, 2, 1, s.Sx);
  a.dq = o.part(t->dcq, 1, 0, s.S); a.dk = o.part(t->dckv, 2, 0, s.Sx); a.dv = o.part(t->dckv, 2, 1, s.Sx);
  a.Sq = s.S; a.Sk = s.Sx; a.site = s.site(l) + PL_PROBS_CROSS;
  a.Pm = w.P; a.kt = w.kt; a.lse = w.lse; a.ao = w.ao;
  return a;
}

// cross-attention block of decoder layer l, forward: x_in -> x_out = x_in + Attn(norm(x_in), hE)
template <typename T>
int attn_cross_fwd(const Ops<T>& o, const CrossAttn& w, const Stack& s, int l, int nB, const float* x_in, float* x_out) {
  m2m_trainer* t = o.t;
  const int d = t->g.d_model, inner = t->inner, Md = nB * s.S, Me = nB * s.Sx;
  int rc;
  RC(o.norm(x_in, w.ln, w.h, Md));
  RC(o.mm(TG_STORE_T, w.h, d, 0, o.W(w.q), d, 0, w.q_out, inner, Md, inner, d));
  RC(o.mm(TG_STORE_T, t->hE, d, 0, o.W(w.kv), d, 0, w.kv_out, 2 * inner, Me, 2 * inner, d));
  RC(attn_core_fwd<T>(o, cross_desc<T>(o, w, s, l), nB));
  RC(o.mm_resid(w.ao, w.o, x_out, Md, d, inner, x_in, s.site(l) + PL_CROSS_OUT));
  return M2M_OK;
}

// ... and backward: dx_out -> dx_in, and the layer's share of the encoder output's gradient into t->dhE
template <typename T>
int attn_cross_bwd(const Ops<T>& o, const CrossAttn& w, const Stack& s, int l, int nB, const float* x_in, const float* dx_out, float* dx_in, float* G) {
  m2m_trainer* t = o.t;
  const int d = t->g.d_model, inner = t->inner, Md = nB * s.S, Me = nB * s.Sx;
  int rc;
  RC(o.begin_sub(1u << m2m_trainer::K_DXT | 1u << m2m_trainer::K_DCQ | 1u << m2m_trainer::K_DCKV));
  RC(o.cvt_branch(dx_out, t->dxT, (int64_t)Md * d, s.site(l) + PL_CROSS_OUT));
  RC(o.dW(t->dxT, d, d, w.ao, inner, inner, G + w.o, Md));
  RC(o.dX(TG_STORE_T, t->dxT, d, w.o, d, inner, t->dO, inner, Md));
  AttnDesc a = cross_desc<T>(o, w, s, l);
  a.dO = t->dO;
  RC(attn_core_bwd<T>(o, a, nB));
  RC(o.dW(t->dcq, inner, inner, w.h, d, d, G + w.q, Md));
  RC(o.dX(TG_STORE_F32, t->dcq, inner, w.q, inner, d, t->dh, d, Md));
  RC(o.norm_bwd(x_in, w.ln, t->dh, dx_out, dx_in, G, Md));
  RC(o.dW(t->dckv, 2 * inner, 2 * inner, t->hE, d, d, G + w.kv, Me));                             // dWckv = dckv^T . hE
  RC(o.dX(s.last(l) ? TG_STORE_F32 : TG_ACC_F32, t->dckv, 2 * inner, w.kv, 2 * inner, d, t->dhE, d, Me));      // dhE (+)= dckv . Wckv
  RC(o.end_sub());
  return M2M_OK;
}

template <typename T>
int ff_fwd(const Ops<T>& o, const FeedFwd& w, const Stack& s, int l, int nB, const float* x_in, float* x_out) {
  m2m_trainer* t = o.t;
  const int d = t->g.d_model, dff = t->g.d_ff, M = nB * s.S;
  int rc;
  RC(o.norm(x_in, w.ln, w.h, M));
  // the gate product with the activation in its epilogue (bf16, grids the 128x128 tile takes anyway): a | b and
  // mid = dropout(gelu_new(a) * b) leave the product together — the gated_fwd_kernel launch and its read of the pair are gone
  if (t->sw.gate_epi && !t->fp8 && t->sw.tuned_gemm && t->Wil && gemm_takes_gated_train(t->precision, M, 2 * dff, d)) {
    GemmArgs a{};
    a.A = w.h; a.W = reinterpret_cast<const T*>(t->Wil) + w.wi; a.M = M; a.N = 2 * dff; a.K = d; a.out = w.mid; a.ldo = dff; a.ab_out = w.ab; a.vt_which = -1;
    o.drop_fields(a, s.site(l) + PL_MID);
    RC(launch_gemm(t->precision, EPI_GATED_TRAIN, a, o.st));
  } else {
    RC(o.mm(TG_STORE_T, w.h, d, 0, o.W(w.wi), d, 0, w.ab, 2 * dff, M, 2 * dff, d));
    RC(o.gated(w.ab, w.mid, M, s.site(l) + PL_MID));
  }
  RC(o.mm_resid(w.mid, w.wo, x_out, M, d, dff, x_in, s.site(l) + PL_FF_OUT));
  return M2M_OK;
}
template <typename T>
int ff_bwd(const Ops<T>& o, const FeedFwd& w, const Stack& s, int l, int nB, const float* x_in, const float* dx_out, float* dx_in, float* G) {
  m2m_trainer* t = o.t;
  const int d = t->g.d_model, dff = t->g.d_ff, M = nB * s.S;
  int rc;
  RC(o.begin_sub(1u << m2m_trainer::K_DXT | 1u << m2m_trainer::K_DAB));
  RC(o.cvt_branch(dx_out, t->dxT, (int64_t)M * d, s.site(l) + PL_FF_OUT));
  RC(o.dW(t->dxT, d, d, w.mid, dff, dff, G + w.wo, M));                                           // dWo = dx^T . mid
  // dmid = dx . Wo, turned into the gate pair's gradient by the product's own epilogue where it can (bf16): dmid is never stored,
  // the gated_bwd_kernel launch and its reads are gone
  if (t->sw.gate_epi && !t->fp8 && t->sw.tuned_gemm && gemm_takes_gated_bwd(t->precision, M, dff, d)) {
    GemmArgs a{};
    a.A = t->dxT; a.W = reinterpret_cast<const T*>(t->WT) + w.wo; a.M = M; a.N = dff; a.K = d; a.out = t->dab; a.ldo = 2 * dff; a.ab_out = w.ab;
    a.vt_which = -1;
    o.drop_fields(a, s.site(l) + PL_MID);
    RC(launch_gemm(t->precision, EPI_GATED_BWD, a, o.st));
  } else {
    RC(o.dX(TG_STORE_T, t->dxT, d, w.wo, d, dff, t->dmid, dff, M));                               // dmid = dx . Wo
    RC(o.gated_bwd(w.ab, t->dmid, t->dab, M, s.site(l) + PL_MID));
  }
  RC(o.dW(t->dab, 2 * dff, 2 * dff, w.h, d, d, G + w.wi, M));                                     // dWi = dab^T . h
  RC(o.dX(TG_STORE_F32, t->dab, 2 * dff, w.wi, 2 * dff, d, t->dh, d, M));                         // dh = dab . Wi
  RC(o.norm_bwd(x_in, w.ln, t->dh, dx_out, dx_in, G, M));
  RC(o.end_sub());
  return M2M_OK;
}

// Everything a pass needs before its first product and that depends on nothing but the inputs, in ONE launch.  (The pad ranges: the
// flat gradient buffer is OVERWRITTEN by every pass — each tensor in full, by its own product / reduction — so all that needs zeroing
// is the alignment padding between tensors, <= 63 floats each, instead of a 121 MB memset; tests fill the buffer with NaN before a
// pass, so a tensor nobody wrote would show.  An accumulating pass — m2m_train_forward_backward_acc — ADDS every tensor instead; the
// pads, which belong to no tensor, are zeroed all the same.)  In ONE launch (they were six:
// two bias-table gathers, the dropout key, the pad zeroing, the valid-label count, the decoder inputs — ~5 us of launch each for
// microseconds of work).  Block roles by index: [0, nb_e) encoder bias table, [nb_e, nb_e + nb_d) decoder bias table, then the pad
// ranges (one wave each), then shift_right; block 0 also advances the dropout key (thread 0) and, the LAST block counts
// the scored labels (a single-block reduction).
struct PrologueArgs {
  const float *w_e, *w_d;              // relative-position-bias weights [buckets][H]
  const int *bucket_e, *bucket_d;
  float *tab_e, *tab_d;
  int H, nrel_e, nrel_d, nb_e, nb_d;
  uint64_t seed;
  uint64_t *ctr, *key;
  const int64_t* pads;
  int n_pads, nb_p;
  float* G;                            // null: forward only (no pads)
  const int64_t* labels;
  int64_t* dec_in;
  int B, L, start_id, pad_id, nb_s;
  float* inv_n;
  int scaled;                          // accumulate-mode passes: inv_n[2] = inv_n[0] * (gscale_dev ? *gscale_dev : gscale), the dlogits factor
  const float* gscale_dev;
  float gscale;
};
__global__ __launch_bounds__(256) void train_prologue_kernel(PrologueArgs a) {
  int blk = blockIdx.x;
  if (blk == 0 && threadIdx.x == 0) {                      // key of this pass = splitmix64(seed + passes since set_dropout); the counter lives on the device so that a replayed graph advances it
    const uint64_t c = *a.ctr;
    *a.key = splitmix64(a.seed + c);
    *a.ctr = c + 1;
  }
  if (blk < a.nb_e + a.nb_d) {                             // bias tables from the CURRENT (trainable) bucket weights
    const bool dec = blk >= a.nb_e;
    const int idx = (dec ? blk - a.nb_e : blk) * 256 + threadIdx.x, nrel = dec ? a.nrel_d : a.nrel_e;
    if (idx < a.H * nrel) {
      const int hh = idx / nrel, i = idx - hh * nrel;
      (dec ? a.tab_d : a.tab_e)[idx] = (dec ? a.w_d : a.w_e)[(int64_t)(dec ? a.bucket_d : a.bucket_e)[i] * a.H + hh];
    }
    return;
  }
  blk -= a.nb_e + a.nb_d;
  if (blk < a.nb_p) {                                      // alignment padding of the flat gradient buffer
    const int i = blk * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i < a.n_pads) {
      const int64_t off = a.pads[2 * i], cnt = a.pads[2 * i + 1];
      for (int64_t j = lane; j < cnt; j += 64) a.G[off + j] = 0.f;
    }
    return;
  }
  blk -= a.nb_p;
  if (blk < a.nb_s) {                                      // decoder inputs = shift_right(labels)
    const int i = blk * 256 + threadIdx.x;
    if (i < a.B * a.L) {
      const int tpos = i % a.L;
      int64_t v = tpos == 0 ? a.start_id : a.labels[i - 1];
      if (v == -100) v = a.pad_id;
      a.dec_in[i] = v;
    }
    return;
  }
  // last block: number of scored labels
  __shared__ int cnt[256];
  int c = 0;
  const int n = a.B * a.L;
  for (int i = threadIdx.x; i < n; i += 256) c += a.labels[i] != -100;
  cnt[threadIdx.x] = c;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (threadIdx.x < st) cnt[threadIdx.x] += cnt[threadIdx.x + st];
    __syncthreads();
  }
  // no label to score: the mean over zero rows is NaN, as torch's CrossEntropyLoss gives (its gradient is zero there too)
  if (threadIdx.x == 0) {
    a.inv_n[0] = cnt[0] > 0 ? 1.0f / (float)cnt[0] : __builtin_nanf(""); a.inv_n[1] = (float)cnt[0];
    if (a.scaled) a.inv_n[2] = a.inv_n[0] * (a.gscale_dev ? *a.gscale_dev : a.gscale);
  }
}

template <typename T>
int forward_backward_t(m2m_trainer* t, const float* P, const float* enc_inputs, const int64_t* cond_idx, const int64_t* labels, int B, int S,
                       int L, float* loss_out, float* G, float* logits_out, hipStream_t st, hipStream_t st_side,
                       const std::function<int()>* at_split = nullptr) {
  const m2m_t5_geometry& g = t->g;
  const int d = g.d_model, V = g.vocab_size, H = g.num_heads, Le = g.num_layers, Ld = g.num_decoder_layers;
  const int Me = B * S, Md = B * L, ldv = (int)align_up(V, 8);
  Ops<T> o{t, st, P};
  o.Gbase = G;
  o.gacc = G && (t->gmode & m2m_trainer::GM_ACC) ? 1 : 0;
  const bool scaled = G && (t->gmode & m2m_trainer::GM_SCALED);
  o.group = G && t->sw.dw_group && !(t->fp8 && t->sw.fp8.dw);
  o.st2 = (G && !o.group) ? st_side : nullptr;
  const Stack enc{S, 0, Le, t->etab, t->ebucket, t->o_erb, 0, SITE_ENC}, dec{L, S, Ld, t->dtab, t->dbucket, t->o_drb, 1, SITE_DEC};
  int rc;
  // (the bucket tables of this geometry are on the device already: ensure_tables())
  {
    PrologueArgs a{};
    a.w_e = P + t->o_erb; a.w_d = P + t->o_drb; a.bucket_e = t->ebucket; a.bucket_d = t->dbucket; a.tab_e = t->etab; a.tab_d = t->dtab;
    a.H = H; a.nrel_e = 2 * S - 1; a.nrel_d = 2 * L - 1; a.nb_e = ceil_div(H * a.nrel_e, 256); a.nb_d = ceil_div(H * a.nrel_d, 256);
    a.seed = t->drop_seed; a.ctr = t->step_ctr_dev; a.key = t->step_key_dev;
    a.pads = t->pads_dev; a.n_pads = G ? t->n_pads : 0; a.nb_p = ceil_div(a.n_pads, 4); a.G = G;
    a.labels = labels; a.dec_in = t->dec_in; a.B = B; a.L = L; a.start_id = g.decoder_start_token_id; a.pad_id = g.pad_token_id;
    a.nb_s = ceil_div(Md, 256); a.inv_n = t->inv_n;
    a.scaled = scaled ? 1 : 0; a.gscale_dev = t->gscale_src; a.gscale = t->gscale;
    hipLaunchKernelGGL(train_prologue_kernel, dim3(a.nb_e + a.nb_d + a.nb_p + a.nb_s + 1), dim3(256), 0, st, a);
    M2M_CHECK_HIP(hipGetLastError());
  }
  if (G || t->precision == M2M_PREC_BF16) {      // W^T for the dX products (with gradients) and the bf16 copy the forward products read, one pass over P
    const bool bf16 = t->precision == M2M_PREC_BF16;
    RC(launch_weights_transpose(t->precision, (const WtBlock*)t->wt_blocks, t->n_wt_blocks, P, G ? t->WT : nullptr, bf16 ? t->Wc : nullptr,
                                bf16 && !t->fp8 ? t->Wil : nullptr, st));
  }
  if (t->fp8) {
    const int rc = launch_mxq_weights((const W8Tile*)t->w8_tiles, t->n_w8_tiles, P, t->w8, st);
    if (rc != M2M_OK) return rc;
  }

  // ================= forward =================
  if (enc_inputs != t->xe[0]) M2M_CHECK_HIP(hipMemcpyAsync(t->xe[0], enc_inputs, (size_t)Me * d * 4, hipMemcpyDeviceToDevice, st));
  if (o.dropping(SITE_ENC + SITE_EMB)) {     // conditioning rows + the dropout on the embeddings, one launch
    hipLaunchKernelGGL(enc_input_kernel, dim3(grid_1d((int64_t)Me * d / 4)), dim3(256), 0, st, P, t->cond_off_dev, t->cond_rows_dev, t->n_cond, cond_idx,
                       t->xe[0], B, S, d, o.key(SITE_ENC + SITE_EMB), t->drop_thresh, t->drop_scale);
  } else if (t->n_cond > 0) {
    hipLaunchKernelGGL(cond_gather_kernel, dim3(B * t->n_cond), dim3(128), 0, st, P, t->cond_off_dev, t->cond_rows_dev, t->n_cond, cond_idx,
                       t->xe[0], S, d);
  }
  for (int l = 0; l < Le; ++l) {
    RC(attn_self_fwd<T>(o, t->enc[l].self, enc, l, B, t->xe[2 * l], t->xe[2 * l + 1]));
    RC(ff_fwd<T>(o, t->enc[l].ff, enc, l, B, t->xe[2 * l + 1], t->xe[2 * l + 2]));
  }
  RC(o.norm_drop(t->xe[2 * Le], t->o_eln, t->hE, Me, SITE_ENC + SITE_FIN));
  // decoder
  if (o.dropping(SITE_DEC + SITE_EMB)) {
    hipLaunchKernelGGL(embed_rows_drop_kernel, dim3(ceil_div(Md, 4)), dim3(256), 0, st, t->dec_in, P + t->o_shared, t->xd[0], Md, d, V, g.pad_token_id,
                       o.key(SITE_DEC + SITE_EMB), t->drop_thresh, t->drop_scale);
    M2M_CHECK_HIP(hipGetLastError());
  } else {
    RC(launch_embed_rows(t->dec_in, P + t->o_shared, t->xd[0], Md, d, V, g.pad_token_id, st));
  }
  for (int l = 0; l < Ld; ++l) {
    RC(attn_self_fwd<T>(o, t->dec[l].self, dec, l, B, t->xd[3 * l], t->xd[3 * l + 1]));
    RC(attn_cross_fwd<T>(o, t->dec[l].cross, dec, l, B, t->xd[3 * l + 1], t->xd[3 * l + 2]));
    RC(ff_fwd<T>(o, t->dec[l].ff, dec, l, B, t->xd[3 * l + 2], t->xd[3 * l + 3]));
  }
  RC(o.norm_drop(t->xd[3 * Ld], t->o_dln, t->hD, Md, SITE_DEC + SITE_FIN));
  RC(o.mm(TG_STORE_F32, t->hD, d, 0, o.W(t->o_lm), d, 0, t->logits, V, Md, V, d));
  if (logits_out) M2M_CHECK_HIP(hipMemcpyAsync(logits_out, t->logits, (size_t)Md * V * 4, hipMemcpyDeviceToDevice, st));
  // loss + gradient of the logits (a scaled pass: d (loss * gscale) — where autograd meets the 1/N of gradient accumulation; the loss
  // itself stays unscaled)
  hipLaunchKernelGGL(ce_kernel<T>, dim3(ceil_div(Md, 4)), dim3(256), 0, st, t->logits, labels, scaled ? t->inv_n + 2 : t->inv_n, t->row_loss, (T*)t->dlog,
                     Md, V, ldv);
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(256), 0, st, t->row_loss, Md, t->inv_n, loss_out);
  M2M_CHECK_HIP(hipGetLastError());
  if (!G) return M2M_OK;

  // ================= backward =================
  RC(o.begin_sub(0));
  RC(o.dW(t->dlog, ldv, V, t->hD, d, d, G + t->o_lm, Md));                                        // dW_lm = dlogits^T . hD
  RC(o.end_sub());
  // dhD = dlogits . W_lm: an NT product against the transposed copy, whose rows are V long; when V is no multiple of the product's
  // 16-byte row unit that copy cannot be an operand, and the product reads W_lm itself k-major ([V][d] rows, d % 64 == 0)
  if (V % (t->precision == M2M_PREC_BF16 ? 8 : 4) == 0) RC(o.dX(TG_STORE_F32, t->dlog, ldv, t->o_lm, V, d, t->dh, d, Md));
  else RC(o.mm(TG_STORE_F32, t->dlog, ldv, 0, o.W(t->o_lm), d, 1, t->dh, d, Md, d, V));
  float* dcur = t->dxa;
  float* dnext = t->dxb;
  o.after_site = SITE_DEC + 16 * (Ld - 1) + PL_FF_OUT;
  RC(o.norm_bwd(t->xd[3 * Ld], t->o_dln, t->dh, nullptr, dcur, G, Md, SITE_DEC + SITE_FIN));
  for (int l = Ld - 1; l >= 0; --l) {
    o.after_site = SITE_DEC + 16 * l + PL_CROSS_OUT;
    RC(ff_bwd<T>(o, t->dec[l].ff, dec, l, B, t->xd[3 * l + 2], dcur, dnext, G));
    std::swap(dcur, dnext);
    // ---- cross-attention backward: dcur = d x[3l+2] ----
    o.after_site = SITE_DEC + 16 * l + PL_SELF_OUT;
    RC(attn_cross_bwd<T>(o, t->dec[l].cross, dec, l, B, t->xd[3 * l + 1], dcur, dnext, G));
    std::swap(dcur, dnext);
    // ---- causal self-attention backward ----
    o.after_site = l > 0 ? SITE_DEC + 16 * (l - 1) + PL_FF_OUT : -2;
    RC(attn_self_bwd<T>(o, t->dec[l].self, dec, l, B, t->xd[3 * l], dcur, dnext, G));
    std::swap(dcur, dnext);
  }
  // token embedding (decoder inputs; the encoder is fed inputs_embeds) — hf: modeling_t5.py embed_tokens = shared
  {
    const auto dr = o.drop(SITE_DEC + SITE_EMB);
    M2M_OPT_IN_LDS(embed_bwd_kernel<EMB_NW_SHARED>, 158 * 1024);
    hipLaunchKernelGGL(embed_bwd_kernel<EMB_NW_SHARED>, dim3(V), dim3(64 * EMB_NW_SHARED), embed_bwd_smem(Md), st, t->dec_in, Md, 1, 0, dcur, (int64_t)1, (int64_t)0, G + t->o_shared, d,
                       g.pad_token_id, V, dr.key, dr.thresh, dr.scale, o.gacc);
  }
  // Split pass (data-parallel overlap): everything the decoder side deferred is issued now, so the gradients of the shared embedding,
  // lm_head and every decoder block are FINAL here — the caller's hook releases whoever waits for them — and the encoder side
  // flushes again at the end (into the other half of the tables).  Same products, same reductions: bit-identical gradients.
  if (at_split && o.group) {
    RC(o.flush_group());
    RC(o.flush_norms());
    RC(o.flush_bias());
    RC((*at_split)());
    o.phase = 1;
  }
  // (Single-GPU passes flush ONCE, at the end.  Round 3 measured the alternative — the decoder half of the grouped launch and the
  //  decoder's small reductions issued here on the side stream, beside the encoder's backward chain: 3.73 -> 3.86 ms per pass at
  //  16 clips x S = 261, unchanged at 64 clips and at S = 190.  The chain's launches are latency-bound, one or two workgroups per CU,
  //  and every one of them ends when its slowest workgroup does; sharing CUs with a matrix-core-bound launch stretches all of them by
  //  more than the 0.18 ms it hides.  Stream priorities (main highest, side lowest) did not change that and cost 0.18 ms on their own.)
  // encoder
  o.after_site = SITE_ENC + 16 * (Le - 1) + PL_FF_OUT;
  RC(o.norm_bwd(t->xe[2 * Le], t->o_eln, t->dhE, nullptr, dcur, G, Me, SITE_ENC + SITE_FIN));
  for (int l = Le - 1; l >= 0; --l) {
    o.after_site = SITE_ENC + 16 * l + PL_SELF_OUT;
    RC(ff_bwd<T>(o, t->enc[l].ff, enc, l, B, t->xe[2 * l + 1], dcur, dnext, G));
    std::swap(dcur, dnext);
    o.after_site = l > 0 ? SITE_ENC + 16 * (l - 1) + PL_FF_OUT : -2;
    RC(attn_self_bwd<T>(o, t->enc[l].self, enc, l, B, t->xe[2 * l], dcur, dnext, G));
    std::swap(dcur, dnext);
  }
  // The tail of the pass is a set of reductions that do not depend on one another: the grouped weight-gradient launch (0.35 ms,
  // seven rounds of workgroups) and a handful of small ones — conditioning-embedding rows, the norm-weight column sums, the
  // relative-position-bias reductions (~90 us as a chain).  The small ones go to the side stream and run beside the big launch.
  const bool fork = o.group && st_side && t->sw.tail_side;
  hipStream_t small = fork ? st_side : st;
  if (fork) {
    M2M_CHECK_HIP(hipEventRecord(t->ev_ready, st));
    M2M_CHECK_HIP(hipStreamWaitEvent(st_side, t->ev_ready, 0));
  }
  // conditioning embeddings: rows 0 .. n_cond-1 of every clip's encoder input (ref: music2midi/input.py:57-59)
  for (int i = 0; i < t->n_cond; ++i) {
    const auto dr = o.drop(SITE_ENC + SITE_EMB);
    hipLaunchKernelGGL(embed_bwd_kernel<4>, dim3(t->cond_rows[i]), dim3(256), embed_bwd_smem(B, 4), small, cond_idx, B, t->n_cond, i, dcur, (int64_t)S, (int64_t)i,
                       G + t->o_cond[i], d, 0, t->cond_rows[i], dr.key, dr.thresh, dr.scale, o.gacc);
  }
  M2M_CHECK_HIP(hipGetLastError());
  RC(o.join_side());
  o.st = small;
  rc = o.flush_norms();
  if (rc == M2M_OK) rc = o.flush_bias();
  o.st = st;
  if (rc != M2M_OK) return rc;
  if (fork) M2M_CHECK_HIP(hipEventRecord(t->ev_free[0], st_side));
  RC(o.flush_group());
  if (fork) M2M_CHECK_HIP(hipStreamWaitEvent(st, t->ev_free[0], 0));
  return M2M_OK;
}

}  // namespace

// ------------------------------------------------------------------ C ABI ---
namespace { void drop_graph(m2m_trainer* t); }

extern "C" int m2m_trainer_create(const m2m_t5_geometry* geom, int n_cond, const int* cond_rows, int precision, int max_batch,
                                  int max_enc_len, int max_dec_len, m2m_trainer** out) {
  M2M_REQUIRE(geom && out && (n_cond == 0 || cond_rows), "m2m_trainer_create: null argument");
  M2M_REQUIRE(precision == M2M_PREC_FP32 || precision == M2M_PREC_BF16 || precision == M2M_PREC_FP8, "m2m_trainer_create: bad precision %d", precision);
  const bool fp8 = precision == M2M_PREC_FP8;
  if (fp8) {
    precision = M2M_PREC_BF16;       // storage type and every non-projection product are the bf16 mode's
    M2M_REQUIRE(geom->d_model % 128 == 0 && geom->d_ff % 128 == 0 && (geom->num_heads * geom->d_kv) % 128 == 0,
                "m2m_trainer_create: fp8 mode needs d_model, d_ff and num_heads*d_kv to be multiples of 128 (MX blocks of 32 in 128-byte rows)");
  }
  M2M_REQUIRE(geom->d_kv == DK, "m2m_trainer_create: d_kv=%d unsupported (64 only)", geom->d_kv);
  M2M_REQUIRE(geom->d_model % 64 == 0 && geom->d_model <= 512 && geom->d_ff % 8 == 0, "m2m_trainer_create: d_model must be a multiple of 64 (<= 512), d_ff of 8");
  // the embedding kernels map an ignored label (-100) to pad_token_id and read its row: every special id must be a row
  M2M_REQUIRE(geom->vocab_size >= 2 && geom->pad_token_id >= 0 && geom->pad_token_id < geom->vocab_size && geom->eos_token_id >= 0 &&
                  geom->eos_token_id < geom->vocab_size && geom->decoder_start_token_id >= 0 && geom->decoder_start_token_id < geom->vocab_size,
              "m2m_trainer_create: pad_token_id=%d, eos_token_id=%d and decoder_start_token_id=%d must lie in [0, vocab_size=%d)",
              geom->pad_token_id, geom->eos_token_id, geom->decoder_start_token_id, geom->vocab_size);
  M2M_REQUIRE(n_cond >= 0 && n_cond <= 8 && max_batch >= 1 && max_enc_len > n_cond && max_dec_len >= 1, "m2m_trainer_create: bad sizes");
  // embed_bwd_kernel keeps the pass's whole id list in LDS (embed_bwd_smem: 4 bytes per label position + 16 KiB against the 158 KiB opt-in)
  M2M_REQUIRE(embed_bwd_smem(max_batch * max_dec_len) <= (size_t)158 * 1024,
              "m2m_trainer_create: max_batch * max_dec_len = %d label positions per pass exceed the %d the shared-embedding gradient kernel "
              "lists in LDS; use a smaller dataloader batch or shorter label sequences (the reference trains 16 x <= ~360)",
              max_batch * max_dec_len, (int)((158 * 1024 - EMB_NW_SHARED * 256 * 4) / 4));
  m2m_trainer* t = new m2m_trainer();
  t->g = *geom; t->precision = precision; t->inner = geom->num_heads * geom->d_kv; t->n_cond = n_cond;
  t->es = precision == M2M_PREC_BF16 ? 2 : 4;
  t->fp8 = fp8;
  // Gradient operands: e4m3 by default — with a scale per 32 elements the range of e5m2 is not needed, and its third
  // mantissa bit halves the noise every backward product adds (measured on the full model, per-tensor gradient cosine
  // against the fp32 oracle: e5m2 median 0.931 / min 0.908; e4m3: see tests/test_train_gpu.py).  M2M_FP8_GRAD=e5m2 selects e5m2.
  // every environment switch the trainer obeys is read here, once: t->sw by its constructor above
  t->enc_sw = read_enc_switches();
  t->max_batch = max_batch; t->max_enc = max_enc_len; t->max_dec = max_dec_len;
  t->cond_rows.assign(cond_rows, cond_rows + n_cond);
  build_layout(t);
  int rc = build_arena(t);
  if (rc == M2M_OK) rc = build_optimizer(t);
  if (rc != M2M_OK) { m2m_trainer_destroy(t); return rc; }
  // streams / events of the step
  if (t->sw.side) {
    hipError_t e = hipStreamCreateWithFlags(&t->s_main, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&t->s_side, hipStreamNonBlocking);
    hipEvent_t* evs[] = {&t->ev_in, &t->ev_out, &t->ev_ready, &t->ev_free[0], &t->ev_free[1], &t->ev_mid};
    for (hipEvent_t* ev : evs)
      if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    if (e != hipSuccess) { set_error("m2m_trainer_create: stream / event creation failed: %s", hipGetErrorString(e)); m2m_trainer_destroy(t); return M2M_ERR_HIP; }
  }
  *out = t;
  return M2M_OK;
}

extern "C" void m2m_trainer_destroy(m2m_trainer* t) {
  if (!t) return;
  (void)hipDeviceSynchronize();
  drop_graph(t);
  hipEvent_t evs[] = {t->ev_in, t->ev_out, t->ev_ready, t->ev_free[0], t->ev_free[1], t->ev_mid};
  for (hipEvent_t ev : evs)
    if (ev) (void)hipEventDestroy(ev);
  if (t->s_main) (void)hipStreamDestroy(t->s_main);
  if (t->s_side) (void)hipStreamDestroy(t->s_side);
  if (t->arena) (void)hipFree(t->arena);
  if (t->af_mem) (void)hipFree(t->af_mem);
  delete t;
}

extern "C" int64_t m2m_trainer_num_params(const m2m_trainer* t) { return t ? t->n_floats : (int64_t)M2M_ERR_INVALID; }
extern "C" int m2m_trainer_num_tensors(const m2m_trainer* t) { return t ? (int)t->tensors.size() : M2M_ERR_INVALID; }
extern "C" int64_t m2m_trainer_workspace_bytes(const m2m_trainer* t) { return t ? t->arena_bytes : (int64_t)M2M_ERR_INVALID; }

extern "C" int m2m_trainer_tensor_info(const m2m_trainer* t, int index, m2m_tensor_info* out) {
  M2M_REQUIRE(t && out, "m2m_trainer_tensor_info: null argument");
  M2M_REQUIRE(index >= 0 && index < (int)t->tensors.size(), "m2m_trainer_tensor_info: index %d out of range", index);
  const TensorDesc& d = t->tensors[index];
  memset(out, 0, sizeof(*out));
  strncpy(out->name, d.name.c_str(), sizeof(out->name) - 1);
  out->offset = d.off; out->rows = d.rows; out->cols = d.cols;
  return M2M_OK;
}

namespace {

// relative-position bucket tables of (S, L) on the device (host-built, uploaded synchronously: never inside a capture)
int ensure_tables(m2m_trainer* t, int S, int L, hipStream_t st) {
  const m2m_t5_geometry& g = t->g;
  if (t->tab_S != S) {
    const std::vector<int> eb = bucket_table(g, S, S, true);
    M2M_CHECK_HIP(hipMemcpyAsync(t->ebucket, eb.data(), eb.size() * 4, hipMemcpyHostToDevice, st));
    M2M_CHECK_HIP(hipStreamSynchronize(st));   // eb is a stack object
    t->tab_S = S;
  }
  if (t->tab_L != L) {
    const std::vector<int> db = bucket_table(g, L, L, false);
    M2M_CHECK_HIP(hipMemcpyAsync(t->dbucket, db.data(), db.size() * 4, hipMemcpyHostToDevice, st));
    M2M_CHECK_HIP(hipStreamSynchronize(st));
    t->tab_L = L;
  }
  return M2M_OK;
}

int run_pass(m2m_trainer* t, const float* P, const float* x, const int64_t* cond, const int64_t* labels, int B, int S, int L, float* loss, float* G,
             float* logits, hipStream_t st, hipStream_t side, const std::function<int()>* at_split = nullptr) {
  return t->precision == M2M_PREC_BF16 ? forward_backward_t<bf16_t>(t, P, x, cond, labels, B, S, L, loss, G, logits, st, side, at_split)
                                       : forward_backward_t<float>(t, P, x, cond, labels, B, S, L, loss, G, logits, st, side, at_split);
}

void drop_slot_graphs(m2m_trainer::GraphSlot& s) {
  if (s.gexec) { (void)hipGraphExecDestroy(s.gexec); s.gexec = nullptr; }
  if (s.gexec2) { (void)hipGraphExecDestroy(s.gexec2); s.gexec2 = nullptr; }
}
void drop_graph(m2m_trainer* t) {
  for (auto& s : t->slots) { drop_slot_graphs(s); s.valid = false; s.calls = 0; }
}
// the slot of `key`: its own if the key is cached, else the least recently used one, recycled (tables stay: the next direct pass
// compares against their host image and uploads what differs — behind a stream sync, so no kept graph of THIS slot is in flight)
int slot_for(m2m_trainer* t, const m2m_trainer::GraphKey& key) {
  int lru = 0;
  for (int i = 0; i < m2m_trainer::N_SLOTS; ++i) {
    if (t->slots[i].valid && t->slots[i].key == key) return i;
    if (!t->slots[i].valid) { if (t->slots[lru].valid) lru = i; }
    else if (t->slots[lru].valid && t->slots[i].last_use < t->slots[lru].last_use) lru = i;
  }
  m2m_trainer::GraphSlot& s = t->slots[lru];
  drop_slot_graphs(s);
  s.key = key; s.valid = true; s.calls = 0;
  return lru;
}

}  // namespace

// One forward (+ backward) pass.  Three ways to issue the same ~600 kernels, chosen here:
//  * directly on the caller's stream (forward only, M2M_TRAIN_GRAPH=0 / M2M_TRAIN_SIDE=0, or the first call of a shape);
//  * on the trainer's own two streams: the weight-gradient products of a sub-layer run beside the next sub-layer's
//    gradient chain (they fill the CUs the small dX products leave idle);
//  * as ONE captured HIP graph of those two streams, replayed from the second call with the same buffers and shapes on:
//    inputs are staged into trainer-owned buffers first, so the graph never holds a caller pointer other than the flat
//    parameter / gradient buffers (part of its key), and the dropout key advances on the device.
extern "C" int m2m_train_forward_backward(m2m_trainer* t, const float* params_dev, const float* enc_inputs_dev, const int64_t* cond_idx_dev,
                                          const int64_t* labels_dev, int B, int S, int Ld, float* loss_out_dev, float* grads_dev,
                                          float* logits_out_dev, void* stream) {
  M2M_REQUIRE(t && params_dev && enc_inputs_dev && labels_dev && loss_out_dev, "m2m_train_forward_backward: null argument");
  M2M_REQUIRE(t->n_cond == 0 || cond_idx_dev, "m2m_train_forward_backward: cond_idx_dev is null");
  M2M_REQUIRE(B >= 1 && B <= t->max_batch && S > t->n_cond && S <= t->max_enc && Ld >= 1 && Ld <= t->max_dec,
              "m2m_train_forward_backward: (B=%d, S=%d, Ld=%d) outside the trainer's (%d, %d, %d)", B, S, Ld, t->max_batch, t->max_enc, t->max_dec);
  hipStream_t caller = (hipStream_t)stream;
  const EncSwitchScope sw_scope(&t->enc_sw);
  int rc = ensure_tables(t, S, Ld, caller);
  if (rc != M2M_OK) return rc;
  const bool two = grads_dev && t->sw.side && t->s_main && t->s_side;
  // split pass: the stream that carries the decoder-side gradient all-reduce waits for ev_mid, recorded where those gradients are final
  const bool split = grads_dev && t->sync_stream && t->ev_mid && t->sw.dw_group && !(t->fp8 && t->sw.fp8.dw);
  hipStream_t work = two ? t->s_main : caller;
  const std::function<int()> release = [t, work]() -> int {
    M2M_CHECK_HIP(hipEventRecord(t->ev_mid, work));
    M2M_CHECK_HIP(hipStreamWaitEvent(t->sync_stream, t->ev_mid, 0));
    return M2M_OK;
  };
  // A sync stream is set but this pass is NOT split (per-product weight gradients: M2M_TRAIN_DW_GROUP=0, fp8 weight gradients):
  // whoever enqueues the early all-reduce on the sync stream must still find FINISHED gradients, so the stream is released at
  // the END of the pass instead of half-way (no overlap, no race)
  const bool release_at_end = grads_dev && t->sync_stream && t->ev_mid && !split;
  if (!two) {
    t->gscale_src = nullptr;                      // (a scaled pass issued directly carries its factor as a kernel argument)
    t->cur_slot = m2m_trainer::N_SLOTS;
    rc = run_pass(t, params_dev, enc_inputs_dev, cond_idx_dev, labels_dev, B, S, Ld, loss_out_dev, grads_dev, logits_out_dev, caller, nullptr,
                  split ? &release : nullptr);
    if (rc == M2M_OK && release_at_end) rc = release();
    return rc;
  }

  // ---- stage the inputs (stream-ordered behind whatever produced them), then hand over to the trainer's streams ----
  const m2m_t5_geometry& g = t->g;
  // (one launch instead of three copy dispatches of ~5 us each on the caller's stream: they sit between two steps)
  {
    const int64_t n4 = (int64_t)B * S * g.d_model / 4, nl = (int64_t)B * Ld, nc = (int64_t)B * t->n_cond;
    hipLaunchKernelGGL(stage_inputs_kernel, dim3(grid_1d(n4 + nl + nc)), dim3(256), 0, caller, reinterpret_cast<const float4*>(enc_inputs_dev),
                       reinterpret_cast<float4*>(t->xe[0]), n4, labels_dev, reinterpret_cast<int64_t*>(t->labels_buf), nl, cond_idx_dev,
                       reinterpret_cast<int64_t*>(t->cond_buf), nc, (t->gmode & m2m_trainer::GM_SCALED) ? t->inv_n + 3 : nullptr, t->gscale);
    M2M_CHECK_HIP(hipGetLastError());
  }
  M2M_CHECK_HIP(hipEventRecord(t->ev_in, caller));
  M2M_CHECK_HIP(hipStreamWaitEvent(t->s_main, t->ev_in, 0));
  t->gscale_src = (t->gmode & m2m_trainer::GM_SCALED) ? t->inv_n + 3 : nullptr;     // staged above: one graph serves every factor

  const m2m_trainer::GraphKey key{params_dev, grads_dev, B, S, Ld, t->drop_thresh, t->drop_seed, split, t->gmode};
  const int si = slot_for(t, key);
  m2m_trainer::GraphSlot& slot = t->slots[si];
  slot.calls += 1;
  slot.last_use = ++t->tick;
  t->cur_slot = si;
  if (t->sw.graph && slot.calls >= 2 && !slot.gexec) {                    // second call with this key: capture
    // a split pass becomes TWO graphs: the capture is closed and reopened where the decoder-side gradients are final, and the
    // replay records ev_mid between the two launches
    hipGraphExec_t first = nullptr;
    int n_nodes = 0;
    const auto close_capture = [t, &n_nodes](hipGraphExec_t* out) -> int {
      hipGraph_t graph = nullptr;
      const hipError_t ce = hipStreamEndCapture(t->s_main, &graph);
      if (ce != hipSuccess || !graph) {
        if (graph) (void)hipGraphDestroy(graph);
        set_error("m2m_train_forward_backward: graph capture failed: %s", hipGetErrorString(ce));
        return M2M_ERR_HIP;
      }
      size_t nn = 0;
      if (hipGraphGetNodes(graph, nullptr, &nn) == hipSuccess) n_nodes += (int)nn;
      const hipError_t ie = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
      (void)hipGraphDestroy(graph);
      if (ie != hipSuccess) { *out = nullptr; set_error("m2m_train_forward_backward: hipGraphInstantiate: %s", hipGetErrorString(ie)); return M2M_ERR_HIP; }
      return M2M_OK;
    };
    const std::function<int()> cut = [t, &first, &close_capture]() -> int {
      const int r = close_capture(&first);
      if (r != M2M_OK) return r;
      M2M_CHECK_HIP(hipStreamBeginCapture(t->s_main, hipStreamCaptureModeThreadLocal));
      return M2M_OK;
    };
    M2M_CHECK_HIP(hipStreamBeginCapture(t->s_main, hipStreamCaptureModeThreadLocal));
    rc = run_pass(t, params_dev, t->xe[0], t->cond_buf, t->labels_buf, B, S, Ld, t->loss_dev, grads_dev, nullptr, t->s_main, t->s_side,
                  split ? &cut : nullptr);
    hipGraphExec_t last = nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(t->s_main, &cs);
    int rc2 = M2M_OK;
    if (cs != hipStreamCaptureStatusNone) rc2 = close_capture(&last);       // (a failed cut leaves no capture open)
    if (rc != M2M_OK || rc2 != M2M_OK || (split && !first)) {
      if (first) (void)hipGraphExecDestroy(first);
      if (last) (void)hipGraphExecDestroy(last);
      if (rc == M2M_OK && rc2 == M2M_OK) { set_error("m2m_train_forward_backward: the split pass never reached its split point"); rc = M2M_ERR_INVALID; }
      slot.valid = false;                                                    // the next call starts this key over
      return rc != M2M_OK ? rc : rc2;
    }
    if (split) { slot.gexec = first; slot.gexec2 = last; } else { slot.gexec = last; }
    slot.nodes = n_nodes;
  }
  // A replayed graph that is not split is launched straight on the CALLER's stream: the inputs were staged there, the loss copy and the
  // optimizer follow there, so neither hand-over event (ev_in / ev_out: a cross-stream dependency on each side of every step) is needed.
  // M2M_TRAIN_GRAPH_CALLER=0: on the trainer's own stream, as the directly issued and the split passes run.
  if (slot.gexec && !split && !release_at_end && t->sw.graph_caller) {
    M2M_CHECK_HIP(hipGraphLaunch(slot.gexec, caller));
    M2M_CHECK_HIP(hipMemcpyAsync(loss_out_dev, t->loss_dev, 4, hipMemcpyDeviceToDevice, caller));
    if (logits_out_dev)
      M2M_CHECK_HIP(hipMemcpyAsync(logits_out_dev, t->logits, (size_t)B * Ld * g.vocab_size * 4, hipMemcpyDeviceToDevice, caller));
    return M2M_OK;
  }
  if (slot.gexec) {
    M2M_CHECK_HIP(hipGraphLaunch(slot.gexec, t->s_main));
    if (split) {
      rc = release();
      if (rc != M2M_OK) return rc;
      M2M_CHECK_HIP(hipGraphLaunch(slot.gexec2, t->s_main));
    }
  } else {
    rc = run_pass(t, params_dev, t->xe[0], t->cond_buf, t->labels_buf, B, S, Ld, t->loss_dev, grads_dev, nullptr, t->s_main, t->s_side,
                  split ? &release : nullptr);
    if (rc != M2M_OK) { slot.valid = false; return rc; }
  }
  if (release_at_end) { rc = release(); if (rc != M2M_OK) return rc; }
  M2M_CHECK_HIP(hipEventRecord(t->ev_out, t->s_main));
  M2M_CHECK_HIP(hipStreamWaitEvent(caller, t->ev_out, 0));
  M2M_CHECK_HIP(hipMemcpyAsync(loss_out_dev, t->loss_dev, 4, hipMemcpyDeviceToDevice, caller));
  if (logits_out_dev)
    M2M_CHECK_HIP(hipMemcpyAsync(logits_out_dev, t->logits, (size_t)B * Ld * g.vocab_size * 4, hipMemcpyDeviceToDevice, caller));
  return M2M_OK;
}

// Gradient accumulation: the same pass with d (loss * grad_scale) as its gradient, ADDED to grads_dev when `accumulate` is set (every
// writer of the flat buffer — the grouped weight-gradient launch, the norm column sums, the bias-table and embedding reductions —
// adds in its own epilogue; there is no extra pass over the buffer).  The pad ranges between tensors are zeroed as in the
// overwriting pass.  The mode is part of the per-shape graph key; the factor is not (one graph per shape and mode serves any N).
extern "C" int m2m_train_forward_backward_acc(m2m_trainer* t, const float* params_dev, const float* enc_inputs_dev, const int64_t* cond_idx_dev,
                                              const int64_t* labels_dev, int B, int S, int Ld, float* loss_out_dev, float* grads_dev,
                                              float* logits_out_dev, float grad_scale, int accumulate, void* stream) {
  M2M_REQUIRE(t && grads_dev, "m2m_train_forward_backward_acc: null trainer or gradient buffer");
  M2M_REQUIRE(isfinite(grad_scale) && grad_scale > 0.f && (accumulate == 0 || accumulate == 1),
              "m2m_train_forward_backward_acc: grad_scale must be finite and > 0 (got %g), accumulate 0 or 1 (got %d)", (double)grad_scale, accumulate);
  t->gmode = m2m_trainer::GM_SCALED | (accumulate ? m2m_trainer::GM_ACC : 0);
  t->gscale = grad_scale;
  const int rc = m2m_train_forward_backward(t, params_dev, enc_inputs_dev, cond_idx_dev, labels_dev, B, S, Ld, loss_out_dev, grads_dev,
                                            logits_out_dev, stream);
  t->gmode = 0;
  t->gscale = 1.f;
  t->gscale_src = nullptr;
  return rc;
}

extern "C" int m2m_trainer_set_dropout(m2m_trainer* t, float p, uint64_t seed) {
  M2M_REQUIRE(t && p >= 0.f && p < 1.f, "m2m_trainer_set_dropout: p must be in [0, 1)");
  t->drop_thresh = p > 0.f ? (uint32_t)((double)p * 4294967296.0) : 0u;
  t->drop_scale = 1.0f / (1.0f - p);
  t->drop_seed = seed;
  M2M_CHECK_HIP(hipDeviceSynchronize());                               // nothing of an earlier pass still reads the counter
  M2M_CHECK_HIP(hipMemset(t->step_ctr_dev, 0, 8));                     // the mask sequence restarts
  return M2M_OK;
}

// Data-parallel overlap.  With a sync stream set, every forward+backward call issues the backward pass in two parts and makes
// `stream` wait (an event, no host sync) for the point where the gradients in the two "early" ranges are final; work the caller
// then enqueues on `stream` — the all-reduce of those ranges — runs beside the encoder-side backward.  nullptr switches it off.
extern "C" int m2m_trainer_set_sync_stream(m2m_trainer* t, void* stream) {
  M2M_REQUIRE(t, "m2m_trainer_set_sync_stream: null trainer");
  if (stream && !t->ev_mid) {                                            // (a trainer built without its own streams has no events yet)
    M2M_CHECK_HIP(hipEventCreateWithFlags(&t->ev_mid, hipEventDisableTiming));
  }
  t->sync_stream = (hipStream_t)stream;
  return M2M_OK;
}
// out[0..3] = {offset, count, offset, count} (floats of the flat gradient buffer): shared embedding + lm_head, and the decoder blocks
extern "C" int m2m_trainer_early_grad_ranges(const m2m_trainer* t, int64_t* out) {
  M2M_REQUIRE(t && out, "m2m_trainer_early_grad_ranges: null argument");
  out[0] = 0; out[1] = t->o_erb;
  out[2] = t->dec_begin; out[3] = t->dec_end - t->dec_begin;
  return M2M_OK;
}

extern "C" int m2m_trainer_graph_nodes(const m2m_trainer* t) {
  if (!t) return M2M_ERR_INVALID;
  const m2m_trainer::GraphSlot& s = t->slots[t->cur_slot];
  return (s.valid && s.gexec) ? s.nodes : 0;
}

extern "C" int m2m_adafactor_step(m2m_trainer* t, float* params_dev, const float* grads_dev, void* stream) {
  M2M_REQUIRE(t && params_dev && grads_dev, "m2m_adafactor_step: null argument");
  t->step += 1;
  if (t->clip_mode == AF_CLIP_NORM) {      // the norm of this step's gradient first; its two words stay readable (m2m_trainer_grad_norm, grads_dev = NULL)
    const int rc = launch_grad_norm(t->af, grads_dev, t->clip_value, t->af.gn_words, (hipStream_t)stream);
    if (rc != M2M_OK) return rc;
  }
  return launch_adafactor(t->af, params_dev, grads_dev, t->step, (hipStream_t)stream, t->clip_mode, t->af.gn_words + 1, t->clip_value);
}

extern "C" int m2m_trainer_set_grad_clip(m2m_trainer* t, int algorithm, float value) {
  M2M_REQUIRE(t, "m2m_trainer_set_grad_clip: null trainer");
  M2M_REQUIRE(algorithm == AF_CLIP_OFF || algorithm == AF_CLIP_NORM || algorithm == AF_CLIP_VALUE,
              "m2m_trainer_set_grad_clip: algorithm must be 0 (off), 1 (norm) or 2 (value), got %d", algorithm);
  M2M_REQUIRE(algorithm == AF_CLIP_OFF || value > 0.f, "m2m_trainer_set_grad_clip: the clip value must be > 0 (got %g)", (double)value);
  t->clip_mode = algorithm;
  t->clip_value = algorithm == AF_CLIP_OFF ? 0.f : value;
  return M2M_OK;
}

extern "C" int m2m_trainer_grad_norm(m2m_trainer* t, const float* grads_dev, float* out_dev, void* stream) {
  M2M_REQUIRE(t && out_dev, "m2m_trainer_grad_norm: null argument");
  const float* words = t->af.gn_words;                 // grads_dev NULL: the words the last norm-mode step left
  if (grads_dev) {
    const float max_norm = t->clip_mode == AF_CLIP_NORM ? t->clip_value : INFINITY;      // off / value: coef against +inf, i.e. 1
    const int rc = launch_grad_norm(t->af, grads_dev, max_norm, t->af.gn_words + 2, (hipStream_t)stream);
    if (rc != M2M_OK) return rc;
    words = t->af.gn_words + 2;
  }
  M2M_CHECK_HIP(hipMemcpyAsync(out_dev, words, 2 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return M2M_OK;
}

extern "C" int m2m_adafactor_get_step(const m2m_trainer* t) { return t ? t->step : M2M_ERR_INVALID; }
extern "C" int64_t m2m_adafactor_state_floats(const m2m_trainer* t) { return t ? t->af.state_floats : (int64_t)M2M_ERR_INVALID; }

extern "C" int m2m_adafactor_state_export(const m2m_trainer* t, float* state_out_dev, void* stream) {
  M2M_REQUIRE(t && state_out_dev, "m2m_adafactor_state_export: null argument");
  M2M_CHECK_HIP(hipMemcpyAsync(state_out_dev, t->af.state, (size_t)t->af.state_floats * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return M2M_OK;
}
extern "C" int m2m_adafactor_state_import(m2m_trainer* t, const float* state_in_dev, int step, void* stream) {
  M2M_REQUIRE(t && state_in_dev && step >= 0, "m2m_adafactor_state_import: bad argument");
  M2M_CHECK_HIP(hipMemcpyAsync(t->af.state, state_in_dev, (size_t)t->af.state_floats * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  t->step = step;
  return M2M_OK;
}

#ifdef M2M_ST_STAMP
// diagnostic builds only (not declared in the public header): the stripe kernel's last phase stamps, [variant][phase]
extern "C" int m2m_debug_stripe_stamps(unsigned long long* out_host) {
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(m2m::g_st_stamp), sizeof(unsigned long long) * 48) == hipSuccess ? 0 : -1;
}
#endif
