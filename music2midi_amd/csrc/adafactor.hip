// Adafactor step of the training path (the plan and its device tables: train.h; build_optimizer in train.hip fills them).
#include "train.h"

#include <math.h>

namespace m2m {

// transformers.optimization.Adafactor as ref: music2midi/model.py:27-30 builds it:
//   Adafactor(params, lr=None, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0.0,
//             scale_parameter=True, relative_step=True, warmup_init=True)
// per tensor p with gradient g at step t (1-based):
//   rho   = min(1e-6 * t, 1/sqrt(t))                       (relative step with warm-up init)
//   lr    = max(1e-3, rms(p)) * rho                        (scale_parameter)
//   b2    = 1 - t^-0.8
//   u     = g^2 + 1e-30
//   2-D:  R <- b2 R + (1-b2) mean_cols(u);  C <- b2 C + (1-b2) mean_rows(u);  upd = g * rsqrt(R / mean(R)) [row] * rsqrt(C) [col]
//   1-D:  V <- b2 V + (1-b2) u;             upd = g * rsqrt(V)
//   upd  /= max(1, rms(upd) / 1.0);   p <- p - lr * upd
// Three passes over (p, g) with the reductions between them; one launch per pass for ALL tensors (block -> (tensor,
// row block) through a table), every reduction in a fixed order.  A block takes AF_ROWS rows of a matrix, or a whole vector as one row.

// Gradient clipping (Lightning's Trainer(gradient_clip_val, gradient_clip_algorithm); rules: music2midi_amd/clipping.py) is folded into the
// three passes that read g, as a template parameter CLIP: 0 off (the code as it was), 1 norm: g * coef with coef the device word
// gn_finish wrote (grad_clip.hip), 2 value: g clamped to +-v.  The clipped value is taken straight after the load, before anything else
// touches g, so the second moments see the clipped gradient exactly as Adafactor does after clip_grad_norm_'s g.mul_(coef).  No pass
// writes G: the gradient buffer keeps the unclipped gradient after the step.
template <int CLIP>
__device__ __forceinline__ float af_clip_arg(const float* __restrict__ coef_dev, float clip_v) {      // once per workgroup
  return CLIP == 1 ? *coef_dev : clip_v;
}
template <int CLIP>
__device__ __forceinline__ float af_clipped(float g, float cv) {
  if (CLIP == 1) return g * cv;                                  // one rounded fp32 multiply
  if (CLIP == 2) return g < -cv ? -cv : (g > cv ? cv : g);       // not fminf / fmaxf: they would swallow a NaN
  return g;
}

// pass A: per block: sum p^2, per-row sum of (g^2 + eps1) -> rowsum[tensor rows], per-block column partial sums
template <int CLIP>
__global__ __launch_bounds__(256) void af_pass_a(const AfBlock* __restrict__ blocks, const AfTensor* __restrict__ tensors,
                                                 const float* __restrict__ P, const float* __restrict__ G, float* __restrict__ rowsum,
                                                 float* __restrict__ colpart, float* __restrict__ blk_p2,
                                                 const float* __restrict__ coef_dev, float clip_v) {
  __shared__ float sred[256];
  const float cv = af_clip_arg<CLIP>(coef_dev, clip_v);
  const AfBlock bk = blocks[blockIdx.x];
  const AfTensor t = tensors[bk.tensor];
  const float* p = P + t.offset;
  const float* g = G + t.offset;
  float p2 = 0.f;
  const int r1 = min(bk.row0 + AF_ROWS, t.rows);
  // thread tid owns columns tid, tid + 256, ... ; rows are walked in order -> fixed summation order per column.  ONE read of
  // g and p (the first form read g a second time for the row sums, one dependent load per row: 157 us per step): the per-row
  // partial sums of this thread's columns stay in registers and are reduced by wave, then over the four waves, in a fixed order
  __shared__ float rred[4][AF_ROWS];
  float rs[AF_ROWS];
#pragma unroll
  for (int j = 0; j < AF_ROWS; ++j) rs[j] = 0.f;
  for (int c = threadIdx.x; c < t.cols; c += 256) {
    float gv[AF_ROWS], pv[AF_ROWS];
#pragma unroll
    for (int j = 0; j < AF_ROWS; ++j) {
      const int r = min(bk.row0 + j, r1 - 1);          // clamped: every load of the tile is in flight at once
      gv[j] = g[(int64_t)r * t.cols + c];
      if (CLIP) gv[j] = af_clipped<CLIP>(gv[j], cv);
      pv[j] = p[(int64_t)r * t.cols + c];
    }
    float cs = 0.f;
#pragma unroll
    for (int j = 0; j < AF_ROWS; ++j) {
      if (bk.row0 + j < r1) {
        const float q = gv[j] * gv[j] + 1e-30f;
        cs += q;
        rs[j] += q;
        p2 += pv[j] * pv[j];
      }
    }
    colpart[bk.col_off + c] = cs;
  }
  {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < AF_ROWS; ++j) {
      const float v = wave_sum(rs[j]);
      if (lane == 0) rred[wave][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < AF_ROWS && bk.row0 + (int)threadIdx.x < r1)
      rowsum[t.row_off + bk.row0 + threadIdx.x] = (rred[0][threadIdx.x] + rred[1][threadIdx.x]) + (rred[2][threadIdx.x] + rred[3][threadIdx.x]);
  }
  sred[threadIdx.x] = p2;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sred[threadIdx.x] += sred[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) blk_p2[blockIdx.x] = sred[0];
}

// pass A2: one block per tensor: finish rms(p), update the factored second moments, derive the row / column factors
__global__ __launch_bounds__(256) void af_pass_a2(const AfTensor* __restrict__ tensors, const float* __restrict__ rowsum,
                                                  const float* __restrict__ colpart, const float* __restrict__ blk_p2,
                                                  float* __restrict__ state, float* __restrict__ rfac, float* __restrict__ cfac,
                                                  float* __restrict__ tstat, float beta2t, float omb2t) {
  __shared__ float sred[256];
  const AfTensor t = tensors[blockIdx.x];
  float acc = 0.f;
  for (int b = threadIdx.x; b < t.nblocks; b += 256) acc += blk_p2[t.block0 + b];
  sred[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) { if (threadIdx.x < s) sred[threadIdx.x] += sred[threadIdx.x + s]; __syncthreads(); }
  const float p_rms = sqrtf(sred[0] / (float)((int64_t)t.rows * t.cols));
  __syncthreads();
  float* R = state + t.state_off;               // [rows] (matrix) or [cols] full second moment (vector: rows == 1)
  float* C = R + t.rows;                        // [cols] (matrix only)
  if (t.rows > 1) {
    // rows
    float racc = 0.f;
    for (int r = threadIdx.x; r < t.rows; r += 256) {
      const float v = beta2t * R[r] + omb2t * (rowsum[t.row_off + r] / (float)t.cols);
      R[r] = v;
      racc += v;
    }
    sred[threadIdx.x] = racc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (threadIdx.x < s) sred[threadIdx.x] += sred[threadIdx.x + s]; __syncthreads(); }
    const float rmean = sred[0] / (float)t.rows;
    __syncthreads();
    for (int r = threadIdx.x; r < t.rows; r += 256) rfac[t.row_off + r] = rsqrtf(R[r] / rmean);
    for (int c = threadIdx.x; c < t.cols; c += 256) {
      float cs = 0.f;
      int b = 0;
      for (; b + 8 <= t.nblocks; b += 8) {            // eight partial rows in flight (the plain loop paid a memory round trip per row block: 28 us per step)
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = colpart[t.col_off + (int64_t)(b + u) * t.cols + c];
#pragma unroll
        for (int u = 0; u < 8; ++u) cs += v[u];
      }
      for (; b < t.nblocks; ++b) cs += colpart[t.col_off + (int64_t)b * t.cols + c];
      const float v = beta2t * C[c] + omb2t * (cs / (float)t.rows);
      C[c] = v;
      cfac[t.cfac_off + c] = rsqrtf(v);
    }
  } else {
    for (int c = threadIdx.x; c < t.cols; c += 256) {
      const float v = beta2t * R[c] + omb2t * colpart[t.col_off + c];     // one block, one row: colpart = g^2 + eps
      R[c] = v;
      cfac[t.cfac_off + c] = rsqrtf(v);
    }
    if (threadIdx.x == 0) rfac[t.row_off] = 1.0f;
  }
  if (threadIdx.x == 0) tstat[2 * blockIdx.x] = p_rms;
}

// pass B: per block sum of upd^2, upd = g * rfac[row] * cfac[col]
template <int CLIP>
__global__ __launch_bounds__(256) void af_pass_b(const AfBlock* __restrict__ blocks, const AfTensor* __restrict__ tensors,
                                                 const float* __restrict__ G, const float* __restrict__ rfac, const float* __restrict__ cfac,
                                                 float* __restrict__ blk_u2, const float* __restrict__ coef_dev, float clip_v) {
  __shared__ float sred[256];
  const float cv = af_clip_arg<CLIP>(coef_dev, clip_v);
  const AfBlock bk = blocks[blockIdx.x];
  const AfTensor t = tensors[bk.tensor];
  const float* g = G + t.offset;
  const int r1 = min(bk.row0 + AF_ROWS, t.rows);
  float u2 = 0.f;
  for (int c = threadIdx.x; c < t.cols; c += 256) {
    const float cf = cfac[t.cfac_off + c];
    float gv[AF_ROWS];
#pragma unroll
    for (int j = 0; j < AF_ROWS; ++j) gv[j] = g[(int64_t)min(bk.row0 + j, r1 - 1) * t.cols + c];
    if (CLIP) {
#pragma unroll
      for (int j = 0; j < AF_ROWS; ++j) gv[j] = af_clipped<CLIP>(gv[j], cv);
    }
#pragma unroll
    for (int j = 0; j < AF_ROWS; ++j) {
      if (bk.row0 + j < r1) {
        const float u = gv[j] * rfac[t.row_off + bk.row0 + j] * cf;
        u2 += u * u;
      }
    }
  }
  sred[threadIdx.x] = u2;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) { if (threadIdx.x < s) sred[threadIdx.x] += sred[threadIdx.x + s]; __syncthreads(); }
  if (threadIdx.x == 0) blk_u2[blockIdx.x] = sred[0];
}
// pass B2: per tensor: step size = lr / max(1, rms(upd))
__global__ __launch_bounds__(256) void af_pass_b2(const AfTensor* __restrict__ tensors, const float* __restrict__ blk_u2,
                                                  float* __restrict__ tstat, float rho) {
  __shared__ float sred[256];
  const AfTensor t = tensors[blockIdx.x];
  float acc = 0.f;
  for (int b = threadIdx.x; b < t.nblocks; b += 256) acc += blk_u2[t.block0 + b];
  sred[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) { if (threadIdx.x < s) sred[threadIdx.x] += sred[threadIdx.x + s]; __syncthreads(); }
  if (threadIdx.x == 0) {
    const float u_rms = sqrtf(sred[0] / (float)((int64_t)t.rows * t.cols));
    const float lr = fmaxf(1e-3f, tstat[2 * blockIdx.x]) * rho;
    tstat[2 * blockIdx.x + 1] = lr / fmaxf(1.0f, u_rms);
  }
}
// pass C: p -= step * g * rfac[row] * cfac[col]
template <int CLIP>
__global__ __launch_bounds__(256) void af_pass_c(const AfBlock* __restrict__ blocks, const AfTensor* __restrict__ tensors,
                                                 float* __restrict__ P, const float* __restrict__ G, const float* __restrict__ rfac,
                                                 const float* __restrict__ cfac, const float* __restrict__ tstat,
                                                 const float* __restrict__ coef_dev, float clip_v) {
  const float cv = af_clip_arg<CLIP>(coef_dev, clip_v);
  const AfBlock bk = blocks[blockIdx.x];
  const AfTensor t = tensors[bk.tensor];
  float* p = P + t.offset;
  const float* g = G + t.offset;
  const float step = tstat[2 * bk.tensor + 1];
  const int r1 = min(bk.row0 + AF_ROWS, t.rows);
  // eight rows of a column in flight per thread (a row-by-row loop kept one load pair per thread in flight: 78 us for the pass's 366 MB; 70 us this way, same arithmetic)
  for (int c = threadIdx.x; c < t.cols; c += 256) {
    const float cf = cfac[t.cfac_off + c];
    for (int r = bk.row0; r < r1; r += 8) {
      float gv[8], pv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t at = (int64_t)min(r + j, r1 - 1) * t.cols + c;
        gv[j] = g[at];
        if (CLIP) gv[j] = af_clipped<CLIP>(gv[j], cv);
        pv[j] = p[at];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (r + j < r1) p[(int64_t)(r + j) * t.cols + c] = pv[j] - gv[j] * (rfac[t.row_off + r + j] * step) * cf;
    }
  }
}

namespace {

template <int CLIP>
void launch_passes(const AfPlan& pl, float* P, const float* G, float beta2t, float omb2t, float rho, const float* coef_dev, float clip_v,
                   hipStream_t st) {
  hipLaunchKernelGGL(af_pass_a<CLIP>, dim3(pl.n_blocks), dim3(256), 0, st, pl.blocks, pl.tensors, P, G, pl.rowsum, pl.colpart, pl.blk_a,
                     coef_dev, clip_v);
  hipLaunchKernelGGL(af_pass_a2, dim3(pl.n_tensors), dim3(256), 0, st, pl.tensors, pl.rowsum, pl.colpart, pl.blk_a, pl.state, pl.rfac,
                     pl.cfac, pl.tstat, beta2t, omb2t);
  hipLaunchKernelGGL(af_pass_b<CLIP>, dim3(pl.n_blocks), dim3(256), 0, st, pl.blocks, pl.tensors, G, pl.rfac, pl.cfac, pl.blk_b, coef_dev,
                     clip_v);
  hipLaunchKernelGGL(af_pass_b2, dim3(pl.n_tensors), dim3(256), 0, st, pl.tensors, pl.blk_b, pl.tstat, rho);
  hipLaunchKernelGGL(af_pass_c<CLIP>, dim3(pl.n_blocks), dim3(256), 0, st, pl.blocks, pl.tensors, P, G, pl.rfac, pl.cfac, pl.tstat,
                     coef_dev, clip_v);
}

}  // namespace

int launch_adafactor(const AfPlan& pl, float* P, const float* G, int step, hipStream_t st, int clip, const float* coef_dev,
                     float clip_value) {
  const double t = (double)step;
  const float beta2t = (float)(1.0 - pow(t, -0.8));
  // 1 - beta2 = t^-0.8 rounded from the double, as the reference's add_(.., alpha=1.0 - beta2t) has it: 1.f - beta2t keeps only the bits
  // above half an ulp of 1, a relative error of up to 3e-8 * t^0.8 (4e-5 at t = 9 999) on every newly added second moment
  const float omb2t = (float)pow(t, -0.8);
  const double rho_d = fmin(1e-6 * t, 1.0 / sqrt(t));
  const float rho = (float)rho_d;
  if (clip == AF_CLIP_NORM) launch_passes<1>(pl, P, G, beta2t, omb2t, rho, coef_dev, 0.f, st);
  else if (clip == AF_CLIP_VALUE) launch_passes<2>(pl, P, G, beta2t, omb2t, rho, nullptr, clip_value, st);
  else launch_passes<0>(pl, P, G, beta2t, omb2t, rho, nullptr, 0.f, st);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

}  // namespace m2m
