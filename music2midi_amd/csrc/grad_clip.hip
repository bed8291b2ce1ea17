// Global gradient norm of the training path: what torch.nn.utils.clip_grad_norm_ computes before it scales (Lightning's
// Trainer(gradient_clip_val=, gradient_clip_algorithm="norm"); the rules: music2midi_amd/clipping.py).  The scaling itself is not
// here: passes A, B and C of the Adafactor step read g * coef on the fly (adafactor.hip, CLIP = 1).
#include "train.h"

#include <math.h>

namespace m2m {

// launch one: one workgroup per AfBlock (AF_ROWS rows of a matrix, or a whole vector) -> blk_g[block] = sum of g^2.  The block tables
// are the optimizer's, so the padding between the tensors of the flat buffer is never read.  Thread tid owns columns tid, tid + 256, ...
// and walks the rows in order; the 256 partial sums are added by pass A's fixed-order tree.
__global__ __launch_bounds__(256) void gn_blocks(const AfBlock* __restrict__ blocks, const AfTensor* __restrict__ tensors,
                                                 const float* __restrict__ G, float* __restrict__ blk_g) {
  __shared__ float sred[256];
  const AfBlock bk = blocks[blockIdx.x];
  const AfTensor t = tensors[bk.tensor];
  const float* g = G + t.offset;
  const int r1 = min(bk.row0 + AF_ROWS, t.rows);
  float g2 = 0.f;
  for (int c = threadIdx.x; c < t.cols; c += 256) {
    float gv[AF_ROWS];
#pragma unroll
    for (int j = 0; j < AF_ROWS; ++j) gv[j] = g[(int64_t)min(bk.row0 + j, r1 - 1) * t.cols + c];      // clamped: every load of the tile in flight at once
#pragma unroll
    for (int j = 0; j < AF_ROWS; ++j)
      if (bk.row0 + j < r1) g2 += gv[j] * gv[j];
  }
  sred[threadIdx.x] = g2;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) sred[threadIdx.x] += sred[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) blk_g[blockIdx.x] = sred[0];
}

// launch two: one workgroup.  Thread i takes tensors i, i + 256, ...: the tensor's block sums in block order, sqrtf -> its norm.  The
// squares of the norms are then added in tensor order (torch's stack of per-tensor norms, not one flat sum), sqrtf again.
__global__ __launch_bounds__(256) void gn_finish(const AfTensor* __restrict__ tensors, int n_tensors, const float* __restrict__ blk_g,
                                                 float max_norm, float* __restrict__ words) {
  // Both sums run in double (a few hundred adds in all): up to 258 block sums of one tensor added one after the other in fp32 would
  // alone cost a few 1e-7 of that tensor's norm.  The norms themselves are fp32 values, as torch's are.
  __shared__ double sq[256];
  double total2 = 0.0;                                 // thread 0's
  for (int base = 0; base < n_tensors; base += 256) {  // more than 256 tensors: another trip
    const int i = base + (int)threadIdx.x;
    double v = 0.0;
    if (i < n_tensors) {
      const AfTensor t = tensors[i];
      double acc = 0.0;
      for (int b = 0; b < t.nblocks; ++b) acc += (double)blk_g[t.block0 + b];
      const float nrm = sqrtf((float)acc);
      v = (double)nrm * (double)nrm;
    }
    sq[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = min(256, n_tensors - base);
      for (int k = 0; k < n; ++k) total2 += sq[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float total = sqrtf((float)total2);
    const float q = max_norm / (total + 1e-6f);
    words[0] = total;
    words[1] = q > 1.0f ? 1.0f : q;                    // torch.clamp(q, max=1): a NaN stays a NaN (fminf would answer 1)
  }
}

int launch_grad_norm(const AfPlan& pl, const float* G, float max_norm, float* words, hipStream_t st) {
  hipLaunchKernelGGL(gn_blocks, dim3(pl.n_blocks), dim3(256), 0, st, pl.blocks, pl.tensors, G, pl.blk_g);
  hipLaunchKernelGGL(gn_finish, dim3(1), dim3(256), 0, st, pl.tensors, pl.n_tensors, pl.blk_g, max_norm, words);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

}  // namespace m2m
