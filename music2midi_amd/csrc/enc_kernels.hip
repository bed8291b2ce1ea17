// Encoder-side row kernels (one shot per clip batch): RMSNorm and the embedding gather.  The MFMA GEMM family is in
// enc_gemm.hip, the flash-style attention in enc_attn.hip.  Together they replace the HF T5 encoder stack that
// ref: music2midi/transformer.py:44 runs once per generate() (hf: models/t5/modeling_t5.py:663-750), and the
// cross-attention K/V projections (hf: :319-332) for all decoder layers in one GEMM.
//
// RMSNorm is templated on the storage type T of the precision mode: float (parity mode) or bf16 (throughput mode).
#include "mma.h"
#include "rms.h"
#include "t5.h"

namespace m2m {

// ============================================================== RMSNorm ====
// One wave per row: y = x * rsqrt(mean(x^2) + eps) * w   (hf: modeling_t5.py:59-72), fp32 math,
// output in storage type T (GEMM input) and/or fp32.  (rms_sumsq4: rms.h, shared to the bit with norm_gemm_kernel.)
template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                      T* __restrict__ outT, float* __restrict__ outF, int M, int d,
                                                      float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* xr = x + (int64_t)row * d;
  float ss = 0.f;
  for (int c = lane * 4; c < d; c += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + c);
    ss = ss + rms_sumsq4(v);
  }
  ss = wave_sum(ss);
  const float rstd = rsqrtf(ss / (float)d + eps);
  for (int c = lane * 4; c < d; c += 256) {
    const float4 v = *reinterpret_cast<const float4*>(xr + c);
    const float4 g = *reinterpret_cast<const float4*>(w + c);
    const float y0 = g.x * (v.x * rstd), y1 = g.y * (v.y * rstd), y2 = g.z * (v.z * rstd), y3 = g.w * (v.w * rstd);
    if (outT) {
      T* o = outT + (int64_t)row * d + c;
      o[0] = from_f32<T>(y0); o[1] = from_f32<T>(y1); o[2] = from_f32<T>(y2); o[3] = from_f32<T>(y3);
    }
    if (outF) *reinterpret_cast<float4*>(outF + (int64_t)row * d + c) = make_float4(y0, y1, y2, y3);
  }
}

int launch_rmsnorm(int precision, const float* x, const float* w, void* out, int M, int d, float eps, hipStream_t st) {
  M2M_REQUIRE(d % 4 == 0, "rmsnorm: d_model must be a multiple of 4");
  dim3 grid((unsigned)ceil_div(M, 4));
  if (precision == M2M_PREC_BF16)
    hipLaunchKernelGGL(rmsnorm_kernel<bf16_t>, grid, dim3(256), 0, st, x, w, (bf16_t*)out, (float*)nullptr, M, d, eps);
  else
    hipLaunchKernelGGL(rmsnorm_kernel<float>, grid, dim3(256), 0, st, x, w, (float*)out, (float*)nullptr, M, d, eps);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

int launch_final_norm_f32(const float* x, const float* w, float* out_f32, void* out_T, int precision, int M, int d,
                          float eps, hipStream_t st) {
  dim3 grid((unsigned)ceil_div(M, 4));
  if (precision == M2M_PREC_BF16)
    hipLaunchKernelGGL(rmsnorm_kernel<bf16_t>, grid, dim3(256), 0, st, x, w, (bf16_t*)out_T, out_f32, M, d, eps);
  else
    hipLaunchKernelGGL(rmsnorm_kernel<float>, grid, dim3(256), 0, st, x, w, (float*)out_T, out_f32, M, d, eps);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

// ====================================================== embedding rows ====
// x[row][:] = table[ids[row]][:]  (decoder input embedding of the teacher-forced pass, fp32 residual stream)
__global__ __launch_bounds__(256) void embed_rows_kernel(const int64_t* __restrict__ ids, const float* __restrict__ table,
                                                        float* __restrict__ x, int M, int d, int V, int pad_id) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;
  int tok = (int)ids[row];
  if (tok < 0 || tok >= V) tok = pad_id;
  for (int c = lane * 4; c < d; c += 256)
    *reinterpret_cast<float4*>(x + (int64_t)row * d + c) = *reinterpret_cast<const float4*>(table + (int64_t)tok * d + c);
}

int launch_embed_rows(const int64_t* ids, const float* table, float* x, int M, int d, int V, int pad_id, hipStream_t st) {
  hipLaunchKernelGGL(embed_rows_kernel, dim3((unsigned)ceil_div(M, 4)), dim3(256), 0, st, ids, table, x, M, d, V, pad_id);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

}  // namespace m2m
