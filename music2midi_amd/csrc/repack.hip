// Weight repacking kernels: fp32 HuggingFace-layout tensors -> kernel layouts in the
// storage type of the precision mode (fp32 or bf16).  Run once in m2m_model_create.
#include "t5.h"

namespace m2m {

template <typename T>
__global__ void convert_kernel(const float* __restrict__ src, T* __restrict__ dst, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = from_f32<T>(src[i]);
}

// dst rows: for chunk c: [c*2*half, +half) = wi0 rows [c*half, +half); next half rows = wi1 rows [c*half, +half)
template <typename T>
__global__ void interleave_kernel(const float* __restrict__ wi0, const float* __restrict__ wi1,
                                  T* __restrict__ dst, int dff, int d, int half) {
  const int64_t n = (int64_t)2 * dff * d;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    const int row = (int)(i / d), col = (int)(i - (int64_t)row * d);
    const int c = row / (2 * half), r = row - c * 2 * half;
    const float* src = (r < half) ? wi0 : wi1;
    const int srow = c * half + (r < half ? r : r - half);
    dst[i] = from_f32<T>(src[(int64_t)srow * d + col]);
  }
}

static inline int grid_for(int64_t n) {
  int64_t g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

int launch_convert(int precision, const float* src, void* dst, int64_t n, hipStream_t st) {
  if (precision == M2M_PREC_BF16)
    hipLaunchKernelGGL(convert_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st, src, (bf16_t*)dst, n);
  else
    hipLaunchKernelGGL(convert_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, src, (float*)dst, n);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

int launch_interleave(int precision, const float* wi0, const float* wi1, void* dst, int dff, int d, int half,
                      hipStream_t st) {
  const int64_t n = (int64_t)2 * dff * d;
  if (precision == M2M_PREC_BF16)
    hipLaunchKernelGGL(interleave_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st, wi0, wi1, (bf16_t*)dst, dff, d, half);
  else
    hipLaunchKernelGGL(interleave_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, wi0, wi1, (float*)dst, dff, d, half);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

// Feed-forward step image (t5.h DecLayerPacked::ff_img): a permutation of the CONVERTED wi (16-row interleave) and wo_ff in 16-byte
// chunks, no second rounding.  Chunk i of the image = lane i % 64 of load instruction i / 64; a fragment is 16 / sizeof(T) / 2
// such instructions (bf16: one; fp32: the lanes' elements 0..3, then their elements 4..7).
template <typename T>
__global__ void ff_image_kernel(const T* __restrict__ wi, const T* __restrict__ wo, T* __restrict__ img, int dff, int d) {
  constexpr int EPC = 16 / (int)sizeof(T), HPF = 8 / EPC;     // elements per chunk, chunks per lane and fragment
  const int KS = d / 64;
  const int64_t n = (int64_t)3 * dff * d / EPC;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int lane = (int)(i & 63), r = lane & 15, g = lane >> 4;
    int64_t q = i >> 6;
    const int half = (int)(q % HPF); q /= HPF;
    const int f = (int)(q % 12); q /= 12;
    const int ks = (int)(q % KS), c = (int)(q / KS);
    const T* src = f < 8 ? wi + (int64_t)(64 * c + 16 * (f >> 1) + r) * d + 64 * ks + 32 * (f & 1) + 8 * g
                         : wo + (int64_t)(16 * (4 * ks + f - 8) + r) * dff + 32 * c + 8 * g;
    reinterpret_cast<uint4*>(img)[i] = *reinterpret_cast<const uint4*>(src + EPC * half);
  }
}

int launch_ff_image(int precision, const void* wi, const void* wo_ff, void* img, int dff, int d, hipStream_t st) {
  const int64_t n = (int64_t)3 * dff * d / (precision == M2M_PREC_BF16 ? 8 : 4);
  if (precision == M2M_PREC_BF16)
    hipLaunchKernelGGL(ff_image_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st, (const bf16_t*)wi, (const bf16_t*)wo_ff, (bf16_t*)img, dff, d);
  else
    hipLaunchKernelGGL(ff_image_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, (const float*)wi, (const float*)wo_ff, (float*)img, dff, d);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

// Attention output-projection step image (t5.h DecLayerPacked::wo_img / wco_img): a permutation of the CONVERTED [d, H * 64] matrix
// in 16-byte chunks.  Chunk i = thread i % 2d of load instruction (i / 2d) % (32 / E) of head i / (2d * 32 / E).
template <typename T>
__global__ void attn_out_image_kernel(const T* __restrict__ wo, T* __restrict__ img, int H, int d) {
  constexpr int E = 16 / (int)sizeof(T), OCH = 32 / E;
  const int64_t n = (int64_t)H * OCH * 2 * d;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int tid = (int)(i % (2 * d)), u = (int)((i / (2 * d)) % OCH), h = (int)(i / ((int64_t)2 * d * OCH));
    reinterpret_cast<uint4*>(img)[i] = *reinterpret_cast<const uint4*>(wo + (int64_t)(tid >> 1) * (H * 64) + 64 * h + 32 * (tid & 1) + E * u);
  }
}

int launch_attn_out_image(int precision, const void* wo, void* img, int H, int d, hipStream_t st) {
  const int64_t n = (int64_t)H * 64 * d / (precision == M2M_PREC_BF16 ? 8 : 4);
  if (precision == M2M_PREC_BF16)
    hipLaunchKernelGGL(attn_out_image_kernel<bf16_t>, dim3(grid_for(n)), dim3(256), 0, st, (const bf16_t*)wo, (bf16_t*)img, H, d);
  else
    hipLaunchKernelGGL(attn_out_image_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, (const float*)wo, (float*)img, H, d);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

// 64-bit position-weighted checksum of a device buffer (32-bit words w_i): sum of w_i * (2 i + 1) mod 2^64.  Integer adds in any
// order give the same value, so it is reproducible; the odd multipliers make it sensitive to WHERE a word sits, not only to the
// multiset of words.  Used after the multi-GPU weight broadcast: every rank's repacked weights must be the same bytes.
__global__ __launch_bounds__(256) void checksum_kernel(const uint32_t* __restrict__ w, int64_t n, unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long part[4];
  unsigned long long s = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    s += (unsigned long long)w[i] * (unsigned long long)(2 * i + 1);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(acc, part[0] + part[1] + part[2] + part[3]);
}

int launch_checksum(const void* buf, int64_t bytes, unsigned long long* acc_dev, hipStream_t st) {
  const int64_t n = bytes / 4;
  hipLaunchKernelGGL(checksum_kernel, dim3(grid_for(n)), dim3(256), 0, st, (const uint32_t*)buf, n, acc_dev);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

int launch_copy_f32(const float* src, float* dst, int64_t n, hipStream_t st) {
  M2M_CHECK_HIP(hipMemcpyAsync(dst, src, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
  return M2M_OK;
}

int launch_fill_zero(void* dst, int64_t bytes, hipStream_t st) {
  M2M_CHECK_HIP(hipMemsetAsync(dst, 0, (size_t)bytes, st));
  return M2M_OK;
}

}  // namespace m2m
