// What the audio ingest (ingest.hip) and the dataset crop (dataset.hip) share: the conversion of one WAVE sample as audio.read_wav
// converts it, and the host checks both make on their arguments.  Included AFTER the includer's `#pragma clang fp contract(off)`:
// nothing here may be contracted into a fused multiply-add.
#pragma once
#include "common.h"

namespace m2m {
namespace {

// little-endian loads; `aligned`: the address is a multiple of the width
__device__ inline uint32_t ig_ld16(const unsigned char* p, bool aligned) {
  if (aligned) return *reinterpret_cast<const uint16_t*>(p);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8);
}
__device__ inline uint32_t ig_ld32(const unsigned char* p, bool aligned) {
  if (aligned) return *reinterpret_cast<const uint32_t*>(p);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ inline uint64_t ig_ld64(const unsigned char* p, bool aligned) {
  if (aligned) return *reinterpret_cast<const uint64_t*>(p);
  return (uint64_t)ig_ld32(p, false) | ((uint64_t)ig_ld32(p + 4, false) << 32);
}

__host__ __device__ inline int ig_width(int format) {
  switch (format) {
    case M2M_PCM_U8: return 1;
    case M2M_PCM_S16: return 2;
    case M2M_PCM_S24: return 3;
    case M2M_PCM_S32: return 4;
    case M2M_PCM_F32: return 4;
    case M2M_PCM_F64: return 8;
    default: return 0;
  }
}

// one sample as audio.read_wav converts it
template <int FORMAT>
__device__ inline float ig_sample(const unsigned char* p, bool aligned) {
  if constexpr (FORMAT == M2M_PCM_U8) {
    return ((float)p[0] - 128.0f) / 128.0f;
  } else if constexpr (FORMAT == M2M_PCM_S16) {
    return (float)(int16_t)ig_ld16(p, aligned) / 32768.0f;
  } else if constexpr (FORMAT == M2M_PCM_S24) {
    int32_t v = (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16));
    if (v & 0x800000) v -= 0x1000000;
    return (float)v / 8388608.0f;
  } else if constexpr (FORMAT == M2M_PCM_S32) {
    return (float)((double)(int32_t)ig_ld32(p, aligned) / 2147483648.0);
  } else if constexpr (FORMAT == M2M_PCM_F32) {
    return __builtin_bit_cast(float, ig_ld32(p, aligned));
  } else {
    return (float)__builtin_bit_cast(double, ig_ld64(p, aligned));
  }
}

// one frame as load_audio's y.mean(axis=1) averages it below 8 channels: the samples summed in channel order in fp32 from +0
// (numpy's reduction starts there: a frame of -0 samples sums to +0), then divided by the fp32 channel count
template <int FORMAT>
__device__ inline float ig_frame(const unsigned char* p, int channels, bool aligned) {
  constexpr int width = FORMAT == M2M_PCM_U8 ? 1 : FORMAT == M2M_PCM_S16 ? 2 : FORMAT == M2M_PCM_S24 ? 3 : FORMAT == M2M_PCM_F64 ? 8 : 4;
  float sum = 0.0f;
  for (int c = 0; c < channels; ++c) sum = sum + ig_sample<FORMAT>(p + c * width, aligned);
  return sum / (float)channels;
}

inline bool ig_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

inline int ig_gcd(int a, int b) {
  while (b) { const int t = a % b; a = b; b = t; }
  return a;
}

}  // namespace
}  // namespace m2m
