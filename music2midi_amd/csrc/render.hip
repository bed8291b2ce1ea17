// Notes -> audio for gfx950: the packed notes of a batch of clips -> fp32 samples in ONE launch, a wavetable voice.  Stands in for
// ref: webui.py:66 (PrettyMIDI.fluidsynth) and PrettyMIDI.synthesize; the definition is render_host (music2midi_amd/render.py).
// Every sample repeats the definition's steps - integer phase and decay arithmetic, then single rounded fp32 operations - in its
// order, and adds the notes in packed order, so a row is EQUAL to render_host's; nothing in this file may be contracted into a
// fused multiply-add (the pragma below; every product and its sum are separate statements) or reassociated.
//
// One workgroup = one tile of RN_TILE consecutive output samples of one clip (blockIdx.y).  The tile's notes come from a CSR list
// the host builds (tile_start, tile_notes): the loop over them is uniform over the workgroup, so the list entry and the note's
// record are scalar loads and its fields live in scalar registers.  A lane owns RN_PER samples, RN_THREADS apart (coalesced
// stores), and keeps their accumulators in registers; a sample outside the note takes no part (a wave none of whose samples the
// note touches skips the body).  The wavetable row (16 KiB) and the decay table are read through the caches: consecutive samples
// read consecutive or equal entries, and the six rows (98 KiB) stay in L2.  No LDS.
#include "common.h"

#pragma clang fp contract(off)

namespace m2m {
namespace {

constexpr int RN_THREADS = 256;
constexpr int RN_PER = 4;                            // samples per lane; measured against 2 and 8
constexpr int RN_TILE = RN_THREADS * RN_PER;         // samples per workgroup

struct RnVoice {
  const float* wave;
  const float* decay;
  int row;                                           // floats of a wavetable row: table_size + 1
  int shift;                                         // 32 - log2 table_size
  uint32_t mask;                                     // 2^shift - 1
  float scale;                                       // 2^-shift
  int n_tables, J, A, R;
  float invA, invR;
};

// One note's share of output sample n, on <= n < min(off + R, n_samples): the definition's steps 1-4, every operation a statement
// of its own.  W is the note's wavetable row, off is min(nt.off, n_samples).
__device__ inline float rn_sample(const RnVoice& v, const float* __restrict__ W, const m2m_render_note& nt, int off, int n) {
  const uint32_t k = (uint32_t)n - (uint32_t)nt.on;                 // n - on < 2^28 + RN_TILE + 2^31: no wrap
  // 1. phase -> wavetable, linear interpolation
  const uint32_t phase = k * nt.inc;
  const uint32_t i = phase >> v.shift;                               // < table_size; i + 1 is the guard entry at most
  const float fr = (float)(phase & v.mask) * v.scale;
  const float w0 = W[i], w1 = W[i + 1];
  const float dw = w1 - w0;
  const float pw = fr * dw;
  const float w = w0 + pw;
  // 2. decay
  const uint64_t u = (uint64_t)k * (uint64_t)nt.dec;
  const uint64_t j = u >> 16;
  float env;
  if (j >= (uint64_t)v.J) {
    env = v.decay[v.J];
  } else {
    const float ef = (float)(uint32_t)(u & 0xFFFFu) * 1.52587890625e-05f;   // 2^-16
    const float e0 = v.decay[j], e1 = v.decay[j + 1];
    const float de = e1 - e0;
    const float pe = ef * de;
    env = e0 + pe;
  }
  // 3. attack and release
  const int ka = k + 1u < (uint32_t)v.A ? (int)(k + 1u) : v.A;
  const float att = (float)ka * v.invA;
  const float rel = n < off ? 1.0f : (float)(v.R - (n - off)) * v.invR;
  // 4. mix
  const float s0 = w * env;
  const float s1 = s0 * att;
  const float s2 = s1 * rel;
  return s2 * nt.gain;
}

__global__ __launch_bounds__(RN_THREADS) void rn_render_kernel(const m2m_render_note* __restrict__ notes, int n_notes,
                                                               const int32_t* __restrict__ tile_start,
                                                               const int32_t* __restrict__ tile_notes, RnVoice v,
                                                               float* __restrict__ out, int n_samples, int64_t row_stride) {
  const int64_t slot = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int e0 = tile_start[slot], e1 = tile_start[slot + 1];        // uniform
  const int n0 = (int)blockIdx.x * RN_TILE + (int)threadIdx.x;       // < 2^28 + RN_TILE
  float acc[RN_PER];
#pragma unroll
  for (int r = 0; r < RN_PER; ++r) acc[r] = 0.0f;
  for (int e = e0; e < e1; ++e) {
    int idx = tile_notes[e];
    idx = idx < 0 ? 0 : (idx > n_notes - 1 ? n_notes - 1 : idx);    // e0 < e1 only with n_notes >= 1 (the host refuses otherwise)
    const m2m_render_note nt = notes[idx];                           // uniform: scalar registers
    int table = nt.table;
    table = table < 0 ? 0 : (table > v.n_tables - 1 ? v.n_tables - 1 : table);
    const float* W = v.wave + (int64_t)table * v.row;
    const int off = nt.off < n_samples ? nt.off : n_samples;        // off + R below 2^28 + 2^24
    const int end = off + v.R < n_samples ? off + v.R : n_samples;
#pragma unroll
    for (int r = 0; r < RN_PER; ++r) {
      const int n = n0 + r * RN_THREADS;
      if (n >= nt.on && n < end) {
        const float s = rn_sample(v, W, nt, off, n);
        acc[r] = acc[r] + s;
      }
    }
  }
  float* row = out + (int64_t)blockIdx.y * row_stride;
#pragma unroll
  for (int r = 0; r < RN_PER; ++r) {
    const int n = n0 + r * RN_THREADS;
    if (n < n_samples) row[n] = acc[r];
  }
}

}  // namespace
}  // namespace m2m

// ------------------------------------------------------------------ C ABI ---
using namespace m2m;

extern "C" int m2m_render_tile(void) { return RN_TILE; }

extern "C" int m2m_render_notes_f32(const m2m_render_note* notes_dev, int n_notes, const int32_t* tile_start_dev,
                                    const int32_t* tile_notes_dev, int64_t n_entries, const m2m_render_voice* voice, float* out_dev,
                                    int64_t n_samples, int64_t row_stride, int n_clips, void* stream) {
  // every refusal is made on the arguments alone, before the first HIP call
  M2M_REQUIRE(n_samples >= 1 && n_samples <= M2M_RENDER_MAX_SAMPLES, "m2m_render_notes_f32: n_samples = %lld out of range (1..%d)",
              (long long)n_samples, M2M_RENDER_MAX_SAMPLES);
  M2M_REQUIRE(n_clips >= 1 && n_clips <= M2M_RENDER_MAX_CLIPS, "m2m_render_notes_f32: %d clips out of range (1..%d)", n_clips,
              M2M_RENDER_MAX_CLIPS);
  M2M_REQUIRE(n_notes >= 0 && n_notes <= M2M_RENDER_MAX_NOTES, "m2m_render_notes_f32: %d notes out of range (0..%d)", n_notes,
              M2M_RENDER_MAX_NOTES);
  M2M_REQUIRE(n_entries >= 0 && n_entries <= 0x7FFFFFFFll && (n_entries == 0 || n_notes > 0),
              "m2m_render_notes_f32: %lld list entries for %d notes (0..2^31 - 1, none without notes)", (long long)n_entries, n_notes);
  M2M_REQUIRE(row_stride >= n_samples, "m2m_render_notes_f32: row_stride %lld below n_samples = %lld", (long long)row_stride,
              (long long)n_samples);
  M2M_REQUIRE(voice && tile_start_dev && out_dev, "m2m_render_notes_f32: null voice / tile starts / output");
  M2M_REQUIRE(n_notes == 0 || (notes_dev && tile_notes_dev), "m2m_render_notes_f32: null notes / tile list with %d notes", n_notes);
  M2M_REQUIRE(voice->wave_dev && voice->decay_dev, "m2m_render_notes_f32: null wavetables / decay table");
  M2M_REQUIRE(((uintptr_t)notes_dev | (uintptr_t)tile_start_dev | (uintptr_t)tile_notes_dev | (uintptr_t)out_dev |
               (uintptr_t)voice->wave_dev | (uintptr_t)voice->decay_dev) % 4 == 0,
              "m2m_render_notes_f32: a pointer is not 4-byte aligned");
  M2M_REQUIRE(voice->attack >= 1 && voice->attack <= M2M_RENDER_MAX_RAMP && voice->release >= 1 && voice->release <= M2M_RENDER_MAX_RAMP,
              "m2m_render_notes_f32: attack / release = %d / %d samples out of range (1..%d)", voice->attack, voice->release,
              M2M_RENDER_MAX_RAMP);
  int bits = 0;
  while (bits < 31 && (1 << bits) < voice->table_size) ++bits;
  M2M_REQUIRE(voice->table_size == (1 << bits) && bits >= 8 && bits <= 16,
              "m2m_render_notes_f32: table_size = %d is not a power of two in 256..65536", voice->table_size);
  M2M_REQUIRE(voice->n_tables >= 1 && voice->n_tables <= 64, "m2m_render_notes_f32: %d wavetables out of range (1..64)", voice->n_tables);
  M2M_REQUIRE(voice->decay_steps >= 1 && voice->decay_steps <= M2M_RENDER_MAX_RAMP, "m2m_render_notes_f32: %d decay steps out of range (1..%d)",
              voice->decay_steps, M2M_RENDER_MAX_RAMP);
  M2M_REQUIRE(voice->reserved == 0, "m2m_render_notes_f32: reserved = %d", voice->reserved);
  RnVoice v;
  v.wave = voice->wave_dev;
  v.decay = voice->decay_dev;
  v.row = voice->table_size + 1;
  v.shift = 32 - bits;
  v.mask = (1u << v.shift) - 1u;
  v.scale = 1.0f / (float)(1u << v.shift);             // a power of two: exact
  v.n_tables = voice->n_tables;
  v.J = voice->decay_steps;
  v.A = voice->attack;
  v.R = voice->release;
  v.invA = 1.0f / (float)voice->attack;                // one rounded division each, as the definition's
  v.invR = 1.0f / (float)voice->release;
  const dim3 grid((unsigned)((n_samples + RN_TILE - 1) / RN_TILE), (unsigned)n_clips), block(RN_THREADS);
  hipLaunchKernelGGL(rn_render_kernel, grid, block, 0, (hipStream_t)stream, notes_dev, n_notes, tile_start_dev, tile_notes_dev, v, out_dev,
                     (int)n_samples, row_stride);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}
