// Decoder-side kernels: the KV-cached greedy step.  Replaces the per-token loop of HF
// generate() that ref: music2midi/transformer.py:44 drives (hf: generation/utils.py:2876-2937,
// one T5 decoder forward hf: models/t5/modeling_t5.py:448-509,1031-1047 per token, ~60 vendor
// kernel launches and a host sync each).  Here a step is a fixed sequence of kernels that read
// the step index from device memory, so the whole loop replays captured hipGraphs with no
// host round trip; finished-row bookkeeping (pad after EOS) lives in device memory.
//
// Clips are independent, so a batch is decoded as several independent CHAINS ("views": a
// contiguous range of clips with its own step counter, stream and graph).  One chain's kernels
// are latency-bound (12..72 workgroups each); running several chains side by side fills the
// 256 CUs and overlaps one chain's HBM-bound attention with another chain's projections.
//
//   dec_attn_kernel  one (clip, head) per 1024-thread workgroup: RMSNorm + that head's projection
//                    (self: q,k,v + cache append; cross: q) fused in front of the attention, which
//                    streams K then V straight from HBM to registers (16 B per lane per load, no
//                    LDS staging: each byte is used once), fp32 softmax, shuffle + LDS reduction.
//   dec_attn_mc_kernel  the same for large chains: one head of C = 2 / 4 consecutive clips per workgroup (one row round trip, the
//                    head's weights fetched once, the clips' K/V streams back to back).  This step's k / v rows go through dec_attn_kernel's
//                    da_project + da_append_kv; the other pieces (q, DaSoftmax, da_merge, da_out_row, da_book_row) it repeats by hand
//                    (DESIGN 9.7): a row's bits do not depend on the form.
//   dec_ff_kernel    the whole gated feed-forward sub-layer: RMSNorm + MFMA up projection of a 32-column
//                    slice + gated GELU (LDS) + MFMA down projection, added into the residual stream.
//   dec_ff_multi_kernel  the same for large chains: several consecutive slices per workgroup, summed as integers before ONE
//                    atomic per element.  Both are thin wrappers over one body, dec_ff_body.
//   dec_gemm_kernel  lm_head: RMSNorm + skinny projection, one 16x16 MFMA tile per workgroup, waves split K.
//   dec_head_kernel  argmax / EOS+pad bookkeeping / next-token embedding / step counter.
#include "mma.h"
#include "t5.h"

#include <stdlib.h>
#include <type_traits>

namespace m2m {

// ---- optional in-kernel wall-clock stamps (diagnostic builds only: -DM2M_STAMPS) ----
// s_memrealtime runs at a constant 100 MHz and is the same clock on every CU, so stamps from
// different kernels can be laid on one timeline.  Block 0 / thread 0 of every decode kernel logs
// {kernel id, phase, ticks}.  Never compiled into the product library.
#ifdef M2M_STAMPS
__device__ unsigned long long g_stamps[1 << 18];
__device__ unsigned int g_stamp_n;
// phase 0 claims 8 consecutive slots with ONE returning atomic (its round trip is paid at kernel
// entry, before anything is timed); later phases are fire-and-forget stores into the claimed slots.
#define M2M_STAMP(kid, phase)                                                                   \
  do {                                                                                          \
    if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) {                               \
      static_assert((phase) < 8, "phase");                                                      \
      if ((phase) == 0) m2m_stamp_base = atomicAdd(&g_stamp_n, 8u);                             \
      const unsigned long long tk = __builtin_amdgcn_s_memrealtime();                           \
      if (m2m_stamp_base + 8 <= (1u << 18))                                                     \
        g_stamps[m2m_stamp_base + (phase)] = ((unsigned long long)(kid) << 56) | ((unsigned long long)(phase) << 48) | (tk & 0xFFFFFFFFFFFFull); \
    }                                                                                           \
  } while (0)
#define M2M_STAMP_DECL unsigned int m2m_stamp_base = 0; (void)m2m_stamp_base;
#else
#define M2M_STAMP(kid, phase) do {} while (0)
#define M2M_STAMP_DECL
#endif

// ---- decoder residual stream: int64 fixed point (scale 2^30) ----
// The output projections of the attention sub-layers are accumulated per head straight from the
// attention kernels (8 workgroups per clip add into the same row).  Float atomics would make the
// sum depend on arrival order; integer adds are associative, so the result is bit-reproducible
// whatever the order, and exact (2^-30 resolution, +-8.6e9 range) where fp32 would round.
//
// The stream lives in THREE buffers that rotate (A -> B -> C -> A): an attention kernel READS the
// complete row from one buffer and ACCUMULATES residual + per-head projections into the next one,
// which the kernel before it left zeroed, and zeroes the third.  A workgroup that starts late
// (more workgroups than CUs) therefore never reads a row that a finished sibling has already
// added to, which a single read-modify buffer would allow.
typedef long long xq_t;
// float -> fixed point, round to nearest even: (double)v * 2^30 is exact, adding 1.5 * 2^52 leaves the rounded
// integer in the low mantissa bits (two's complement), so the conversion is cvt + mul + add + a 64-bit subtract
// instead of the ~14-instruction float -> int64 sequence.  Valid for |v| < 2^21.
__device__ inline xq_t xq_fix(float v) {
  const double m = (double)v * 1073741824.0 + 6755399441055744.0;
  return __double_as_longlong(m) - 0x4338000000000000ll;
}
// The same conversion with the range guarded: a value the magic-number add cannot represent (|v| >= 2^21, Inf,
// NaN - a corrupt checkpoint, a diverged fine-tune) would otherwise become an arbitrary integer and the decoder
// would go on emitting plausible-looking ids where the reference produces NaN logits.  Such a value is clamped
// (NaN -> 0) and a sticky flag is raised in the chain's DecState; m2m_generate_greedy / m2m_decode_forced return
// M2M_ERR_RANGE when they find it.  One compare per conversion; the store happens only on the failure path.
constexpr float XQ_LIMIT = 2097152.0f;   // 2^21
__device__ inline xq_t xq_fix_guarded(float v, DecState* st) {
  if (!(fabsf(v) < XQ_LIMIT)) {          // also true for NaN
    st->overflow = 1;
    v = (v != v) ? 0.f : copysignf(XQ_LIMIT - 1.0f, v);
  }
  return xq_fix(v);
}
// via double: int64 -> f64 is 4 instructions (two 32-bit converts + fma) against ~12 for the correctly
// rounded int64 -> f32 sequence, and the result is the same single rounding while |q| < 2^53 (|x| < 8.4e6)
__device__ inline float xq_flt(xq_t q) { return (float)((double)q * (1.0 / 1073741824.0)); }
__device__ inline float4 xq_load4(const xq_t* p) {   // p 16-byte aligned
  const longlong2 a = *reinterpret_cast<const longlong2*>(p);
  const longlong2 b = *reinterpret_cast<const longlong2*>(p + 2);
  return make_float4(xq_flt(a.x), xq_flt(a.y), xq_flt(b.x), xq_flt(b.y));
}

// ---- residual rows of an MFMA tile, staged through LDS (dec_ff_kernel and dec_gemm_kernel) ----
// The MFMA operand pattern gives lane (r, g) 64-byte pieces of row r: read from memory that way, one wave instruction touches
// 32 different 128-byte lines, uses a quarter of each, and every line is asked for by four instructions - and these are the loads
// the kernel's first barrier waits for.  Instead the block loads its rows cooperatively as raw fixed-point words, 16 bytes per
// lane with consecutive lanes on consecutive addresses (a wave instruction = 1 KB of one row, whole lines), in front of every
// other request (loads retire in order), stores them to LDS, and each lane reads back exactly the 16 elements it used to read
// from memory: the conversions and every sum see the same values in the same order.  Same-box A/B against the earlier form
// (DESIGN 4.3): dec_ff_kernel 7.03 -> 6.61 us per launch, lm_head 4.91 -> 4.87 us at 16 clips and 5.27 -> 4.90 at 64;
// dec_ff_multi_kernel gained 1.6 %, inside the run-to-run spread, and reads its rows from memory as before.
// Place, in 16-byte chunks, of chunk cc of tile row r (< 16) in an image of cpr chunks per row (cpr a multiple of 16, so rows
// start on a 256-byte bank row).  Lane (r, g) reads chunks base + 4 g + q: the XOR with the row's two halves swapped keeps the
// four 16-lane groups of a 16-byte LDS read on 16 different bank slots (a group holds lanes whose r >> 2 differ wherever their g
// differs), and the 8 consecutive lanes of a 16-byte LDS write stay on 8 different slots.
typedef long long xq2_t __attribute__((ext_vector_type(2)));   // one 16-byte chunk of a row (a plain vector: it stays in registers)
__device__ inline int row_stage_at(int r, int cc, int cpr) { return r * cpr + (cc ^ (((r & 3) << 2) | (r >> 2))); }

// ---- headless greedy loop: the arg-max travels as a packed 64-bit key ----
// The lm_head workgroups reduce their 16 columns per row and atomicMax a key into keys[row]; the NEXT step's layer-0
// self-attention workgroups decode it (token id -> embedding row = their input), the layer-0 cross-attention kernel
// does the per-row bookkeeping (token matrix, finished flag, unfinished count) and clears the key, the layer-0
// feed-forward kernel turns "no row unfinished" into done.  That removes dec_head_kernel (a kernel boundary + two
// dependent memory round trips per step) from the greedy chain; teacher forcing keeps the head kernel.
// key = (order-preserving image of the fp32 logit) << 32 | (0xFFFFFFFF - column): the largest key is the largest logit,
// ties go to the lowest column (torch.argmax); 0 = "no key".
__device__ inline unsigned long long amax_key(float v, int col) {
  unsigned int u = __float_as_uint(v + 0.0f);                      // -0 -> +0: they must tie
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)col);
}
__device__ inline int amax_key_token(unsigned long long key, int fin, int V, int pad_id) {
  int tok = (int)(0xFFFFFFFFu - (unsigned int)(key & 0xFFFFFFFFull));
  if (fin || tok < 0 || tok >= V) tok = pad_id;                    // finished rows keep emitting pad (hf generation/utils.py:2929)
  return tok;
}
// every kernel of a step: the chain is over when done is set OR the step counter has reached the step budget
__device__ inline int chain_done(const DecState* st) { return st->done | (st->t >= st->max_steps); }

// ===================================================== skinny projection ====
// lm_head: logits[B, V] = RMSNorm(x) . W^T (untied, no d_model**-0.5 scaling: transformers 4.34 semantics).
struct DecGemmArgs {
  const xq_t* x;         // [rows, K] fixed-point residual stream
  int ldx;
  const float* ln_w;     // [K] RMSNorm weight
  float eps;
  const void* W;         // [Npad, K] T
  int K, N, B;
  DecState* state;
  float* out;            // [B, ldo] logits
  int ldo;
  unsigned long long* keys;   // headless greedy loop: [B] arg-max keys (the logits themselves are not stored)
};

// One 16-row x 16-column output tile per workgroup (MFMA 16x16x32 / 16x16x4), NW waves split K.
// A CU fetches only ~25 GB/s from beyond its L2 and every kernel starts cold for what the previous
// one wrote, so a skinny projection's time IS the bytes one workgroup pulls: small tiles spread W (and
// the rows of x) over many CUs.  Every global load (weights, activations, norm weights) is issued
// before the first use, so a launch is one memory round trip; RMSNorm statistics are reduced across
// waves through LDS while the weight loads are in flight; the cross-wave sum has a fixed order.
//
// NS (32-wide k-steps per wave) is a template parameter: a runtime bound would put every load of
// the unrolled batch behind its own branch + s_waitcnt (cdna_hip_programming.md, "three .s-level
// traps" item c).  blockDim.x = 64 * NW with NW = K / (32 * NS) <= 12.
typedef float f32x4_t __attribute__((ext_vector_type(4)));
constexpr int DG_MAXW = 12;

__device__ inline void mma32_16(f32x4_t& acc, const Frag<bf16_t>& a, const Frag<bf16_t>& b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a.v), __builtin_bit_cast(bf16x8_t, b.v),
                                                acc, 0, 0, 0);
}
// fp32: lane (r, g) holds k = 8g + j, j = 0..7; MFMA j sums the four lane groups -> k in {j, 8+j, 16+j, 24+j}
__device__ inline void mma32_16(f32x4_t& acc, const Frag<float>& a, const Frag<float>& b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo.x, b.lo.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo.y, b.lo.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo.z, b.lo.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.lo.w, b.lo.w, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi.x, b.hi.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi.y, b.hi.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi.z, b.hi.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.hi.w, b.hi.w, acc, 0, 0, 0);
}

template <typename T, int NS, bool HEADLESS>
__global__ __launch_bounds__(64 * DG_MAXW) void dec_gemm_kernel(DecGemmArgs a) {
  M2M_STAMP_DECL
  __shared__ float ss_s[DG_MAXW][16];
  __shared__ float red[DG_MAXW][16 * 17];
  M2M_STAMP(2, 0);
  // headless: "live" comes from done and the STABLE copy of t (this kernel advances t itself at its end)
  const int t_cur = HEADLESS ? a.state->t_copy : 0;
  const int done = HEADLESS ? (a.state->done | (t_cur >= a.state->max_steps)) : chain_done(a.state);   // consumed only before the stores
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nw = blockDim.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int b0 = blockIdx.y * 16;
  const int K = a.K;
  const T* W = reinterpret_cast<const T*>(a.W);
  const int kbeg = wave * (32 * NS) + 8 * g;
  const bool row_ok = (b0 + r) < a.B;
  const T* wr = W + (int64_t)(n0 + r) * K + kbeg;
  // epilogue coordinates of this thread (threads 0..255 own one output each)
  const int orow = (tid >> 4) & 15, ocol = tid & 15;
  const int ob = b0 + orow, on = n0 + ocol;

  // the tile's rows first (row_stage_at above): a pass of the block's 64 nw lanes covers RPI = 4 / NS rows, thread tid takes chunk
  // scc of tile rows srow, srow + RPI, ...; rows past the batch re-read its last row (clamped, never a branch around a load)
  constexpr int RPI = 4 / NS, NXL = 4 * NS;
  __shared__ __align__(16) xq2_t xs[16 * (NS == 1 ? 64 : 256)];   // K <= 128 (NS = 1) / 512: dec_gemm_shape
  const int cpr = K >> 1;                                             // 16-byte chunks per row
  int srow = 0;
#pragma unroll
  for (int i = 1; i < RPI; ++i) srow += tid >= i * cpr ? 1 : 0;
  const int scc = tid - srow * cpr;
  xq2_t xst[NXL];
#pragma unroll
  for (int i = 0; i < NXL; ++i)
    xst[i] = *reinterpret_cast<const xq2_t*>(a.x + (int64_t)min(b0 + RPI * i + srow, a.B - 1) * a.ldx + 2 * scc);
  __builtin_amdgcn_sched_barrier(0);               // the latency-critical rows go out FIRST (loads retire in order)
  float4 g0[NS], g1[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    g0[s] = *reinterpret_cast<const float4*>(a.ln_w + kbeg + 32 * s);
    g1[s] = *reinterpret_cast<const float4*>(a.ln_w + kbeg + 32 * s + 4);
  }
  Frag<T> wf[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) wf[s] = load_frag(wr + 32 * s);
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::"s"(done));   // materialise the flag now, under the vector loads (else it is sunk to the epilogue)
#pragma unroll
  for (int i = 0; i < NXL; ++i) xs[row_stage_at(RPI * i + srow, scc, cpr)] = xst[i];
  __syncthreads();

  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  {
    float4 x0[NS], x1[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {   // lane (r, g): elements kbeg + 32 s + [0, 8) of row r (padding rows hold the last row: rs = 0 below)
      const int cc = (kbeg >> 1) + 16 * s;
      const xq2_t q0 = xs[row_stage_at(r, cc, cpr)], q1 = xs[row_stage_at(r, cc + 1, cpr)];
      const xq2_t q2 = xs[row_stage_at(r, cc + 2, cpr)], q3 = xs[row_stage_at(r, cc + 3, cpr)];
      x0[s] = make_float4(xq_flt(q0.x), xq_flt(q0.y), xq_flt(q1.x), xq_flt(q1.y));
      x1[s] = make_float4(xq_flt(q2.x), xq_flt(q2.y), xq_flt(q3.x), xq_flt(q3.y));
    }
    float ss = 0.f;
#pragma unroll
    for (int s = 0; s < NS; ++s)
      ss += x0[s].x * x0[s].x + x0[s].y * x0[s].y + x0[s].z * x0[s].z + x0[s].w * x0[s].w +
            x1[s].x * x1[s].x + x1[s].y * x1[s].y + x1[s].z * x1[s].z + x1[s].w * x1[s].w;
    ss += lane_xor<16>(ss);
    ss += lane_xor<32>(ss);
    if (g == 0) ss_s[wave][r] = ss;
    __syncthreads();
    float tot = 0.f;
    for (int w = 0; w < nw; ++w) tot += ss_s[w][r];
    const float rs = row_ok ? rsqrtf(tot / (float)K + a.eps) : 0.f;   // rs = 0 zeroes the padding rows
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const float xv[8] = {g0[s].x * (x0[s].x * rs), g0[s].y * (x0[s].y * rs), g0[s].z * (x0[s].z * rs),
                           g0[s].w * (x0[s].w * rs), g1[s].x * (x1[s].x * rs), g1[s].y * (x1[s].y * rs),
                           g1[s].z * (x1[s].z * rs), g1[s].w * (x1[s].w * rs)};
      const Frag<T> fa = pack_frag<T>(xv);
      mma32_16(acc, fa, wf[s]);
    }
  }
  // ---- cross-wave reduction (fixed order: deterministic).  acc[i]: row 4g + i, column r ----
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wave][(4 * g + i) * 17 + r] = acc[i];
  M2M_STAMP(2, 1);
  __syncthreads();
  if constexpr (HEADLESS) {
    if (done || tid >= 256) return;                     // (wave-uniform: waves 0-3 hold the 256 outputs)
    const int idx = orow * 17 + ocol;
    float v = red[0][idx];
    for (int w = 1; w < nw; ++w) v += red[w][idx];
    const bool ok = ob < a.B && on < a.N;
    if (ok && !(fabsf(v) <= 3.0e38f)) a.state->overflow = 1;        // non-finite logit: the reference would emit NaN, never a token
    unsigned long long key = ok ? amax_key(v, on) : 0ull;
    // max over the tile's 16 columns = the 16 lanes of this row's group (xor 8, 4, 2, 1 stay inside it)
    auto kmax = [&](unsigned long long o) { key = o > key ? o : key; };
    unsigned int lo = (unsigned int)key, hi = (unsigned int)(key >> 32);
#define M2M_KEY_STEP(M)                                                                                     \
    {                                                                                                       \
      const unsigned int olo = __builtin_bit_cast(unsigned int, lane_xor<M>(__builtin_bit_cast(float, lo)));  \
      const unsigned int ohi = __builtin_bit_cast(unsigned int, lane_xor<M>(__builtin_bit_cast(float, hi)));  \
      kmax(((unsigned long long)ohi << 32) | olo);                                                          \
      lo = (unsigned int)key; hi = (unsigned int)(key >> 32);                                               \
    }
    M2M_KEY_STEP(8) M2M_KEY_STEP(4) M2M_KEY_STEP(2) M2M_KEY_STEP(1)
#undef M2M_KEY_STEP
    if (ocol == 0 && ob < a.B) atomicMax(a.keys + ob, key);
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) a.state->t = t_cur + 1;    // the step is over: advance the position
    M2M_STAMP(2, 2);
  } else {
    if (done || tid >= 256 || ob >= a.B || on >= a.N) return;
    const int idx = orow * 17 + ocol;
    float v = red[0][idx];
    for (int w = 1; w < nw; ++w) v += red[w][idx];
    a.out[(int64_t)ob * a.ldo + on] = v;
    M2M_STAMP(2, 2);
  }
}

// waves x steps decomposition of the reduction length: K = 32 * NS * NW
static bool dec_gemm_shape(int K, int* ns, int* nw) {
  switch (K) {
    case 128: *ns = 1; *nw = 4; return true;
    case 256: *ns = 2; *nw = 4; return true;
    case 384: *ns = 2; *nw = 6; return true;
    case 512: *ns = 2; *nw = 8; return true;
    default: return false;
  }
}

template <typename T>
static int launch_dec_gemm_t(const DecGemmArgs& a, hipStream_t st) {
  int ns = 0, nw = 0;
  if (!dec_gemm_shape(a.K, &ns, &nw)) {
    set_error("dec_gemm: K=%d not supported by the decode projections (128/256/384/512)", a.K);
    return M2M_ERR_INVALID;
  }
  dim3 grid((unsigned)ceil_div(a.N, 16), (unsigned)ceil_div(a.B, 16));
  dim3 block((unsigned)(64 * nw));
  if (a.keys) {
    if (ns == 1) hipLaunchKernelGGL((dec_gemm_kernel<T, 1, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((dec_gemm_kernel<T, 2, true>), grid, block, 0, st, a);
  } else {
    if (ns == 1) hipLaunchKernelGGL((dec_gemm_kernel<T, 1, false>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((dec_gemm_kernel<T, 2, false>), grid, block, 0, st, a);
  }
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

static int launch_dec_gemm(int precision, const DecGemmArgs& a, hipStream_t st) {
  return precision == M2M_PREC_BF16 ? launch_dec_gemm_t<bf16_t>(a, st) : launch_dec_gemm_t<float>(a, st);
}

// ===================================================== fused feed-forward ====
// One kernel per layer for  x += wo( gelu_new(wi_0 . n) * (wi_1 . n) ),  n = RMSNorm(x)
// (hf: modeling_t5.py T5DenseGatedActDense + T5LayerFF).  A workgroup owns 32 of the d_ff hidden
// columns for one 16-row block: it computes that slice of the gated activation (64 rows of the
// interleaved wi), keeps it in LDS, multiplies it with the matching 32 columns of wo and ADDS the
// [16 x d_model] partial result into the fixed-point residual stream (integer atomics: the sum does
// not depend on arrival order, see xq_t above).  The hidden activations never reach memory and the
// dependent kernel boundary between the up and the down projection is gone (26 -> 20 kernels/step).
// 32 columns per workgroup is the balance point measured with tools/atomic_rate.hip: d_ff/32 = 36
// adds per residual element cost ~2 us, 72 would cost ~5 us; wider slices put >100 KB of weights
// behind one CU's ~24..60 GB/s fetch path.
//
// Waves = KS = d_model / 64: wave ks multiplies k-slice ks of the normalised rows with all four
// n-tiles of the slice (a tile = 8 wi_0 rows + the matching 8 wi_1 rows, as repack.hip interleaves
// them), so the rows of x — 8 bytes per element, the largest operand — are fetched once per
// workgroup; in phase 2 wave w owns output columns [64 w, 64 w + 64).  One extra workgroup per row
// block adds the residual rows themselves and zeroes the third buffer of the rotation.  A CU pulls only ~25-30 GB/s
// from beyond its L2, so the kernel's time is the bytes one workgroup requests (at d_model 384 in bf16: x 24 KB with 8-row tiles,
// 48 KB with 16-row tiles - real rows only, whole lines, staged through LDS: row_stage_at - + weights 74 KB, 147 KB in fp32);
// every global load is issued before the first use, the rows first.  The weights come from the layer's step image (Wimg below, written
// once in m2m_model_create): a slice's 72 KiB are one block in which every load instruction of a wave reads 1 KiB of consecutive memory -
// row-major, a wo load used half of each of its 16 lines and the two wf loads of a tile shared theirs (L1 -> L2 read
// requests per launch 70 368 -> 56 544, L1 accesses 447 k -> 198 k, 6.60 -> 5.76 us).
struct DecFfArgs {
  const xq_t* x;         // [B, d] residual stream after the attention sub-layers (complete)
  xq_t* x_out;           // [B, d] zero on entry: x + FF(x) is accumulated into it
  xq_t* x_zero;          // [B, d] third buffer of the rotation, left zeroed
  const float* ln_w;
  float eps;
  const void* Wimg;      // [d_ff / 32][d / 64][12][512] T, the step image of wi and wo_ff (t5.h DecLayerPacked::ff_img): per hidden slice and
                         // wave the 8 fragment loads wf[j][s] of the interleaved wi (16-row groups: 8 rows of wi_0 then the same 8 of
                         // wi_1), then the 4 loads wo[j] of wo_ff, each 64 lanes x 16 bytes of consecutive memory (whole 128-byte lines,
                         // none shared with another slice; in the row-major layouts a wo load used half of each of its 16 lines)
  int d, d_ff, B;
  DecState* state;
  int check_done;        // headless greedy loop, layer 0: the carry workgroup of row block 0 turns "no row unfinished" into done
};

// FF_R = residual rows per workgroup (<= 16, the MFMA tile height), a template parameter chosen per chain.  Small chains: 8 halves
// the fixed-point rows a workgroup pulls (they were just written, so they come from HBM, not from a cache: tools/l2_persist.hip) at
// the price of reading the weight slices twice from the Infinity Cache: 247.3 -> 244.6 ms per batch at 2 x 16 clips; 4 rows: 259.5.
// Large chains (round 6): 16 rows halve the workgroups and the weight-slice reads of a launch (decode_ff_rows).  A row's arithmetic
// does not depend on its tile (MFMA rows are independent): ids are bit-identical whichever is taken.
constexpr int FF_C = 32;        // hidden columns per workgroup
constexpr int FF_HP = FF_C + 8; // LDS row pitch of the activation slice (elements; keeps 16-byte alignment)

// diagnostic builds only (-DM2M_FF_ABL=mask, never the product): 1 = the slice workgroups add nothing (x passes through), 2 = they read no rows of x,
// 4 (multi-slice form) = the later slices re-use the first slice's weights
#ifndef M2M_FF_ABL
#define M2M_FF_ABL 0
#endif
// The extra workgroup of each row block carries the residual itself into x_out and zeroes the third buffer (blockDim.x == d_model:
// one column per thread), so the slice workgroups issue no conditional loads (a branch around a load costs them a full s_waitcnt).
template <int FF_R>
__device__ __forceinline__ void dec_ff_carry(const DecFfArgs& a, int b0, int done) {
  const int tid = threadIdx.x, K = a.d;
  xq_t v[FF_R];
#pragma unroll
  for (int i = 0; i < FF_R; ++i) v[i] = a.x[(int64_t)min(b0 + i, a.B - 1) * K + tid];
  if (done) return;
  if (a.check_done && b0 == 0 && tid == 0) {
    // every row's layer-0 cross workgroup has counted itself in (the kernel before this one): none unfinished = the
    // batch is complete.  The token fed THIS step (position t) was the last one: t + 1 valid columns.
    if (a.state->n_unfinished == 0) { a.state->done = 1; a.state->out_len = a.state->t + 1; }
    a.state->n_unfinished = 0;
  }
#pragma unroll
  for (int i = 0; i < FF_R; ++i) {
    if (b0 + i < a.B) {
      const int64_t at = (int64_t)(b0 + i) * K + tid;
      atomicAdd(reinterpret_cast<unsigned long long*>(a.x_out + at), (unsigned long long)v[i]);
      a.x_zero[at] = 0;
    }
  }
}

// The whole sub-layer, for both kernels below: a workgroup walks NSL consecutive hidden slices of its FF_R-row block with the SAME
// normalised rows (read and normalised once).  NSL = 1 is dec_ff_kernel.  NSL > 1 (dec_ff_multi_kernel, large chains, round 6): at
// 64 clips per chain the one-slice form is bound by its atomics - 36 slice workgroups + the carry add into every residual element
// (885 K 64-bit atomics per launch; ablation build -DM2M_FF_ABL=1: 11.9 -> 7.6 us of kernel time, tools/r6_ablate.sh) - so each
// slice's partial output is converted to fixed point as for one slice and the NSL integers are summed in registers: ONE atomic per
// element and workgroup, atomics and row reads per launch / NSL.  Integer adds are associative and every float operation of a row
// is the same code whatever NSL and FF_R are, so the residual stream - and every id - is bit-identical in every form
// (tests/test_t5_gpu.py::test_multi_clip_attention_and_wide_ff_tiles_are_bit_identical).  The next slice's up-projection weights
// are requested as soon as this slice's MFMAs have consumed theirs, its down-projection weights once this slice's have been used.
// What depends on the form: the row path, the register sets of slice weights, and the store layout (16-row tiles: NSL = 1 only).
#ifndef M2M_FF_MULTI_SETS
#define M2M_FF_MULTI_SETS 1
#endif
// Fragment load f (0..7: wf[f / 2][f % 2], 8..11: wo[f - 8]) of a wave's block of the step image; p = the block + the lane's chunk.
// bf16: one 16-byte load.  fp32: two, the lanes' low halves and, 1 KiB on, their high halves.
__device__ __forceinline__ Frag<bf16_t> ff_img_frag(const bf16_t* p, int f) { return load_frag(p + f * FF_IMG_FRAG); }
__device__ __forceinline__ Frag<float> ff_img_frag(const float* p, int f) {
  Frag<float> v;
  v.lo = *reinterpret_cast<const float4*>(p + f * FF_IMG_FRAG);
  v.hi = *reinterpret_cast<const float4*>(p + f * FF_IMG_FRAG + FF_IMG_FRAG / 2);
  return v;
}
template <typename T, int KS, int FF_R, int NSL>
__device__ __forceinline__ void dec_ff_body(const DecFfArgs& a) {
  static_assert(NSL == 1 || FF_R == 8, "several slices per workgroup: the lane pairing of the 8-row form");
  M2M_STAMP_DECL
  constexpr int CPR = 32 * KS;                         // 16-byte chunks per row
  __shared__ float ss_s[KS][16];
  __shared__ float red[KS][4][16 * 17];
  __shared__ __align__(16) T hs[16 * FF_HP];
  if constexpr (NSL == 1) M2M_STAMP(4, 0);   // (the stamps are the one-slice form's: kernel id 4)
  const int done = chain_done(a.state);
  const int tid = threadIdx.x, lane = tid & 63, ks = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  // XCD-aware order (workgroup id % 8 picks the XCD, each has its own L2): the row blocks that share a group of weight
  // slices run on the same XCD, so the slices are fetched into that L2 once instead of once per row block
  // (PMC: 14.2 MB fetched per launch for 2.75 MB of unique operands with the row-major order)
  const int nrb = (a.B + FF_R - 1) / FF_R, ngr = a.d_ff / (FF_C * NSL) + 1;   // row blocks; slice groups + the carry
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int c = xcd + 8 * (slot / nrb), b0 = (slot - (slot / nrb) * nrb) * FF_R;
  const int K = a.d;
  if (c >= ngr) return;   // padding workgroups (uniform)
  if (c == ngr - 1) {
    dec_ff_carry<FF_R>(a, b0, done);
    return;
  }
  const int kbeg = ks * 64 + 8 * g;
  const bool row_ok = r < FF_R && (b0 + r) < a.B;
  const int s0 = c * NSL;                                   // first slice of this workgroup
  // this lane's 16 bytes of the wave's fragment loads, slice 0: slice s is KS blocks further, fragment f of it at ff_img_frag(.., f)
  const T* const Wimg = reinterpret_cast<const T*>(a.Wimg) + (int64_t)ks * FF_IMG_WAVE + lane * (16 / (int)sizeof(T));
  constexpr int64_t SLICE = (int64_t)KS * FF_IMG_WAVE;      // elements of a slice's block

  // Lane (r, g)'s operand pieces of the rows: xraw[s][q] = elements kbeg + 32 s + 2 q + {0, 1} of row r, raw, converted only below.
  xq2_t xraw[2][4];
  // NSL = 1: the block's FF_R rows go through LDS (row_stage_at).  The block has 64 KS lanes = two rows of chunks per pass: thread tid
  // takes chunk scc of tile rows srow, srow + 2, ...  Rows past the batch re-read its last row (clamped, never a branch around a load);
  // rs = 0 for them.  srow, scc, xst and xs belong to this path alone; they stand here because the path has two halves, the requests
  // in front of the weight requests and the LDS image behind them.
  const int srow = tid >= CPR ? 1 : 0, scc = tid - srow * CPR;
  xq2_t xst[FF_R / 2];
  xq2_t* xs = nullptr;
  if constexpr (NSL == 1) {
    __shared__ __align__(16) xq2_t xs_lds[FF_R * CPR];   // the block's raw rows: FF_R x d_model x 8 bytes, 24 KB at 8 x 384
    xs = xs_lds;
#pragma unroll
    for (int i = 0; i < FF_R / 2; ++i)
      xst[i] = (M2M_FF_ABL & 2) ? xq2_t{1 << 28, 1 << 27} : *reinterpret_cast<const xq2_t*>(a.x + (int64_t)min(b0 + 2 * i + srow, a.B - 1) * K + 2 * scc);
    __builtin_amdgcn_sched_barrier(0);               // the latency-critical rows go out FIRST (loads retire in order)
  } else {
    // NSL > 1: rows read from memory in the operand pattern (staging them through LDS gave 12.28 -> 12.09 us per launch at 64 clips,
    // inside the run-to-run spread - DESIGN 4.3)
    const xq_t* xr = a.x + (int64_t)(b0 + (row_ok ? r : 0)) * K + kbeg;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int q = 0; q < 4; ++q) xraw[s][q] = (M2M_FF_ABL & 2) ? xq2_t{1 << 28, 1 << 27} : *reinterpret_cast<const xq2_t*>(xr + 32 * s + 2 * q);
  }
  float4 g0[2], g1[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    g0[s] = *reinterpret_cast<const float4*>(a.ln_w + kbeg + 32 * s);
    g1[s] = *reinterpret_cast<const float4*>(a.ln_w + kbeg + 32 * s + 4);
  }
  // NB register sets of slice weights (slice i in set i % NB, the slice NB ahead requested into the set just consumed).  The ablation
  // build prices the later slices' fetches at 2.9 of the kernel's 12.2 us with NB = 1 (-DM2M_FF_ABL=4: the later slices re-use the
  // first slice's weights), but TWO sets in flight measured SLOWER on the same box (tools/native_mc_sweep.py, us per step): 2 x 64
  // clips 351.7 / 352.7 against 344-348, with 2 slices 365.7 against 349-353, 2 x 32 clips 301.1 against 291.9 - as with the K/V
  // prefetch, bytes requested earlier delay everybody's latency-critical rows.  NB = 1.
  constexpr int NB = (NSL > 1 && sizeof(T) == 2) ? M2M_FF_MULTI_SETS : 1;
  // wf: the four n-tiles of the slice's wi rows; wo (phase 2): this wave's four output n-tiles of wo, columns [32 s, 32 s + 32) of d_ff
  Frag<T> wf[NB][4][2];
  Frag<T> wo[NB][4];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int s = 0; s < 2; ++s) wf[b][j][s] = ff_img_frag(Wimg + (s0 + b) * SLICE, 2 * j + s);
#pragma unroll
    for (int j = 0; j < 4; ++j) wo[b][j] = ff_img_frag(Wimg + (s0 + b) * SLICE, 8 + j);
  }
  // every load is in flight; the loop-state flag is forced here (two dependent scalar loads that the
  // compiler would otherwise sink to the first use, in front of the barrier on the critical path)
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("" ::"s"(done));
  if constexpr (NSL == 1) {
#pragma unroll
    for (int i = 0; i < FF_R / 2; ++i) xs[row_stage_at(2 * i + srow, scc, CPR)] = xst[i];
    __syncthreads();
    // With 8-row tiles the lanes r >= 8 are padding: they re-read the piece of lane (r - 8, g ^ 1), which sits in their own 16-lane
    // LDS read group (the same address: a broadcast, no bank conflict).
    const int lr = r & (FF_R - 1), lcc = (kbeg >> 1) ^ (r >= FF_R ? 4 : 0);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int q = 0; q < 4; ++q) xraw[s][q] = xs[row_stage_at(lr, lcc + 16 * s + q, CPR)];
  }
  float4 x0[2], x1[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    x0[s] = make_float4(xq_flt(xraw[s][0].x), xq_flt(xraw[s][0].y), xq_flt(xraw[s][1].x), xq_flt(xraw[s][1].y));
    x1[s] = make_float4(xq_flt(xraw[s][2].x), xq_flt(xraw[s][2].y), xq_flt(xraw[s][3].x), xq_flt(xraw[s][3].y));
  }

  // ---- RMSNorm once: the normalised fragments serve every slice ----
  float ss = 0.f;
#pragma unroll
  for (int s = 0; s < 2; ++s)
    ss += x0[s].x * x0[s].x + x0[s].y * x0[s].y + x0[s].z * x0[s].z + x0[s].w * x0[s].w +
          x1[s].x * x1[s].x + x1[s].y * x1[s].y + x1[s].z * x1[s].z + x1[s].w * x1[s].w;
  ss += lane_xor<16>(ss);
  ss += lane_xor<32>(ss);
  if (g == 0) ss_s[ks][r] = ss;
  __syncthreads();
  if constexpr (NSL == 1) M2M_STAMP(4, 3);
  float tot = 0.f;
#pragma unroll
  for (int w = 0; w < KS; ++w) tot += ss_s[w][r];
  const float rs = row_ok ? rsqrtf(tot / (float)K + a.eps) : 0.f;   // rs = 0 zeroes the padding rows
  Frag<T> fa[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const float xv[8] = {g0[s].x * (x0[s].x * rs), g0[s].y * (x0[s].y * rs), g0[s].z * (x0[s].z * rs),
                         g0[s].w * (x0[s].w * rs), g1[s].x * (x1[s].x * rs), g1[s].y * (x1[s].y * rs),
                         g1[s].z * (x1[s].z * rs), g1[s].w * (x1[s].w * rs)};
    fa[s] = pack_frag<T>(xv);
  }
  // 8-row tiles: rows 8..15 of the MFMA tile are padding, i.e. lanes g >= 2 hold nothing to store.  They take over half
  // of their partner's rows (lane ^ 32 <-> g ^ 2) so that every lane issues 2 adds per tile instead of
  // half the lanes issuing 4: lane (r, g) stores tile rows 4 (g & 1) + 2 (g >> 1) + {0, 1}.  (rl .. sum1 serve the 8-row forms only,
  // in the slice loop and behind it; with 16-row tiles nothing reads them.)
  const int rl = 4 * (g & 1) + 2 * (g >> 1);
  xq_t* const p0 = a.x_out + (int64_t)(b0 + rl) * K + 64 * ks + r;
  const bool ok0 = rl < FF_R && b0 + rl < a.B, ok1 = rl + 1 < FF_R && b0 + rl + 1 < a.B;
  xq_t sum0[4], sum1[4];       // NSL > 1: the slices' partial outputs, summed as integers
#pragma unroll
  for (int j = 0; j < 4; ++j) { sum0[j] = 0; sum1[j] = 0; }

#pragma unroll
  for (int i = 0; i < NSL; ++i) {
    // ---- phase 1: up projection of slice s0 + i ----
    f32x4_t acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) mma32_16(acc[j], fa[s], wf[i % NB][j][s]);
    if (i + NB < NSL && !(M2M_FF_ABL & 4)) {   // the up-projection weights of the slice NB ahead, into the set just consumed
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int s = 0; s < 2; ++s) wf[i % NB][j][s] = ff_img_frag(Wimg + (s0 + i + NB) * SLICE, 2 * j + s);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) red[ks][j][(4 * g + q) * 17 + r] = acc[j][q];
    if constexpr (NSL == 1) M2M_STAMP(4, 1);
    __syncthreads();
    if (done) return;   // uniform
    // gated activation: column cc of the slice lives in tile cc / 8 at columns (cc % 8) [wi_0] and (cc % 8) + 8 [wi_1];
    // k-slices are summed in a fixed order
    for (int idx = tid; idx < FF_R * FF_C; idx += 64 * KS) {   // rows FF_R..15 of the tile are padding and stay unread
      const int row = idx / FF_C, cc = idx % FF_C;
      const int t = cc >> 3, q = row * 17 + (cc & 7);
      float v0 = red[0][t][q], v1 = red[0][t][q + 8];
#pragma unroll
      for (int w = 1; w < KS; ++w) { v0 += red[w][t][q]; v1 += red[w][t][q + 8]; }
      hs[row * FF_HP + cc] = from_f32<T>(gelu_new_t<T>(v0) * v1);
    }
    __syncthreads();
    if constexpr (NSL == 1) M2M_STAMP(4, 5);

    // ---- phase 2: [16 x 32] activations x [32 x d_model] slice of wo, converted to fixed point per slice ----
    const Frag<T> fh = load_frag(hs + r * FF_HP + 8 * g);
    f32x4_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
      mma32_16(o[j], fh, wo[i % NB][j]);
    }
    if (i + NB < NSL && !(M2M_FF_ABL & 4)) {
#pragma unroll
      for (int j = 0; j < 4; ++j) wo[i % NB][j] = ff_img_frag(Wimg + (s0 + i + NB) * SLICE, 8 + j);
    }
    if (NSL == 1 && (M2M_FF_ABL & 1)) return;
    if constexpr (FF_R <= 8) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x2 = lane_xor<32>(o[j][2]), x3 = lane_xor<32>(o[j][3]);
        const float v0 = g < 2 ? o[j][0] : x2, v1 = g < 2 ? o[j][1] : x3;
        if constexpr (NSL == 1) {
          // one slice: every element is added as soon as it is converted (all eight converted first, then added - the order of the
          // several-slice form - measured 6.59 -> 6.78 us per launch at 2 x 16 clips: DESIGN 9.5)
          if (ok0) atomicAdd(reinterpret_cast<unsigned long long*>(p0 + 16 * j), (unsigned long long)xq_fix_guarded(v0, a.state));
          if (ok1) atomicAdd(reinterpret_cast<unsigned long long*>(p0 + 16 * j + K), (unsigned long long)xq_fix_guarded(v1, a.state));
        } else {
          sum0[j] += xq_fix_guarded(v0, a.state);
          sum1[j] += xq_fix_guarded(v1, a.state);
        }
      }
    } else {   // 16-row tiles (one slice only): every lane adds its four rows of each tile
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = 16 * (4 * ks + j) + r;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = b0 + 4 * g + q;
          if (4 * g + q < FF_R && row < a.B)
            atomicAdd(reinterpret_cast<unsigned long long*>(a.x_out + (int64_t)row * K + col), (unsigned long long)xq_fix_guarded(o[j][q], a.state));
        }
      }
    }
  }
  if constexpr (NSL > 1) {   // ONE atomic per element and workgroup
    if (M2M_FF_ABL & 1) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (ok0) atomicAdd(reinterpret_cast<unsigned long long*>(p0 + 16 * j), (unsigned long long)sum0[j]);
      if (ok1) atomicAdd(reinterpret_cast<unsigned long long*>(p0 + 16 * j + K), (unsigned long long)sum1[j]);
    }
  }
  if constexpr (NSL == 1) M2M_STAMP(4, 2);
}

// FF_R rows, one hidden slice per workgroup: the form of small chains
template <typename T, int KS, int FF_R>
__global__ __launch_bounds__(64 * KS) __attribute__((amdgpu_waves_per_eu(1, 2))) void dec_ff_kernel(DecFfArgs a) {
  dec_ff_body<T, KS, FF_R, 1>(a);
}
// 8 rows, NSL consecutive hidden slices per workgroup: the form of large chains
template <typename T, int KS, int NSL>
__global__ __launch_bounds__(64 * KS) __attribute__((amdgpu_waves_per_eu(1, 2))) void dec_ff_multi_kernel(DecFfArgs a) {
  dec_ff_body<T, KS, 8, NSL>(a);
}

template <typename T, int KS, int FF_R, int NSL>
static void launch_dec_ff_ks(const DecFfArgs& a, dim3 grid, hipStream_t st) {
  if constexpr (NSL == 1) hipLaunchKernelGGL((dec_ff_kernel<T, KS, FF_R>), grid, dim3(64 * KS), 0, st, a);
  else hipLaunchKernelGGL((dec_ff_multi_kernel<T, KS, NSL>), grid, dim3(64 * KS), 0, st, a);
}
template <typename T, int FF_R, int NSL>
static int launch_dec_ff_t(const DecFfArgs& a, hipStream_t st) {
  const int ngr = a.d_ff / (FF_C * NSL) + 1;                                  // + 1: the residual-carry workgroup
  dim3 grid((unsigned)(ceil_div(ngr, 8) * 8 * ceil_div(a.B, FF_R)));
  switch (a.d / 64) {
    case 2: launch_dec_ff_ks<T, 2, FF_R, NSL>(a, grid, st); break;
    case 4: launch_dec_ff_ks<T, 4, FF_R, NSL>(a, grid, st); break;
    case 6: launch_dec_ff_ks<T, 6, FF_R, NSL>(a, grid, st); break;
    case 8: launch_dec_ff_ks<T, 8, FF_R, NSL>(a, grid, st); break;
    default: set_error("dec_ff: d_model=%d not supported (128/256/384/512)", a.d); return M2M_ERR_INVALID;
  }
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

static int launch_dec_ff(int precision, const DecFfArgs& a, int rows, int slices, hipStream_t st) {
  if (a.d % 64 != 0 || a.d_ff % FF_C != 0) {
    set_error("dec_ff: d_model=%d must be a multiple of 64 and d_ff=%d of %d", a.d, a.d_ff, FF_C);
    return M2M_ERR_INVALID;
  }
  const bool bf = precision == M2M_PREC_BF16;
  if (slices > 1 && (a.d_ff / FF_C) % slices == 0) {        // several hidden slices per workgroup (large chains)
    if (slices == 2) return bf ? launch_dec_ff_t<bf16_t, 8, 2>(a, st) : launch_dec_ff_t<float, 8, 2>(a, st);
    if (slices == 4) return bf ? launch_dec_ff_t<bf16_t, 8, 4>(a, st) : launch_dec_ff_t<float, 8, 4>(a, st);
  }
  if (rows == 16) return bf ? launch_dec_ff_t<bf16_t, 16, 1>(a, st) : launch_dec_ff_t<float, 16, 1>(a, st);
  return bf ? launch_dec_ff_t<bf16_t, 8, 1>(a, st) : launch_dec_ff_t<float, 8, 1>(a, st);
}

// ======================================================= decode attention ====
// Fused per-(clip, head) kernel:  RMSNorm(x[b]) -> this head's projection (self: q,k,v + cache
// append at slot t; cross: q) -> single-pass ("online") softmax attention over the cached keys ->
// o[b, head] -> this head's slice of the output projection, ADDED into the residual row (integer
// adds: order-independent).  Every byte of K/V is used once, so it goes HBM -> registers (16 B per lane) with no
// LDS staging, and because the softmax is online there is no workgroup-wide reduction between
// reading K and reading V: both are requested together at kernel start and stream continuously
// while the norm and the projection run; the only reductions are at the very end.
struct DecAttnArgs {
  const xq_t* x;         // [B, d] fixed-point residual stream, complete: read by the norm (never written here)
  xq_t* x_out;           // [B, d] zero on entry: residual + every head's output projection are ADDED into it
  xq_t* x_zero;          // [B, d] third buffer of the rotation: zeroed for the kernel after next
  const float* ln_w;     // [d] RMSNorm weight of this sub-layer
  float eps;
  int d;                 // d_model
  const void* Wp;        // self: wqkv [3*inner, d] ; cross: wcq [inner, d]        (T)
  void* Kc;              // self: K cache [B][H][kv_stride][64] (slot t is written) ; cross: cross K (read only)
  void* Vc;
  int kv_stride;         // keys allocated per (b,h): Lmax (self) or S (cross)
  int n_keys;            // cross: S
  int self_len_override; // bench only: pretend t = self_len_override - 1
  const float* bias;     // self: [H][Lmax] by n = q_pos - k_pos
  int bias_stride;
  const void* Wo;        // [H][32 / E][2 d][E] T, the step image of this sub-layer's [d, inner] output projection (t5.h DecLayerPacked::wo_img /
                         // wco_img): per head and load instruction u, thread tid's 16 bytes = row tid / 2, columns 64 h + 32 (tid & 1) + E u
  int H, inner;
  DecState* state;
  // headless greedy loop, layer 0 only (null / 0 elsewhere)
  const float* emb;            // self: [V, d] token embedding — the input row is emb[token decoded from keys[b]]
  unsigned long long* keys;    // [B] arg-max keys of the previous step (self: read; cross with `book`: read, then cleared)
  int* finished;               // [B]
  int64_t* tokens;             // [session rows, max_len]: the WHOLE token matrix; row of slot b = tok_row[b]
  const int* tok_row;          // [B] clip (token-matrix row) decoded in slot b of this chain: identity until live rows are re-packed
  int max_len, V, pad_id, eos_id;
  int book;                    // cross: head 0's workgroup of every row does the row's bookkeeping at its end
  // Finished-row early-out (greedy loop): fin_skip[b * fin_stride] != 0 -> row b has emitted EOS; its tokens are pad whatever
  // is computed (hf generation/utils.py:2929), so its workgroups stop re-requesting K/V after the entry prefetch.  Never null:
  // "never skip" is a pointer to DecState::zero with stride 0 (an unconditional scalar load: a branch around it would split
  // the prologue's block of loads, see the kernel).
  const int* fin_skip;
  int fin_stride;
  // Beam search (the BEAM instantiations only; beam_nb = 0 elsewhere).  The rows of a chain are clips x beam_nb beams, beam-major.
  // Cross: row b reads the cross K/V of clip b / beam_nb (Kc / Vc hold the view's clips, not its rows).  Self: entry (slot s,
  // position j) of the cache is written once, at step j, by row s; row b reads key / value j from slot
  // (b / beam_nb) * beam_nb + anc[b][j] - its beam's path - instead of its own slot, so beams reorder without copying caches.
  const unsigned char* anc;    // self: [rows][anc_ld] ancestry of the view's first row, parity 0; parity (t & 1) at + anc_par
  int64_t anc_par;
  int anc_ld;
  int beam_nb;
  // Layer-0 token tables (the TAB instantiations of dec_attn_kernel only; null elsewhere): m2m_model::q0_tab / k0_tab / v0_tab,
  // [H][V][64] each (q fp32; k, v T).  The row's tokens: the current one from keys[b], the cached positions' from tokens[tok_row[b]].
  const float* q0_tab;
  const void* k0_tab;
  const void* v0_tab;
};

// K/V rows are read once per step.  When the per-step K/V working set is larger than the 256 MB
// Infinity Cache (540 MB at B = 32) they are loaded NON-TEMPORAL, so they do not evict what the
// latency-bound kernels re-read every step (30 MB of weights, the residual rows): 290 -> 271 ms per
// batch at B = 32.  When it fits (B <= 8) the default policy keeps K/V itself cache-resident across
// steps, which is faster (B = 1: 196 vs 204 us per step) — NT is a launch-time template choice.
typedef unsigned int m2m_u32x4 __attribute__((ext_vector_type(4)));
template <bool NT, typename V> __device__ inline V kv_load(const V* p) {
  if constexpr (NT) return __builtin_bit_cast(V, __builtin_nontemporal_load(reinterpret_cast<const m2m_u32x4*>(p)));
  else return *p;
}
#define M2M_KV_LOAD(p) kv_load<NT>(p)

// softmax exponential of a non-positive argument.  fp32 (parity) mode: accurate expf (~10 instructions).
// bf16 mode: one multiply + v_exp_f32 (relative error ~|x| * 6e-8, far below bf16's 4e-3); every key costs
// one of these in all 16 waves, so it is visible in the stream phase (216.8 -> 215.2 ms).
template <typename T> __device__ inline float m2m_exp(float x) {
  if constexpr (sizeof(T) == 2) return __builtin_amdgcn_exp2f(x * 1.4426950408889634f);
  else return expf(x);
}

// acc += <8 (bf16) / 4 (fp32) weights of one 16-byte chunk, the matching LDS-resident inputs>.
// bf16: the inputs are kept PACKED in LDS (they are rounded to bf16 anyway) and each pair goes through
// v_dot2c_f32_bf16 - 4 instructions per chunk instead of 8 converts + 8 FMAs; the per-head projections
// are VALU-bound (16 waves on 4 SIMDs), so this is their time.  fp32 (parity mode): plain FMA chain.
typedef __bf16 m2m_bf16x2 __attribute__((ext_vector_type(2)));
__device__ inline float dot2_bf16(uint32_t a, uint32_t b, float c) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(m2m_bf16x2, a), __builtin_bit_cast(m2m_bf16x2, b), c, false);
}
template <typename T> __device__ inline float chunk_dot(const Vec16<T>& w, const float* in_lds, int chunk, float acc);
template <> __device__ inline float chunk_dot<bf16_t>(const Vec16<bf16_t>& w, const float* in_lds, int chunk, float acc) {
  const uint4 x = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint32_t*>(in_lds) + chunk * 4);
  acc = dot2_bf16(w.v.x, x.x, acc);
  acc = dot2_bf16(w.v.y, x.y, acc);
  acc = dot2_bf16(w.v.z, x.z, acc);
  return dot2_bf16(w.v.w, x.w, acc);
}
template <> __device__ inline float chunk_dot<float>(const Vec16<float>& w, const float* in_lds, int chunk, float acc) {
  const float* hp = in_lds + chunk * 4;
#pragma unroll
  for (int e = 0; e < 4; ++e) acc = fmaf(hp[e], w.get(e), acc);
  return acc;
}
// store element i of an LDS input vector in the layout chunk_dot reads (bf16: packed halves; fp32: floats)
template <typename T> __device__ inline void put_in(float* in_lds, int i, float v) {
  if constexpr (sizeof(T) == 2) reinterpret_cast<bf16_t*>(in_lds)[i] = from_f32<bf16_t>(v);
  else in_lds[i] = v;
}

// ---- the per-row pieces of the decode attention (dec_attn_kernel: one clip per workgroup; C = 1 below) ----
// A row's ids and logits are bit-identical whichever kernel decodes it (tests/test_t5_gpu.py::
// test_multi_clip_attention_and_wide_ff_tiles_are_bit_identical): every float operation of a row is one of these functions - same
// lane -> element maps, same reduction trees, same key -> lane-group partition, same rounding points.  They are written over the
// clip count so that dec_attn_mc_kernel (C clips per workgroup) can call them too.  It calls da_project<T, C, LPO2> + da_append_kv
// for this step's k / v rows.  The other five were each put into it alone and timed against the parent, runs alternating in one
// job (tools/mc_piece_map.py, tools/ab_kernel_time.py): every one held ids, logits and resources, none held the time bar
// at every geometry, so dec_attn_mc_kernel still carries its own copy of da_project for q, DaSoftmax, da_merge, da_out_row and
// da_book_row, kept equal by hand and by the tests: a change to one of THOSE has to be made there as well.

// The online softmax of one lane group: running (max, sum, weighted-V) over the keys the group visits.
template <typename T> struct DaSoftmax {
  static constexpr int E = 16 / sizeof(T);
  float m_run = -1e30f, l_run = 0.f;
  float acc[E];
  __device__ __forceinline__ DaSoftmax() {
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
  }
  // one exponential per key: of (alpha, p) = (exp(m_run - m_new), exp(s - m_new)) one is always exp(0) = 1
  __device__ __forceinline__ void visit(float s, const float (&vrow)[E]) {
    const bool up = s > m_run;
    const float m_new = up ? s : m_run;
    const float ex = m2m_exp<T>(up ? m_run - s : s - m_run);
    const float alpha = up ? ex : 1.f;
    const float p = up ? 1.f : ex;
    l_run = fmaf(l_run, alpha, p);
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = fmaf(acc[e], alpha, p * vrow[e]);
    m_run = m_new;
  }
  // the key/value appended this step (relative position 0), from the LDS rows kn / vn: for the lanes of group 0
  __device__ __forceinline__ void visit_own(const float (&qv)[E], const float* kn, const float* vn, const float* biasl, int sub) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) s = fmaf(qv[e], kn[sub * E + e], s);
    s = group_sum<DK / E>(s);
    s += biasl[0];
    float vrow[E];
#pragma unroll
    for (int e = 0; e < E; ++e) vrow[e] = vn[sub * E + e];
    visit(s, vrow);
  }
};

// LDS of the merge below: w[16], l[16], lf[16], o[16][DK], g[groups][DK] (per-group partial outputs, 32 KB bf16 / 16 KB fp32).  Each
// kernel declares them as arrays of its own - as members of ONE struct their offsets turned the ORs of the merge's address arithmetic
// into multiplies and adds: dec_attn_kernel 10.66 -> 10.70 us per launch.
struct DaMergeLds { float *w, *l, *lf; float (*o)[DK]; float (*g)[DK]; };
// Merge of the 128 key groups (16 waves x 64 / LPR groups) of one row into oh, the head's output rounded to T.
// Each group's partial output goes to LDS scaled to its WAVE's maximum (one LDS write per lane
// instead of 3 cross-lane exchanges per accumulator register: the exchanges were the bulk of the
// tail's VALU time with 16 waves on 4 SIMDs); waves are then summed group by group, and the 16 wave
// results are brought to the global maximum by the 64 threads that finish the row.  `mid` runs behind the first barrier.
template <typename T, typename Mid>
__device__ __forceinline__ void da_merge(const DaSoftmax<T>& sm, const DaMergeLds& red, float* oh, Mid mid) {
  constexpr int E = 16 / sizeof(T), LPR = DK / E;
  constexpr int GPW = 64 / LPR;                    // groups per wave: 8 (bf16) / 4 (fp32)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sub = lane % LPR;
  const float mw = wave_max(sm.m_run);
  const float scale = m2m_exp<T>(sm.m_run - mw);       // groups that saw no key have m_run = -1e30 -> 0 (or 1 if the whole wave saw none: l = acc = 0)
  float lsum = (sub == 0) ? sm.l_run * scale : 0.f;   // l is replicated over a group's lanes: count it once
  lsum = wave_sum(lsum);
  float* gp = &red.g[wave * GPW + lane / LPR][sub * E];
#pragma unroll
  for (int e = 0; e < E; e += 4)
    *reinterpret_cast<float4*>(gp + e) = make_float4(sm.acc[e] * scale, sm.acc[e + 1] * scale, sm.acc[e + 2] * scale, sm.acc[e + 3] * scale);
  if (lane == 0) { red.w[wave] = mw; red.l[wave] = lsum; }
  __syncthreads();
  mid();
  {
    // every wave brings ITS partial sums to the global maximum here (one exponential per wave, in parallel),
    // so the single wave that finishes the row below only adds: the 16 exponentials it used to evaluate were
    // ~0.4 us of serial VALU time per launch
    float M = red.w[lane & 15];
    M = fmaxf(M, lane_xor<8>(M)); M = fmaxf(M, lane_xor<4>(M)); M = fmaxf(M, lane_xor<2>(M)); M = fmaxf(M, lane_xor<1>(M));
    const float fw = m2m_exp<T>(red.w[wave] - M);
    float sw = red.g[wave * GPW][lane];             // thread (wave, lane = dim): this wave's groups, fixed order
#pragma unroll
    for (int j = 1; j < GPW; ++j) sw += red.g[wave * GPW + j][lane];
    red.o[wave][lane] = sw * fw;
    if (lane == 0) red.lf[wave] = red.l[wave] * fw;
  }
  __syncthreads();
  if (tid < DK) {
    float s = 0.f, L = 0.f;
#pragma unroll
    for (int wv = 0; wv < 16; ++wv) {
      s += red.o[wv][tid];
      L += red.lf[wv];
    }
    // the projection input is rounded to T, as every GEMM input (L = 0: a finished row's empty cross softmax).  !(L <= 0) keeps a NaN
    // softmax (NaN encoder states, e.g. from a NaN sample) NaN, so the residual's range guard sees it instead of a zero head output.
    put_in<T>(oh, tid, !(L <= 0.f) ? s / L : 0.f);
  }
  __syncthreads();
}

// RMSNorm of one row into hn (rounded to the GEMM-input type T) by a 1024-thread workgroup, for dec_token_tables_kernel: thread tid
// holds elements [xc, xc + 4) of the row (`row()`, evaluated by the owning waves only) and of the norm weight gv; redw: 16
// cross-wave slots; `mid` runs behind the first barrier.  This RESTATES section 1 of dec_attn_kernel, statement for statement (a
// change there has to be made here): a table entry must have the step's bits, and the sum of squares is a plain expression that
// the compiler contracts as it sees fit per kernel.  dec_attn_kernel does not call it because called, every instantiation of that
// kernel got another instruction schedule in its prologue, while with its own text the instantiations without tables stay
// instruction for instruction the parent's.  In the ISA the two norms are the same sequence (v_mul, three
// v_fmac, the same wave_sum and 16-slot sum, the same division, v_rsq and v_pk_mul); tests/test_dec_token_tables_gpu.py holds the
// bits: every table leg is torch.equal with the projecting one.
template <typename T, typename Row, typename Mid>
__device__ __forceinline__ void da_norm_row(Row row, const float4& gv, int xc, int d, float eps, float* redw, float* hn, Mid mid) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool own_wave = wave * 256 < d;           // wave-uniform
  const bool own = tid * 4 < d;
  float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (own_wave) {
    xv = row();
    float ss = own ? (xv.x * xv.x + xv.y * xv.y + xv.z * xv.z + xv.w * xv.w) : 0.f;
    ss = wave_sum(ss);
    if (lane == 0) redw[wave] = ss;
  } else if (lane == 0) {
    redw[wave] = 0.f;
  }
  __syncthreads();
  mid();
  if (own) {
    float tot = 0.f;
#pragma unroll
    for (int wv = 0; wv < 16; ++wv) tot += redw[wv];
    const float rs = rsqrtf(tot / (float)d + eps);
    put_in<T>(hn, xc + 0, gv.x * (xv.x * rs));
    put_in<T>(hn, xc + 1, gv.y * (xv.y * rs));
    put_in<T>(hn, xc + 2, gv.z * (xv.z * rs));
    put_in<T>(hn, xc + 3, gv.w * (xv.w * rs));
  }
  __syncthreads();
}

// One projection output of this head for C rows: acc[c] = <weight row, hn row c>, the weight row's 16-byte chunks strided over the
// LPO lanes of the output (`part`: this lane's), the first WREG of them in registers, the rest (d_model / dtype combinations
// beyond the register budget: fp32) fetched here; every lane of the output gets the sums.  hn: [C][d], normalised, rounded to T.
template <typename T, int C, int LPO, int WREG>
__device__ __forceinline__ void da_project(float (&acc)[C], const Vec16<T> (&w)[WREG], const T* wrow, int cnt, int part, const float* hn, int d) {
  constexpr int E = 16 / sizeof(T);
  using V16 = decltype(Vec16<T>().v);
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
#pragma unroll
  for (int u = 0; u < WREG; ++u) {
    if (u < cnt) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] = chunk_dot<T>(w[u], hn + c * d, u * LPO + part, acc[c]);
    }
  }
  for (int i = WREG; i < cnt; i += 4) {
    Vec16<T> w2[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) w2[u].v = *reinterpret_cast<const V16*>(wrow + (min(i + u, cnt - 1) * LPO + part) * E);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (i + u < cnt) {
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = chunk_dot<T>(w2[u], hn + c * d, (i + u) * LPO + part, acc[c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = group_sum<LPO>(acc[c]);
}

// The k / v element (k: which2 == 1) dd2 of this step for row c: rounded to T, appended to the row's cache block at position t
// (Kb / Vb: the block of row 0, rows kv_clip elements apart; `store`: the row exists and its chain is live) and published in kn / vn.
// k or v is a SELECT of the two targets, not a branch: which2 comes from threadIdx, so a branch is two exec-masked store sequences per
// row - in dec_attn_mc_kernel's four rows 18.32 against 18.17 us per launch where the select reads 18.00.
template <typename T>
__device__ __forceinline__ void da_append_kv(float s2, int c, int which2, int dd2, int t, int64_t kv_clip, T* Kb, T* Vb, float* kn, float* vn, bool store) {
  const T r = from_f32<T>(s2);                       // k, v are stored (and used) rounded to T
  const int64_t slot = (int64_t)c * kv_clip + (int64_t)t * DK + dd2;
  (which2 == 1 ? kn : vn)[c * DK + dd2] = to_f32(r);
  if (store) (which2 == 1 ? Kb : Vb)[slot] = r;
}

// Output projection of this head (wo: this lane's half of output column on_) from oh, ADDED into residual row b of x_out.  Head 0 also
// carries the residual itself (`carry()`: its fixed-point value, evaluated by head 0 only), the last head zeroes the third buffer.
template <typename T, int OCH, typename Carry>
__device__ __forceinline__ void da_out_row(const DecAttnArgs& a, const Vec16<T> (&wo)[OCH], const float* oh, int b, bool live, bool add_heads, Carry carry) {
  const int tid = threadIdx.x, hh = blockIdx.x, on_ = min(tid >> 1, a.d - 1), opart = tid & 1;
  float accp = 0.f;
#pragma unroll
  for (int u = 0; u < OCH; ++u) accp = chunk_dot<T>(wo[u], oh, opart * OCH + u, accp);
  accp += lane_xor<1>(accp);
  if (opart == 0 && tid < 2 * a.d && live) {
    xq_t add = xq_fix_guarded(accp, a.state);
    if (hh == 0) add += carry();
    if (add_heads || hh == 0)
      atomicAdd(reinterpret_cast<unsigned long long*>(a.x_out + (int64_t)b * a.d + on_), (unsigned long long)add);
    if (hh == a.H - 1) a.x_zero[(int64_t)b * a.d + on_] = 0;
  }
}

// Headless bookkeeping of row b (one thread), after the layer-0 self-attention kernel (all head workgroups of the row) has consumed
// the key: the token fed at this step goes into the token matrix, EOS finishes the row, the key is cleared for this
// step's lm_head.  (hf generation/utils.py:2925-2937.)
__device__ __forceinline__ void da_book_row(const DecAttnArgs& a, int b, int st_t, int st_done) {
  if (!st_done) {
    const int fin = a.finished[b];
    const int next = amax_key_token(a.keys[b], fin, a.V, a.pad_id);
    if (st_t < a.max_len) a.tokens[(int64_t)a.tok_row[b] * a.max_len + st_t] = next;
    const int nf = fin | (next == a.eos_id);
    a.finished[b] = nf;
    if (!nf) atomicAdd(&a.state->n_unfinished, 1);
    a.keys[b] = 0ull;
  }
  if (b == 0) a.state->t_copy = st_t;      // ALWAYS (also in the no-op steps after the end): the lm_head kernel's "live" test reads it
}

// TAB (layer-0 self-attention of the headless greedy step, FETCH; M2M_DEC_TOKEN_TABLES): 1 takes this step's q, k, v from the
// model's token tables (m2m_model::q0_tab ...: no norm, no projection, no q / k / v weights), 2 also reads the cached K/V rows from
// the tables, addressed by the row's token history, instead of streaming the cache.  Only FETCH: there the input row IS emb[tok].
// The steps that read the row from x (teacher-forced, M2M_HEADLESS=0, the select and beam heads) see its fixed-point image, which
// differs from emb[tok] wherever an element is not a multiple of 2^-30 - their q, k, v are not what the tables hold.
template <typename T, bool SELF, bool NT, bool FETCH = false, bool BEAM = false, int TAB = 0>
__global__ __launch_bounds__(1024) void dec_attn_kernel(DecAttnArgs a) {
  static_assert(!FETCH || SELF, "only the layer-0 self-attention fetches its input row from the embedding table");
  static_assert(!(FETCH && BEAM), "the beam step is not headless");
  static_assert(TAB == 0 || FETCH, "the token tables serve the headless layer-0 self-attention: its input row is emb[tok] itself");
  constexpr bool TABLE = TAB > 0;
  constexpr bool NTS = NT && TAB != 2;   // the stream's cache policy: table rows are re-read by every clip and step, never non-temporal
  constexpr int E = 16 / sizeof(T);      // elements per 16-byte chunk: 8 (bf16) / 4 (fp32)
  constexpr int LPR = DK / E;            // lanes per key row (a "group"): 8 / 16
  constexpr int KPW = 64 / LPR;          // keys per wave-load: 8 / 4
  constexpr int KPB = 16 * KPW;          // keys per block round: 128 / 64
  constexpr int NOUT = DK;               // the query projection (self and cross alike): 64 outputs
  constexpr int LPO = 16;                // lanes per projection output
  // self only: the k,v rows this step appends are projected LATER (their weights stream in under
  // the K/V cache reads and they are needed only for the final key), so the prologue is as short
  // as the cross kernel's: 128 outputs x 8 lanes
  constexpr int LPO2 = 8;
  constexpr int WMAX2 = 6;               // k/v weight chunks per lane held in registers (d_model 384, bf16)
  // K/V rounds (one K row + one V row per lane = 32 KB per workgroup) kept in flight by the rolling
  // prefetch.  The first PF rounds are requested at kernel entry, right behind the prologue's own
  // loads (the x row first: loads retire in order), so the stream is already running while the norm
  // and the query projection execute.  Two rounds is the measured optimum (B = 32, ms per batch:
  // PF 1 / 2 / 3 = 219.4 / 217.4 / 229.2): deeper windows flood the fabric queues ahead of the
  // latency-critical x / weight loads of workgroups that start a little later, and the whole 220 KB
  // stream at once stalls the issuing waves (prologue done at ~9 us).
#ifndef M2M_DA_PF_CROSS
#define M2M_DA_PF_CROSS 2
#endif
#ifndef M2M_DA_PF_SELF
#define M2M_DA_PF_SELF 2
#endif
#ifndef M2M_DA_REQUEST_FIRST
#define M2M_DA_REQUEST_FIRST 0
#endif
  // fp32 (parity) mode, cross-attention: 4 rounds.  Its per-workgroup stream is 442 KB at S = 864 against a ~3 us prologue, and the
  // same-box A/B (tools/r6_fp32_sweep.sh, 32 x S = 864, us per step incl. encoder) reads 345.1 / 345.5 / 345.9 with 2 rounds, 345.5
  // with 3, 340.9 with 4; 3 rounds in the self-attention: 353.4.
#ifndef M2M_DA_PF_CROSS_F32
#define M2M_DA_PF_CROSS_F32 4
#endif
  constexpr int PF = SELF ? M2M_DA_PF_SELF : (sizeof(T) == 4 ? M2M_DA_PF_CROSS_F32 : M2M_DA_PF_CROSS);
  constexpr int WMAX = 3;                // q weight chunks per lane held in registers (d_model 384, bf16)
  using V16 = decltype(Vec16<T>().v);
  extern __shared__ __align__(16) float hn[];   // [d] normalised input row (already rounded to T)
  __shared__ float redw[16], redl[16], redlf[16];   // (redw: also the norm's cross-wave slots, before the merge needs it)
  __shared__ float redo[16][DK];
  __shared__ __align__(16) float redg[16 * (64 / LPR)][DK];
  const DaMergeLds red{redw, redl, redlf, redo, redg};
  __shared__ __align__(16) float qs[DK];
  __shared__ __align__(16) float kn[DK];
  __shared__ __align__(16) float vn[DK];
  __shared__ __align__(16) float oh[DK];
  M2M_STAMP_DECL
  M2M_STAMP(6 + (SELF ? 1 : 0), 0);
  // loop state: requested now, first consumed AFTER the prologue loads below have been issued, so
  // its round trip overlaps theirs instead of preceding it (every kernel of the step is latency-bound:
  // at B = 1 a step still takes 196 us, i.e. 7.5 us per kernel with nothing to stream)
  const int st_t = a.state->t;
  const int st_done = a.state->done | (st_t >= a.state->max_steps);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = blockIdx.x, b = blockIdx.y;   // grid (H, B): linear id = 8 b + h as before (a head's clips on one XCD), no division
  // finished-row flag (scalar, requested with the loop state; first consumed after the prologue).  In the layer-0 cross kernel
  // head 0 of the row WRITES the flag at its end while its siblings may still be starting: they can disagree at the one step in
  // which the row finishes — harmless, that step's output is the first one forced to pad.
  const int row_fin = a.fin_skip[(int64_t)b * a.fin_stride];
  const int sub = lane % LPR;
  const int kslot = wave * KPW + lane / LPR;
  const int bkv = (BEAM && !SELF) ? b / a.beam_nb : b;      // beam cross-attention: the clip's K/V, shared by its beams
  T* Kb = reinterpret_cast<T*>(a.Kc) + ((int64_t)bkv * a.H + hh) * a.kv_stride * DK;
  T* Vb = reinterpret_cast<T*>(a.Vc) + ((int64_t)bkv * a.H + hh) * a.kv_stride * DK;
  // beam self-attention: this row's ancestry (slot of every cached position) goes to LDS before any K/V request, which it addresses
  // (one more round trip at entry; a byte per position).  Values are clamped into the clip, so no request leaves its beams' slots.
  unsigned char* const ancl = reinterpret_cast<unsigned char*>(hn + a.d + (SELF ? a.bias_stride : 0));   // [kv_stride] (BEAM && SELF)
  const int beam = (BEAM && SELF) ? b % a.beam_nb : 0;
  if constexpr (BEAM && SELF) {
    const unsigned char* ar = a.anc + (int64_t)(st_t & 1) * a.anc_par + (int64_t)b * a.anc_ld;
    const int na = min(max(st_t, 1), a.kv_stride);
    for (int j = tid; j < na; j += 1024) ancl[j] = j < st_t ? (unsigned char)min((int)ar[j], a.beam_nb - 1) : (unsigned char)beam;
    __syncthreads();
  }
  // element offset of key row `key` (clamped) from Kb / Vb, for this lane's part of it
  // table form of the stream (TAB == 2): key row `key` is row tokl[key] of this head's k / v table
  unsigned short* const tokl = reinterpret_cast<unsigned short*>(hn + a.d + (SELF ? a.bias_stride : 0));   // [kv_stride] (TAB == 2)
  auto kvoff = [&](int key) -> int64_t {
    if constexpr (TAB == 2) return (int64_t)tokl[key] * DK + sub * E;
    int64_t o = (int64_t)key * DK + sub * E;
    if constexpr (BEAM && SELF) o += ((int64_t)ancl[key] - beam) * ((int64_t)a.H * a.kv_stride * DK);
    return o;
  };
  // where the stream reads from: the row's cache block, or (TAB == 2) this head's tables
  const T* const Ks = TAB == 2 ? reinterpret_cast<const T*>(a.k0_tab) + (int64_t)hh * a.V * DK : Kb;
  const T* const Vs = TAB == 2 ? reinterpret_cast<const T*>(a.v0_tab) + (int64_t)hh * a.V * DK : Vb;

  // ---- 0. requests for the prologue: x row, norm weights, this lane's projection weights.
  //         Every kernel starts with a cold L2 for data other XCDs produced, so these come from
  //         memory; if the 220 KB K/V stream of this workgroup were requested at the same time they
  //         would queue behind it in the fabric (measured: the norm then completes only after ~9 us).
  //         Only the first PF rounds of the stream follow them here. ----
  const int xc = min(tid * 4, a.d - 4);
  const int on_ = min(tid >> 1, a.d - 1), opart = tid & 1;
  // RAW fixed-point words: converted only after every request below has been issued (the conversion needs the
  // data, and in program order it would put the wait for x in front of the K/V prefetch)
  longlong2 xr0 = make_longlong2(0, 0), xr1 = make_longlong2(0, 0);
  xq_t xres = 0;
  unsigned long long kraw = 0;
  int fin0 = 0;
  const int64_t* hrow = nullptr;  // table form: the row's tokens
  if constexpr (FETCH) {          // headless layer 0: the row is an embedding row, chosen by the previous step's arg-max key
    kraw = a.keys[b];
    fin0 = a.finished[b];
    if constexpr (TABLE) hrow = a.tokens + (int64_t)a.tok_row[b] * a.max_len;
  } else {
    xr0 = *reinterpret_cast<const longlong2*>(a.x + (int64_t)b * a.d + xc);
    xr1 = *reinterpret_cast<const longlong2*>(a.x + (int64_t)b * a.d + xc + 2);
    // head 0 also carries the residual row into x_out: its raw fixed-point value, requested now
    xres = a.x[(int64_t)b * a.d + on_];   // unconditional: a branch would split the block of loads
  }
  // table form, cached K/V from the tables: the ids of the cached positions, HPT per thread in registers (2048 positions; more:
  // the loop below), addresses clamped into the row's written part
  constexpr int HPT = 2;
  int64_t hv[TAB == 2 ? HPT : 1];
  if constexpr (TAB == 2) {
#pragma unroll
    for (int u = 0; u < HPT; ++u) hv[u] = hrow[min(tid + 1024 * u, max(st_t - 1, 0))];
  }
  float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (!TABLE) gv = *reinterpret_cast<const float4*>(a.ln_w + xc);
  __builtin_amdgcn_sched_barrier(0);               // the latency-critical row goes out FIRST (loads retire in order)
  const int po = min(tid / LPO, NOUT - 1), part = tid % LPO;
  const int which = po / DK, dd = po - which * DK;
  const T* wrow = reinterpret_cast<const T*>(a.Wp) + ((int64_t)which * a.inner + hh * DK + dd) * a.d;
  const int cnt = a.d / E / LPO;         // chunks per lane
  Vec16<T> w[TABLE ? 1 : WMAX];
  if constexpr (!TABLE) {
#pragma unroll
    for (int u = 0; u < WMAX; ++u) w[u].v = *reinterpret_cast<const V16*>(wrow + (min(u, cnt - 1) * LPO + part) * E);
  }
  // self: this head's relative-position bias row goes to LDS.  Read from global memory inside the key
  // loop it would sit behind the next round's K/V request in the wave's in-order vmcnt queue: the
  // compiler then has to wait vmcnt(0) every round, and the stream runs at one round per memory latency.
  float* const biasl = hn + a.d;                      // [kv_stride] (self only)
  constexpr int BPT = 2;                               // bias entries per thread held in registers (Lmax <= 2048; more: loop below)
  float bv[SELF ? BPT : 1];
  if (SELF) {
#pragma unroll
    for (int u = 0; u < BPT; ++u) bv[u] = a.bias[(int64_t)hh * a.bias_stride + min(tid + 1024 * u, a.bias_stride - 1)];
  }

  // No early exit on st_done: a branch here makes the compiler sink the weight loads above below
  // it, behind the wait for x (one more serial round trip).  A finished chain runs at most the rest
  // of its graph with every store suppressed.
  const int t = SELF ? (a.self_len_override > 0 ? a.self_len_override - 1 : st_t) : 0;
  const int n_prev = SELF ? t : a.n_keys;            // keys that are read from memory
  const int last = max(n_prev - 1, 0);

  // ---- 1. RMSNorm of x[b] -> hn (rounded to the GEMM-input type T) ----
  Vec16<T> kv[PF], vv[PF];
  if constexpr (TAB != 2) {        // (TAB == 2: the stream's addresses are token ids, requested once those are in LDS)
#pragma unroll
    for (int u = 0; u < PF; ++u) {   // clamped addresses, never predicated
      const int64_t off = kvoff(min(kslot + u * KPB, last));
      kv[u].v = kv_load<NTS>(reinterpret_cast<const V16*>(Ks + off));
      vv[u].v = kv_load<NTS>(reinterpret_cast<const V16*>(Vs + off));
    }
  }
  // everything above is in flight before anything waits: without the fence the scheduler places the wait for x
  // (and its int64 -> float conversion) ahead of the weight loads and of the K/V prefetch (the ISA showed the
  // prefetch going out only after x had arrived, ~2 us into the kernel)
  __builtin_amdgcn_sched_barrier(0);
  // Only the waves that own a piece of the row (d / 4 threads: 2 of the 16 at d_model 384) convert it and
  // reduce; the others just post a zero, so the owners do not share their SIMD's issue slots with 3 waves of
  // duplicate work (waves are spread round-robin over the 4 SIMDs).
  const bool own_wave = wave * 256 < a.d;           // wave-uniform
  float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
  float eres = 0.f;
  float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f);
  int tok = 0;
  if constexpr (FETCH) {          // second (dependent) round trip of the headless prologue: the embedding row
    tok = amax_key_token(kraw, fin0, a.V, a.pad_id);
    const float* er = a.emb + (int64_t)tok * a.d;
    if constexpr (!TABLE) e4 = *reinterpret_cast<const float4*>(er + xc);
    eres = er[on_];
  }
  if constexpr (TABLE) {
    // Table form: q, k, v of this row are the entries (head, tok) of the model's tables - what the norm and the two da_project
    // calls below would produce from emb[tok], bit for bit (dec_token_tables_kernel runs them).  Thread tid < 64 publishes q[tid],
    // tid < 128 appends k (tid < 64) or v through da_append_kv: the cache stays valid for every other reader of layer 0.
    const int64_t trow = ((int64_t)hh * a.V + tok) * DK;
    const int dd2 = tid & 63, which2 = 1 + ((tid >> 6) & 1);
    const float qe = a.q0_tab[trow + dd2];
    const T kve = (which2 == 1 ? reinterpret_cast<const T*>(a.k0_tab) : reinterpret_cast<const T*>(a.v0_tab))[trow + dd2];
    if (tid < DK) qs[dd2] = qe;
    if (tid < 2 * DK) da_append_kv<T>(to_f32(kve), 0, which2, dd2, t, 0, Kb, Vb, kn, vn, !st_done);   // (T -> fp32 -> T is the identity)
    if constexpr (TAB == 2) {
      // ids of the cached positions -> LDS, 16 bits each, clamped into the table: an unwritten position addresses a row of it
      const int nh = max(t, 1);
#pragma unroll
      for (int u = 0; u < HPT; ++u)
        if (tid + 1024 * u < nh) tokl[tid + 1024 * u] = (unsigned short)min(max(hv[u], (int64_t)0), (int64_t)a.V - 1);
      for (int n = tid + 1024 * HPT; n < nh; n += 1024) tokl[n] = (unsigned short)min(max(hrow[min(n, last)], (int64_t)0), (int64_t)a.V - 1);
    }
  }
  if constexpr (!TABLE) {
    const bool own = tid * 4 < a.d;
    if (own_wave) {
      if constexpr (FETCH) xv = e4;
      else xv = make_float4(xq_flt(xr0.x), xq_flt(xr0.y), xq_flt(xr1.x), xq_flt(xr1.y));
      float ss = own ? (xv.x * xv.x + xv.y * xv.y + xv.z * xv.z + xv.w * xv.w) : 0.f;
      ss = wave_sum(ss);
      if (lane == 0) redw[wave] = ss;
    } else if (lane == 0) {
      redw[wave] = 0.f;
    }
    __syncthreads();
    M2M_STAMP(6 + (SELF ? 1 : 0), 4);
    if (own) {
      float tot = 0.f;
#pragma unroll
      for (int wv = 0; wv < 16; ++wv) tot += redw[wv];
      const float rs = rsqrtf(tot / (float)a.d + a.eps);
      put_in<T>(hn, xc + 0, gv.x * (xv.x * rs));
      put_in<T>(hn, xc + 1, gv.y * (xv.y * rs));
      put_in<T>(hn, xc + 2, gv.z * (xv.z * rs));
      put_in<T>(hn, xc + 3, gv.w * (xv.w * rs));
    }
    __syncthreads();
    M2M_STAMP(6 + (SELF ? 1 : 0), 5);
  }

  // ---- 2. this head's projection: NOUT outputs, LPO lanes each, 16-byte chunks strided over lanes ----
  if constexpr (!TABLE) {
    float q[1];
    da_project<T, 1, LPO>(q, w, wrow, cnt, part, hn, a.d);
#ifndef M2M_STAMPS_MERGE
    M2M_STAMP(6 + (SELF ? 1 : 0), 6);
#endif
    if (part == 0 && tid < NOUT * LPO) qs[dd] = q[0];      // q stays fp32
  }
  if (SELF) {
#pragma unroll
    for (int u = 0; u < BPT; ++u)
      if (tid + 1024 * u < a.bias_stride) biasl[tid + 1024 * u] = bv[u];
    for (int n = tid + 1024 * BPT; n < a.bias_stride; n += 1024) biasl[n] = a.bias[(int64_t)hh * a.bias_stride + n];
  }
  __syncthreads();
  M2M_STAMP(6 + (SELF ? 1 : 0), 1);
  if constexpr (TAB == 2) {          // the first PF rounds of the table gather (L2 hits on the head's XCD), in front of the wo loads
#pragma unroll
    for (int u = 0; u < PF; ++u) {   // clamped addresses, never predicated
      const int64_t off = kvoff(min(kslot + u * KPB, last));
      kv[u].v = kv_load<NTS>(reinterpret_cast<const V16*>(Ks + off));
      vv[u].v = kv_load<NTS>(reinterpret_cast<const V16*>(Vs + off));
    }
  }

  // this head's slice of the output projection (2 lanes per output column, 32 inputs each):
  // requested now so it arrives under the K/V stream
  constexpr int OCH = 32 / E;            // 16-byte chunks per lane: 4 (bf16) / 8 (fp32)
  // (step image: load u of the workgroup's 2 d live threads is 2 d x 16 consecutive bytes; the threads past them re-read the last chunk)
  const T* woimg = reinterpret_cast<const T*>(a.Wo) + ((int64_t)hh * OCH * 2 * a.d + min(tid, 2 * a.d - 1)) * E;
  Vec16<T> wo[OCH];
#pragma unroll
  for (int u = 0; u < OCH; ++u) wo[u].v = *reinterpret_cast<const V16*>(woimg + (int64_t)u * 2 * a.d * E);
  // self: weights of the k,v rows this step appends (128 outputs x 8 lanes), also under the stream
  const int o2 = tid >> 3, part2 = tid & 7;
  const int which2 = 1 + (o2 >> 6), dd2 = o2 & 63;
  const T* wrow2 = reinterpret_cast<const T*>(a.Wp) + ((int64_t)which2 * a.inner + hh * DK + dd2) * a.d;
  const int cnt2 = a.d / E / LPO2;
  Vec16<T> wkv[SELF && !TABLE ? WMAX2 : 1];
  if (SELF && !TABLE) {
#pragma unroll
    for (int u = 0; u < WMAX2; ++u) wkv[u].v = *reinterpret_cast<const V16*>(wrow2 + (min(u, cnt2 - 1) * LPO2 + part2) * E);
  }

  // ---- 3. single-pass attention: each group of LPR lanes walks its keys with a running
  //         (max, sum, weighted-V) triple; no workgroup-wide step until the end ----
  // A finished row walks NO cached keys: the two rounds requested at entry are dropped, nothing is re-requested (32 KB instead
  // of the whole stream for this workgroup); the self kernel still appends and visits this step's own key, the cross kernel's
  // empty softmax gives a zero head output below.  Nothing of a finished row is observable: its tokens are pad.
  const int n_live = row_fin ? 0 : n_prev;
  float qv[E];
#pragma unroll
  for (int e = 0; e < E; ++e) qv[e] = qs[sub * E + e];
  DaSoftmax<T> sm;
  // One round: consume slot u (scores, online-softmax update), optionally re-request the round PF ahead
  // into the same slot.  REISSUE is a compile-time choice per loop: in the main loop every re-request
  // exists, so the loads are unconditional and the compiler can count them (s_waitcnt vmcnt(N) keeps the
  // next round in flight while this one is consumed); a runtime "is there a round PF ahead" test around
  // the loads makes it fall back to vmcnt(0) at every round, i.e. batches instead of a rolling window.
  auto round = [&](const int k0, const int u, Vec16<T>& ks, Vec16<T>& vs, const int reissue /*0 no, 1 yes, 2 if it exists*/) {
    const int key = k0 + kslot + u * KPB;
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) s = fmaf(qv[e], ks.get(e), s);
    s = group_sum<LPR>(s);                                                   // every lane of the group gets the sum
#if M2M_DA_REQUEST_FIRST       // rounds 1-5: the slot re-requested BEFORE its visit (see below)
    float vrow[E];
#pragma unroll
    for (int e = 0; e < E; ++e) vrow[e] = vs.get(e);
    if (reissue == 1 || (reissue == 2 && k0 + (u + PF) * KPB < n_live)) {   // workgroup-uniform, no lane is predicated
      const int64_t off = kvoff(min(key + PF * KPB, last));
      ks.v = kv_load<NTS>(reinterpret_cast<const V16*>(Ks + off));
      vs.v = kv_load<NTS>(reinterpret_cast<const V16*>(Vs + off));
    }
    if (key < n_live) {   // VALU-only predicate
      if (SELF) s += biasl[t - key];
      sm.visit(s, vrow);
    }
#else
    // The slot is re-requested AFTER it has been consumed (round 6).  With the request in front of the visit the compiler sinks V's
    // unpacking into the predicated block, keeps the packed V alive past the request, loads into a SECOND register set and copies
    // it back behind s_waitcnt vmcnt(0) at the end of EVERY iteration (ISA of rounds 1-5: vmcnt(2), 4 v_mov, vmcnt(0), 4 v_mov at
    // the back edge): the "rolling window" drained once per iteration - two rounds per memory round trip and CU.
    if (key < n_live) {   // VALU-only predicate
      float vrow[E];
#pragma unroll
      for (int e = 0; e < E; ++e) vrow[e] = vs.get(e);
      if (SELF) s += biasl[t - key];
      sm.visit(s, vrow);
    }
    if (reissue == 1 || (reissue == 2 && k0 + (u + PF) * KPB < n_live)) {   // workgroup-uniform, no lane is predicated
      const int64_t off = kvoff(min(key + PF * KPB, last));
      ks.v = kv_load<NTS>(reinterpret_cast<const V16*>(Ks + off));
      vs.v = kv_load<NTS>(reinterpret_cast<const V16*>(Vs + off));
    }
#endif
  };
  int k0 = 0;
  // main loop: all PF re-requests of the iteration exist (the last one targets round k0 / KPB + 2 PF - 1)
  for (; k0 + (2 * PF - 1) * KPB < n_live; k0 += PF * KPB) {
#pragma unroll
    for (int u = 0; u < PF; ++u) round(k0, u, kv[u], vv[u], 1);
  }
  // tail (at most two iterations): past the end nothing is requested, so the merge barrier below does
  // not wait for a useless round trip
  for (; k0 < n_live; k0 += PF * KPB) {
#pragma unroll
    for (int u = 0; u < PF; ++u) round(k0, u, kv[u], vv[u], 2);
  }
  if constexpr (SELF && !TABLE) {
    // project, round to T, append to the cache and publish through LDS the k,v rows of this step (table form: done in the prologue)
    float kvn[1];
    da_project<T, 1, LPO2>(kvn, wkv, wrow2, cnt2, part2, hn, a.d);
    if (part2 == 0) da_append_kv<T>(kvn[0], 0, which2, dd2, t, 0, Kb, Vb, kn, vn, !st_done);
    __syncthreads();
  }
  if (SELF && wave == 0 && lane < LPR) sm.visit_own(qv, kn, vn, biasl, sub);   // group 0
  M2M_STAMP(6 + (SELF ? 1 : 0), 2);

  // ---- 4. merge the 128 key groups (16 waves x 64 / LPR groups) ----
  da_merge<T>(sm, red, oh, [&] {
#ifdef M2M_STAMPS_MERGE
    M2M_STAMP(6 + (SELF ? 1 : 0), 6);
#endif
  });
  M2M_STAMP(6 + (SELF ? 1 : 0), 7);
  // ---- 5. output projection of this head, accumulated into the residual row ----
  da_out_row<T>(a, wo, oh, b, !st_done, true, [&] { return FETCH ? xq_fix_guarded(eres, a.state) : xres; });
  if (!SELF && a.book && hh == 0 && tid == 0) da_book_row(a, b, st_t, st_done);
  M2M_STAMP(6 + (SELF ? 1 : 0), 3);
}

// ---- the layer-0 token tables (t5.h m2m_model::q0_tab / k0_tab / v0_tab; run once in m2m_model_create) ----
// Workgroup (head, tok) computes what dec_attn_kernel<T, true, NT, FETCH = true> computes from emb[tok] in front of its stream: the
// same thread -> element maps and the same calls (da_norm_row; da_project<T, 1, LPO> for q, kept fp32; da_project<T, 1, LPO2> +
// from_f32<T> for k, v), with the same weights in registers - so that an entry has the bits the step would have produced, and the
// table form of the step changes where bytes come from and nothing else (tests/test_dec_token_tables_gpu.py: torch.equal).
template <typename T>
__global__ __launch_bounds__(1024) void dec_token_tables_kernel(const float* __restrict__ emb, const float* __restrict__ ln_w, const T* __restrict__ Wp,
                                                                int d, int inner, int V, float eps, float* __restrict__ q0, T* __restrict__ k0,
                                                                T* __restrict__ v0) {
  constexpr int E = 16 / sizeof(T), NOUT = DK, LPO = 16, LPO2 = 8, WMAX = 3, WMAX2 = 6;   // dec_attn_kernel's
  using V16 = decltype(Vec16<T>().v);
  extern __shared__ __align__(16) float hn[];
  __shared__ float redw[16];
  const int tid = threadIdx.x, hh = blockIdx.x, tok = blockIdx.y;
  const int xc = min(tid * 4, d - 4);
  const float4 gv = *reinterpret_cast<const float4*>(ln_w + xc);
  const float4 e4 = *reinterpret_cast<const float4*>(emb + (int64_t)tok * d + xc);
  const int po = min(tid / LPO, NOUT - 1), part = tid % LPO;
  const int which = po / DK, dd = po - which * DK;
  const T* wrow = Wp + ((int64_t)which * inner + hh * DK + dd) * d;
  const int cnt = d / E / LPO;
  Vec16<T> w[WMAX];
#pragma unroll
  for (int u = 0; u < WMAX; ++u) w[u].v = *reinterpret_cast<const V16*>(wrow + (min(u, cnt - 1) * LPO + part) * E);
  const int o2 = tid >> 3, part2 = tid & 7;
  const int which2 = 1 + (o2 >> 6), dd2 = o2 & 63;
  const T* wrow2 = Wp + ((int64_t)which2 * inner + hh * DK + dd2) * d;
  const int cnt2 = d / E / LPO2;
  Vec16<T> wkv[WMAX2];
#pragma unroll
  for (int u = 0; u < WMAX2; ++u) wkv[u].v = *reinterpret_cast<const V16*>(wrow2 + (min(u, cnt2 - 1) * LPO2 + part2) * E);
  da_norm_row<T>([&] { return e4; }, gv, xc, d, eps, redw, hn, [] {});
  const int64_t trow = ((int64_t)hh * V + tok) * DK;
  float q[1], kvn[1];
  da_project<T, 1, LPO>(q, w, wrow, cnt, part, hn, d);
  if (part == 0 && tid < NOUT * LPO) q0[trow + dd] = q[0];
  da_project<T, 1, LPO2>(kvn, wkv, wrow2, cnt2, part2, hn, d);
  if (part2 == 0) (which2 == 1 ? k0 : v0)[trow + dd2] = from_f32<T>(kvn[0]);
}

int launch_token_tables(const m2m_model* m, hipStream_t st) {
  if (!m->q0_tab) return M2M_OK;
  const m2m_t5_geometry& g = m->g;
  const DecLayerPacked& L = m->dec[0];
  const dim3 grid((unsigned)g.num_heads, (unsigned)g.vocab_size);      // vocab_size <= 65 535 (the gate of m2m_model_create)
  const size_t smem = (size_t)g.d_model * sizeof(float);
  float* q0 = const_cast<float*>(m->q0_tab);
  if (m->precision == M2M_PREC_BF16)
    hipLaunchKernelGGL(dec_token_tables_kernel<bf16_t>, grid, dim3(1024), smem, st, m->shared, L.ln0, (const bf16_t*)L.wqkv, g.d_model, m->inner,
                       g.vocab_size, g.layer_norm_eps, q0, (bf16_t*)const_cast<void*>(m->k0_tab), (bf16_t*)const_cast<void*>(m->v0_tab));
  else
    hipLaunchKernelGGL(dec_token_tables_kernel<float>, grid, dim3(1024), smem, st, m->shared, L.ln0, (const float*)L.wqkv, g.d_model, m->inner,
                       g.vocab_size, g.layer_norm_eps, q0, (float*)const_cast<void*>(m->k0_tab), (float*)const_cast<void*>(m->v0_tab));
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

// ---- the same kernel for LARGE chains: C clips of one head per workgroup (round 6) ----
// At the reference's own chunk (128 three-second segments, S = 190: ref music2midi/model.py:115-135, config.yaml inference.batch_size) a
// chain launches 512 (clip, head) workgroups per attention kernel, one per CU at a time (16 waves x ~124 VGPRs), and each of them is the
// same latency chain as at 16 clips: the row its predecessor wrote (~2.4 us), then its head's projection weights from L2 - 192 KB
// (self) / 96 KB (cross) against a K/V stream of 131 KB (t = 512) / 49 KB: 1 024 workgroups pull more bytes from L2 as weights than
// from HBM as K/V, and the regime is throughput-bound (12 attention launches x 2 rounds of workgroups per chain and step).  Here a
// workgroup owns one head of C consecutive clips: ONE row round trip for all of them (wave pair c normalises clip c's row), the
// head's weights fetched ONCE into the same registers and applied to the C rows (self: q AND this step's k, v rows up front, so
// the 24 weight registers are free again when the streams start), one bias row in LDS, then the clips' K/V streams walked one
// after the other by all 16 waves as ONE continuous stream: a clip's rounds are padded to a multiple of the prefetch depth, and
// its last rounds re-request into the NEXT live clip, so MC_PF rounds are in flight through every merge - and the C output
// projections at the end.
// Per row the arithmetic is the first kernel's (dec_attn_kernel and its da_* pieces above): this step's k / v rows are its
// da_project + da_append_kv, called; the rest is repeated here operation for operation (same lane -> element maps, same reduction
// trees, same key -> lane-group partition, same rounding points; why it is repeated and not called: the note above the pieces and, per
// piece, the one-line notes below): ids and logits are bit-identical whichever form a chain takes
// (tests/test_t5_gpu.py::test_multi_clip_attention_and_wide_ff_tiles_are_bit_identical).  Chosen per chain by its clip count.
// Prefetch depth (rounds in flight per workgroup).  Same-box A/B at 128 x S = 190, two chains of 64 clips, C = 2 (tools/r6_mc_ab.sh,
// us per decode step): 2 rounds 370.0, 3 rounds 379.5, 4 rounds 394.0, 6 rounds 457.5 - as in the small-chain regime (the first
// kernel's PF note) more bytes in flight per CU only lengthen every workgroup's latency-critical loads: the launches of a chain
// start their streams together, the memory system is saturated in those bursts, and its loaded latency is bytes in flight / rate.
#ifndef M2M_MC_PF_SELF
#define M2M_MC_PF_SELF 2
#endif
#ifndef M2M_MC_PF_CROSS
#define M2M_MC_PF_CROSS 2
#endif
// diagnostic builds only (-DM2M_MC_ABL=mask, never the product): 1 = no output-projection atomics, 2 = no K/V stream
#ifndef M2M_MC_ABL
#define M2M_MC_ABL 0
#endif
// Waves per SIMD the kernel is compiled for: 4 = the 128 registers of a 16-wave workgroup alone on its CU; 8 = 64 registers, TWO
// workgroups per CU.  Same-box A/B (tools/r6_mc_ab.sh, 128 x S = 190, us per step): two chains of 64 clips, C = 4: 364.2 / 364.9 at
// 4 waves against 409.4 / 411.4 at 8; C = 2: 379.2 / 382.5 against 384.8 / 387.5; only ONE chain of 128 clips with C = 2 (512
// workgroups per launch) prefers 8 (411-417 against 437-440).  Co-resident workgroups of two chains stream at the same time, and
// more streams in flight cost more than the latency phases they hide - the same finding as the prefetch depth.
#ifndef M2M_MC_WAVES
#define M2M_MC_WAVES 4
#endif
// CIF = clips in flight: register-slot sets, clip c in set c % CIF, a clip's last rounds handed to the next walking clip OF ITS SET.
// 1: one stream, clip after clip (the product).  2 (cross-attention, M2M_MC_CIF=2): measured slower, see launch_dec_attn_mc_t.
template <typename T, bool SELF, bool NT, bool FETCH, int C, int CIF = 1, bool BEAM = false>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(M2M_MC_WAVES, M2M_MC_WAVES))) void dec_attn_mc_kernel(DecAttnArgs a, int nb) {
  static_assert(!BEAM || (CIF == 1 && !FETCH), "beam search: one clip in flight, not headless");
  static_assert(CIF == 1 || (CIF == 2 && !SELF && C % 2 == 0), "two clips in flight: cross-attention, an even clip count");
  static_assert(!FETCH || SELF, "only the layer-0 self-attention fetches its input row from the embedding table");
  static_assert(C >= 2 && C <= 8, "a wave pair normalises one clip's row: at most 8 clips per 16-wave workgroup");
  constexpr int E = 16 / sizeof(T);
  constexpr int LPR = DK / E;
  constexpr int KPW = 64 / LPR;
  constexpr int KPB = 16 * KPW;
  constexpr int NOUT = DK;
  constexpr int LPO = 16;
  constexpr int LPO2 = 8;
  constexpr int WMAX2 = 6;
  constexpr int PF = SELF ? M2M_MC_PF_SELF : M2M_MC_PF_CROSS;
  constexpr int WMAX = 3;
  constexpr int GPW = 64 / LPR;
  using V16 = decltype(Vec16<T>().v);
  extern __shared__ __align__(16) float hn[];   // [C][d] normalised input rows (already rounded to T), then (self) the bias row
  __shared__ float redw[16], redl[16], redlf[16];
  __shared__ float redo[16][DK];
  __shared__ __align__(16) float redg[16 * GPW][DK];
  __shared__ __align__(16) float qs[C][DK];
  __shared__ __align__(16) float kn[SELF ? C : 1][DK];
  __shared__ __align__(16) float vn[SELF ? C : 1][DK];
  __shared__ __align__(16) float oh[C][DK];
  __shared__ __align__(16) xq_t xrow[C][512];    // the fixed-point input rows (d_model <= 512): head 0 adds them into x_out at the end
  const int st_t = a.state->t;
  const int st_done = a.state->done | (st_t >= a.state->max_steps);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hh = blockIdx.x, b0 = blockIdx.y * C;      // linear id = 8 * block + h: a head's workgroups on one XCD, as in the first kernel
  // finished-row flags of the C clips (scalar loads, requested with the loop state) as a bit mask; clips past the chain's end are
  // clamped onto its last clip for every load and never stored
  unsigned finmask = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) finmask |= (a.fin_skip[(int64_t)min(b0 + c, nb - 1) * a.fin_stride] != 0 ? 1u : 0u) << c;
  const int sub = lane % LPR;
  const int kslot = wave * KPW + lane / LPR;
  const int64_t kv_clip = (int64_t)a.H * a.kv_stride * DK;                       // elements between two clips' blocks
  // beam cross-attention: row b0 + c reads the K/V block of clip (b0 + c) / beam_nb (kb0 = the first one's)
  const int kb0 = (BEAM && !SELF) ? b0 / a.beam_nb : b0;
  T* const Kb0 = reinterpret_cast<T*>(a.Kc) + ((int64_t)kb0 * a.H + hh) * a.kv_stride * DK;
  T* const Vb0 = reinterpret_cast<T*>(a.Vc) + ((int64_t)kb0 * a.H + hh) * a.kv_stride * DK;

  // ---- 0. requests for the prologue.  Wave pair cl = wave / 2 owns clip cl's row: wave 2 cl holds its elements 0..255, wave
  //         2 cl + 1 the rest - the lane -> element map and the reduction tree of the first kernel's waves 0 and 1 ----
  const int cl = wave >> 1, tin = (wave & 1) * 64 + lane;
  const int xc = min(tin * 4, a.d - 4);
  const int bx = min(b0 + min(cl, C - 1), nb - 1);
  const bool own_wave = cl < C && (wave & 1) * 256 < a.d;      // wave-uniform
  const bool own = cl < C && tin * 4 < a.d;
  const int on_ = min(tid >> 1, a.d - 1), opart = tid & 1;
  longlong2 xr0 = make_longlong2(0, 0), xr1 = make_longlong2(0, 0);
  unsigned long long kraw = 0;
  int fin0 = 0;
  if constexpr (FETCH) {
    kraw = a.keys[bx];
    fin0 = a.finished[bx];
  } else {
    xr0 = *reinterpret_cast<const longlong2*>(a.x + (int64_t)bx * a.d + xc);
    xr1 = *reinterpret_cast<const longlong2*>(a.x + (int64_t)bx * a.d + xc + 2);
  }
  const float4 gv = *reinterpret_cast<const float4*>(a.ln_w + xc);
  __builtin_amdgcn_sched_barrier(0);               // the latency-critical rows go out FIRST (loads retire in order)
  const int po = min(tid / LPO, NOUT - 1), part = tid % LPO;
  const int which = po / DK, dd = po - which * DK;
  const T* wrow = reinterpret_cast<const T*>(a.Wp) + ((int64_t)which * a.inner + hh * DK + dd) * a.d;
  const int cnt = a.d / E / LPO;
  Vec16<T> w[WMAX];
#pragma unroll
  for (int u = 0; u < WMAX; ++u) w[u].v = *reinterpret_cast<const V16*>(wrow + (min(u, cnt - 1) * LPO + part) * E);
  // self: the weights of the k,v rows this step appends (128 outputs x 8 lanes) are part of the prologue here
  const int o2 = tid >> 3, part2 = tid & 7;
  const int which2 = 1 + (o2 >> 6), dd2 = o2 & 63;
  const T* wrow2 = reinterpret_cast<const T*>(a.Wp) + ((int64_t)which2 * a.inner + hh * DK + dd2) * a.d;
  const int cnt2 = a.d / E / LPO2;
  float* const biasl = hn + C * a.d;                   // [kv_stride] (self only): ONE bias row serves the C clips
  constexpr int BPT = 2;
  float bv[SELF ? BPT : 1];
  if (SELF) {
#pragma unroll
    for (int u = 0; u < BPT; ++u) bv[u] = a.bias[(int64_t)hh * a.bias_stride + min(tid + 1024 * u, a.bias_stride - 1)];
  }
  const int t = SELF ? (a.self_len_override > 0 ? a.self_len_override - 1 : st_t) : 0;
  const int n_prev = SELF ? t : a.n_keys;
  const int last = max(n_prev - 1, 0);
  // a clip's rounds, padded to a multiple of the prefetch depth (the padding rounds re-read its last key row and visit nothing), so
  // that a clip always starts in register slot 0 and its last PF rounds can re-request into the next clip slot for slot
  const int rpc = ((n_prev + KPB - 1) / KPB + PF - 1) / PF * PF;
  // clips that walk keys at all: live rows of this chain with at least one cached key
  unsigned walk = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) walk |= ((n_prev > 0 && !((finmask >> c) & 1u) && b0 + c < nb) ? 1u : 0u) << c;
  if (M2M_MC_ABL & 2) walk = 0;

  // The stream goes through buffer loads: one descriptor per operand for this workgroup's C clips (wave-uniform: built from the
  // kernel arguments and blockIdx only), the clip as the scalar offset, a 32-bit byte offset per lane - one address register per
  // slot serves K and V (with flat 64-bit addresses the compiler kept a register PAIR per load and slot alive across the loop:
  // 2 x 2 x PF registers, which is what limited the depth of the window).
  const unsigned clip_bytes = (unsigned)(kv_clip * (int64_t)sizeof(T));
  // BEAM: the descriptors start at the first block any of the C rows reads - its clip (cross) or its clip's beam 0 (self: every
  // ancestor row) - and end with the last one; a row's block inside them is cb(c) (cross) / its ancestry (self)
  const int last_row = min(b0 + C, nb) - 1;
  const int lo_blk = !BEAM ? b0 : (SELF ? b0 / a.beam_nb * a.beam_nb : kb0);
  const int hi_blk = !BEAM ? last_row : (SELF ? (last_row / a.beam_nb + 1) * a.beam_nb - 1 : last_row / a.beam_nb);
  auto cb = [&](int c) -> unsigned {       // byte offset of row b0 + c's own block (cross: its clip's) from the descriptors' base
    if constexpr (BEAM && !SELF) return (unsigned)(min(b0 + c, nb - 1) / a.beam_nb - kb0) * clip_bytes;
    else return (unsigned)c * clip_bytes;
  };
  T* const Kd0 = (BEAM && SELF) ? reinterpret_cast<T*>(a.Kc) + ((int64_t)lo_blk * a.H + hh) * a.kv_stride * DK : Kb0;
  T* const Vd0 = (BEAM && SELF) ? reinterpret_cast<T*>(a.Vc) + ((int64_t)lo_blk * a.H + hh) * a.kv_stride * DK : Vb0;
  const unsigned span_bytes = (BEAM ? (unsigned)(hi_blk - lo_blk) : (unsigned)(min(C, nb - b0) - 1)) * clip_bytes +
                              (unsigned)(a.kv_stride * DK * (int)sizeof(T));
  const __amdgpu_buffer_rsrc_t rK = __builtin_amdgcn_make_buffer_rsrc(Kd0, 0, (int)span_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rV = __builtin_amdgcn_make_buffer_rsrc(Vd0, 0, (int)span_bytes, 0x00020000);
  // BEAM self: the C rows' ancestries to LDS before the first request (they address it); entries clamped into the clip
  unsigned char* const ancl = reinterpret_cast<unsigned char*>(hn + C * a.d + (SELF ? a.bias_stride : 0));   // [C][kv_stride]
  if constexpr (BEAM && SELF) {
    const int na = min(max(st_t, 1), a.kv_stride);
    for (int i = tid; i < C * na; i += 1024) {
      const int c = i / na, j = i - c * na;
      const int r = min(b0 + c, nb - 1);
      const int v = j < st_t ? min((int)a.anc[(int64_t)(st_t & 1) * a.anc_par + (int64_t)r * a.anc_ld + j], a.beam_nb - 1) : r % a.beam_nb;
      ancl[c * a.kv_stride + j] = (unsigned char)(r / a.beam_nb * a.beam_nb - lo_blk + v);    // the block, relative to the base
    }
    __syncthreads();
  }
  // (lane offset, scalar offset) of this lane's part of key row `key` (clamped) of row b0 + c
  auto kvo = [&](int c, int key, int subc, unsigned& voff, unsigned& soff) {
    voff = (unsigned)((key * DK + subc * E) * (int)sizeof(T));
    if constexpr (BEAM && SELF) { voff += (unsigned)ancl[c * a.kv_stride + key] * clip_bytes; soff = 0u; }
    else soff = cb(c);
  };
  auto kvload = [](__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(V16, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, NT ? 2 : 0));   // aux 2 = nt
  };
  // the first walking clip's first PF rounds, right behind the prologue's own loads (clamped addresses, never predicated; when
  // no clip walks this is clip 0's last row once more - dropped)
  constexpr unsigned SETBITS = CIF == 1 ? 0xFFFFFFFFu : 0x55555555u;      // the clips of set 0
  Vec16<T> kv[CIF][PF], vv[CIF][PF];
#pragma unroll
  for (int st = 0; st < CIF; ++st) {
    const unsigned mine = walk & (SETBITS << st);
    // a set without a walking clip re-reads a clip of the workgroup (dropped), never one past the chain's end: that lies outside the
    // descriptors' span, and their range check sees the lane offset only, not the clip's scalar offset (clip 0 always exists)
    const int c_first = mine ? __builtin_ctz(mine) : (st == 0 ? 0 : min(st, min(C, nb - b0) - 1));
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      if constexpr (BEAM) {
        unsigned off, so;
        kvo(c_first, min(kslot + u * KPB, last), sub, off, so);
        kv[st][u].v = kvload(rK, off, so);
        vv[st][u].v = kvload(rV, off, so);
      } else {
        const unsigned off = (unsigned)((min(kslot + u * KPB, last) * DK + sub * E) * (int)sizeof(T));
        kv[st][u].v = kvload(rK, off, (unsigned)c_first * clip_bytes);
        vv[st][u].v = kvload(rV, off, (unsigned)c_first * clip_bytes);
      }
    }
  }
  __builtin_amdgcn_sched_barrier(0);

  // ---- 1. RMSNorm of the C rows -> hn[c] (rounded to the GEMM-input type T) ----
  float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (FETCH) {
    const int tok = amax_key_token(kraw, fin0, a.V, a.pad_id);
    e4 = *reinterpret_cast<const float4*>(a.emb + (int64_t)tok * a.d + xc);
  }
  if (own_wave) {
    if constexpr (FETCH) xv = e4;
    else xv = make_float4(xq_flt(xr0.x), xq_flt(xr0.y), xq_flt(xr1.x), xq_flt(xr1.y));
    float ss = own ? (xv.x * xv.x + xv.y * xv.y + xv.z * xv.z + xv.w * xv.w) : 0.f;
    ss = wave_sum(ss);
    if (lane == 0) redw[wave] = ss;
  } else if (lane == 0) {
    redw[wave] = 0.f;
  }
  __syncthreads();
  if (own && hh == 0) {     // (hh: uniform) the raw row for head 0's residual carry; an embedding row is converted as the first kernel does
    if constexpr (FETCH) {
      if (!st_done) {
        xr0 = make_longlong2(xq_fix_guarded(xv.x, a.state), xq_fix_guarded(xv.y, a.state));
        xr1 = make_longlong2(xq_fix_guarded(xv.z, a.state), xq_fix_guarded(xv.w, a.state));
      }
    }
    *reinterpret_cast<longlong2*>(&xrow[cl][xc]) = xr0;
    *reinterpret_cast<longlong2*>(&xrow[cl][xc + 2]) = xr1;
  }
  if (own) {
    // the first kernel sums its 16 wave slots in order, 14 of them zeros: 0 + r0 + r1 (+ 0 ...) - the same two adds
    float tot = 0.f;
    tot += redw[2 * cl];
    tot += redw[2 * cl + 1];
    const float rs = rsqrtf(tot / (float)a.d + a.eps);
    float* const hc = hn + cl * a.d;
    put_in<T>(hc, xc + 0, gv.x * (xv.x * rs));
    put_in<T>(hc, xc + 1, gv.y * (xv.y * rs));
    put_in<T>(hc, xc + 2, gv.z * (xv.z * rs));
    put_in<T>(hc, xc + 3, gv.w * (xv.w * rs));
  }
  __syncthreads();

  // ---- 2. this head's projections of the C rows: the weights are in registers once ----
  {   // (da_project<T, C, LPO>, by hand: called, the cross form at S = 864 read 31.28 us per launch against the parent's 31.13-31.25)
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
#pragma unroll
    for (int u = 0; u < WMAX; ++u) {
      if (u < cnt) {
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = chunk_dot<T>(w[u], hn + c * a.d, u * LPO + part, acc[c]);
      }
    }
    for (int i = WMAX; i < cnt; i += 4) {   // d_model / dtype combinations beyond the register budget (fp32)
      Vec16<T> w2[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) w2[u].v = *reinterpret_cast<const V16*>(wrow + (min(i + u, cnt - 1) * LPO + part) * E);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (i + u < cnt) {
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c] = chunk_dot<T>(w2[u], hn + c * a.d, (i + u) * LPO + part, acc[c]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float q = group_sum<LPO>(acc[c]);
      if (part == 0 && tid < NOUT * LPO) qs[c][dd] = q;      // q stays fp32
    }
  }
  if (SELF) {
    // the k,v rows of this step: projected, rounded to T, appended to the cache and kept in LDS for the clips' own-key visits.
    // Their weights are requested only now, into the registers the q weights have left (one more L2 round trip in this workgroup's
    // chain; only the M2M_MC_WAVES = 8 build, 64 registers, has a co-resident workgroup to fill it: the product build, 4 waves per
    // SIMD and 128 registers, runs ONE workgroup per CU)
    Vec16<T> wkv[WMAX2];
#pragma unroll
    for (int u = 0; u < WMAX2; ++u) wkv[u].v = *reinterpret_cast<const V16*>(wrow2 + (min(u, cnt2 - 1) * LPO2 + part2) * E);
    float kvn[C];
    da_project<T, C, LPO2>(kvn, wkv, wrow2, cnt2, part2, hn, a.d);
    if (part2 == 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) da_append_kv<T>(kvn[c], c, which2, dd2, t, kv_clip, Kb0, Vb0, &kn[0][0], &vn[0][0], !st_done && b0 + c < nb);
    }
#pragma unroll
    for (int u = 0; u < BPT; ++u)
      if (tid + 1024 * u < a.bias_stride) biasl[tid + 1024 * u] = bv[u];
    for (int n = tid + 1024 * BPT; n < a.bias_stride; n += 1024) biasl[n] = a.bias[(int64_t)hh * a.bias_stride + n];
  }
  __syncthreads();

  // ---- 3. the clips' streams, one after the other ----
#pragma nounroll
  for (int c0 = 0; c0 < C; c0 += CIF) {
#pragma unroll
  for (int st = 0; st < CIF; ++st) {
    const int c = c0 + st;
    const bool walks = (walk >> c) & 1u;                                          // uniform
    const unsigned cbase = BEAM ? cb(c) : (unsigned)c * clip_bytes;   // this clip inside the descriptors (an invalid tail clip walks nothing)
    // per-clip OPAQUE copies of the lane's place in a round: derived from threadIdx the hand-over offsets below are loop invariants
    // that the compiler keeps from the prologue, spills (at the 64 registers of the M2M_MC_WAVES = 8 build), and reloads in the middle of the stream - and a scratch
    // reload waits vmcnt(0), i.e. for every round in flight
    int kslot_c = kslot, sub_c = sub;
    asm volatile("" : "+v"(kslot_c), "+v"(sub_c));
    const int n_live = walks ? n_prev : 0;
    float qv[E];
#pragma unroll
    for (int e = 0; e < E; ++e) qv[e] = qs[c][sub * E + e];
    // (DaSoftmax, by hand: as the struct, the fp32 cross form read 20.37 us per launch against the parent's 20.24-20.34)
    float m_run = -1e30f, l_run = 0.f;
    float acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
    auto visit = [&](float s, const float (&vrow)[E]) {
      const bool up = s > m_run;
      const float m_new = up ? s : m_run;
      const float ex = m2m_exp<T>(up ? m_run - s : s - m_run);
      const float alpha = up ? ex : 1.f;
      const float p = up ? 1.f : ex;
      l_run = fmaf(l_run, alpha, p);
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = fmaf(acc[e], alpha, p * vrow[e]);
      m_run = m_new;
    };
    // consume slot u (round k0 / KPB + u of this clip); then re-request into it: mode 1 = this clip's round PF ahead, mode 2 = round u
    // of the clip `nxt` elements further on (the next walking clip), mode 0 = nothing.  The mode is a compile-time constant per loop,
    // so every load is unconditional and counted (s_waitcnt vmcnt(N) keeps the other slots in flight).
    auto round = [&](const int k0, const int u, Vec16<T>& ks, Vec16<T>& vs, const int mode, const unsigned nxt) {
      const int key = k0 + kslot_c + u * KPB;
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) s = fmaf(qv[e], ks.get(e), s);
      s = group_sum<LPR>(s);
      if (key < n_live) {   // VALU-only predicate
        float vrow[E];
#pragma unroll
        for (int e = 0; e < E; ++e) vrow[e] = vs.get(e);
        if (SELF) s += biasl[t - key];
        visit(s, vrow);
      }
      // the slot is re-requested AFTER it has been consumed: with the request in front of the visit (the first kernel's order) the
      // compiler sinks V's unpacking into the predicated block, keeps the packed V alive past the request, loads into a SECOND
      // register set and copies it back behind a vmcnt(0) at the end of every iteration (seen in the ISA at PF = 4: the window
      // became batches)
      if (BEAM && SELF && mode == 1) {
        unsigned off, so;
        kvo(c, min(key + PF * KPB, last), sub_c, off, so);
        ks.v = kvload(rK, off, so);
        vs.v = kvload(rV, off, so);
      } else if (BEAM && SELF && mode == 2) {    // nxt: the next walking clip's index, or the out-of-range marker
        const bool oob = nxt >= 0x7F000000u;
        unsigned off = nxt, so = 0u;
        if (!oob) kvo((int)nxt, min(kslot_c + u * KPB, last), sub_c, off, so);
        ks.v = kvload(rK, off, so);
        vs.v = kvload(rV, off, so);
      } else if (mode == 1) {
        const unsigned off = (unsigned)((min(key + PF * KPB, last) * DK + sub_c * E) * (int)sizeof(T));
        ks.v = kvload(rK, off, cbase);
        vs.v = kvload(rV, off, cbase);
      } else if (mode == 2) {
        // (nxt < 2^31: a clip's byte offset goes into the scalar offset; otherwise it is the out-of-range marker and goes into the
        // lane offset, the only part the range check looks at)
        const unsigned off = (unsigned)((min(kslot_c + u * KPB, last) * DK + sub_c * E) * (int)sizeof(T));
        const bool oob = nxt >= 0x7F000000u;                 // uniform
        ks.v = kvload(rK, oob ? nxt : off, oob ? 0u : nxt);
        vs.v = kvload(rV, oob ? nxt : off, oob ? 0u : nxt);
      }
    };
    if (walks) {
      const int kend = rpc * KPB;
      int k0 = 0;
      for (; k0 + PF * KPB < kend; k0 += PF * KPB) {           // every re-request lies inside this clip's (padded) rounds
#pragma unroll
        for (int u = 0; u < PF; ++u) round(k0, u, kv[st][u], vv[st][u], 1, 0);
      }
      // the clip's last PF rounds hand their slots to the next walking clip, so the stream runs through the merge below.  After the
      // LAST walking clip the same loads are issued with a lane offset beyond the descriptor's range: the hardware's range check
      // drops them (zeros, no memory access) - one code path, so the slots stay in ONE register set (with a second, load-free path
      // for the last clip the register allocator kept a second set of 8 PF registers for the handed-over rounds and copied it back)
      const unsigned rest = (walk >> (c + CIF)) & SETBITS;                     // later walking clips of this set
      unsigned nxt;
      if constexpr (BEAM && SELF) nxt = rest ? (unsigned)(c + __builtin_ctz(rest) + CIF) : 0x7F000000u;
      else if constexpr (BEAM) nxt = rest ? cb(c + __builtin_ctz(rest) + CIF) : 0x7F000000u;
      else nxt = rest ? cbase + (unsigned)(__builtin_ctz(rest) + CIF) * clip_bytes : 0x7F000000u;
#pragma unroll
      for (int u = 0; u < PF; ++u) round(k0, u, kv[st][u], vv[st][u], 2, nxt);
    }
    if (SELF && wave == 0 && lane < LPR) {   // the key/value appended this step (relative position 0): group 0
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) s = fmaf(qv[e], kn[c][sub * E + e], s);
      s = group_sum<LPR>(s);
      s += biasl[0];
      float vrow[E];
#pragma unroll
      for (int e = 0; e < E; ++e) vrow[e] = vn[c][sub * E + e];
      visit(s, vrow);
    }
    // ---- merge of the 128 key groups (da_merge, by hand: called, the bf16 self form read 18.30 us per launch against the parent's
    //      18.15-18.22) ----
    {
      const float mw = wave_max(m_run);
      const float scale = m2m_exp<T>(m_run - mw);
      float lsum = (sub == 0) ? l_run * scale : 0.f;
      lsum = wave_sum(lsum);
      float* gp = &redg[wave * GPW + lane / LPR][sub * E];
#pragma unroll
      for (int e = 0; e < E; e += 4)
        *reinterpret_cast<float4*>(gp + e) = make_float4(acc[e] * scale, acc[e + 1] * scale, acc[e + 2] * scale, acc[e + 3] * scale);
      if (lane == 0) { redw[wave] = mw; redl[wave] = lsum; }
      __syncthreads();
      {
        float M = redw[lane & 15];
        M = fmaxf(M, lane_xor<8>(M)); M = fmaxf(M, lane_xor<4>(M)); M = fmaxf(M, lane_xor<2>(M)); M = fmaxf(M, lane_xor<1>(M));
        const float fw = m2m_exp<T>(redw[wave] - M);
        float sw = redg[wave * GPW][lane];
#pragma unroll
        for (int j = 1; j < GPW; ++j) sw += redg[wave * GPW + j][lane];
        redo[wave][lane] = sw * fw;
        if (lane == 0) redlf[wave] = redl[wave] * fw;
      }
      __syncthreads();
      if (tid < DK) {
        float s = 0.f, L = 0.f;
#pragma unroll
        for (int wv = 0; wv < 16; ++wv) {
          s += redo[wv][tid];
          L += redlf[wv];
        }
        put_in<T>(oh[c], tid, !(L <= 0.f) ? s / L : 0.f);   // NaN stays NaN for the range guard (see dec_attn_kernel)
      }
      __syncthreads();
    }
  }   // clips of a trip (sets)
  }

  // ---- 4. output projections of this head, accumulated into the C residual rows (the slice of wo is requested only here: 16 / 32
  //         registers that would otherwise be held through every stream).  da_out_row, by hand: called, the bf16 self form read
  //         18.23 us per launch against the parent's 18.15-18.22 ----
  constexpr int OCH = 32 / E;
  // (step image: load u of the workgroup's 2 d live threads is 2 d x 16 consecutive bytes; the threads past them re-read the last chunk)
  const T* woimg = reinterpret_cast<const T*>(a.Wo) + ((int64_t)hh * OCH * 2 * a.d + min(tid, 2 * a.d - 1)) * E;
  Vec16<T> wo[OCH];
#pragma unroll
  for (int u = 0; u < OCH; ++u) wo[u].v = *reinterpret_cast<const V16*>(woimg + (int64_t)u * 2 * a.d * E);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int bc = min(b0 + c, nb - 1);
    float accp = 0.f;
#pragma unroll
    for (int u = 0; u < OCH; ++u) accp = chunk_dot<T>(wo[u], oh[c], opart * OCH + u, accp);
    accp += lane_xor<1>(accp);
    if (opart == 0 && tid < 2 * a.d && !st_done && b0 + c < nb) {
      xq_t add = xq_fix_guarded(accp, a.state);
      if (hh == 0) add += xrow[c][on_];                 // head 0 also carries the residual itself (kept in LDS since the prologue)
      if (!(M2M_MC_ABL & 1) || hh == 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(a.x_out + (int64_t)bc * a.d + on_), (unsigned long long)add);
      if (hh == a.H - 1) a.x_zero[(int64_t)bc * a.d + on_] = 0;
    }
  }
  if (!SELF && a.book && hh == 0 && tid == 0) {
    // headless bookkeeping of the C rows (da_book_row, by hand: called, the fp32 cross form read 21.83 us per launch against the
    // parent's 21.66-21.71 - eight bytes of code, another schedule of the q projection)
    for (int c = 0; c < C && b0 + c < nb; ++c) {
      const int b = b0 + c;
      if (!st_done) {
        const int fin = a.finished[b];
        const int next = amax_key_token(a.keys[b], fin, a.V, a.pad_id);
        if (st_t < a.max_len) a.tokens[(int64_t)a.tok_row[b] * a.max_len + st_t] = next;
        const int nf = fin | (next == a.eos_id);
        a.finished[b] = nf;
        if (!nf) atomicAdd(&a.state->n_unfinished, 1);
        a.keys[b] = 0ull;
      }
      if (b == 0) a.state->t_copy = st_t;
    }
  }
}

// The (beam, headless, self, nt) decision tree of both attention kernels: launch(SELF, NT, FETCH, BEAM), each a std::bool_constant.
template <typename F>
static void launch_dec_attn_form(bool self, bool nt, const DecAttnArgs& a, F launch) {
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  auto by_nt = [&](auto s, auto fetch, auto beam) {
    if (nt) launch(s, yes, fetch, beam);
    else launch(s, no, fetch, beam);
  };
  if (a.beam_nb > 0) {          // beam search: ancestry reads (self) / a clip's K/V shared by its beams (cross)
    if (self) by_nt(yes, no, yes);
    else by_nt(no, no, yes);
  } else if (self && a.emb) {   // headless layer 0
    by_nt(yes, yes, no);
  } else if (self) {
    by_nt(yes, no, no);
  } else {
    by_nt(no, no, no);
  }
}

// (tab: the token-table form of the layer-0 self-attention, 0 / 1 / 2 - decode_launch_attn decides)
template <typename T>
static void launch_dec_attn_t(bool self, bool nt, int tab, const DecAttnArgs& a, dim3 grid, size_t smem, hipStream_t st) {
  launch_dec_attn_form(self, nt, a, [&](auto s, auto n, auto f, auto bm) {
    if constexpr (f.value) {
      if (tab == 1) { hipLaunchKernelGGL((dec_attn_kernel<T, true, n.value, true, false, 1>), grid, dim3(1024), smem, st, a); return; }
      if (tab == 2) { hipLaunchKernelGGL((dec_attn_kernel<T, true, n.value, true, false, 2>), grid, dim3(1024), smem, st, a); return; }
    }
    hipLaunchKernelGGL((dec_attn_kernel<T, s.value, n.value, f.value, bm.value>), grid, dim3(1024), smem, st, a);
  });
}

// several clips per workgroup (dec_attn_mc_kernel): C = 2 or 4
template <typename T, int C>
static void launch_dec_attn_mc_t(bool self, bool nt, const DecAttnArgs& a, int nb, int cif, size_t smem, hipStream_t st) {
  const dim3 grid((unsigned)a.H, (unsigned)ceil_div(nb, C));
  // M2M_MC_CIF=2 (diagnostic, latched per session): two clips in flight in the cross-attention.  At S = 190 a clip's whole stream is
  // one round trip, so the kernel is C dependent round trips long and two register-slot sets overlap them - on paper 14 -> ~10.5 us
  // per launch; measured on one box (tools/native_mc_sweep.py, us per step, one / two in flight): 2 x 64 clips bf16 340.6 / 338.9
  // against 351.4 / 350.9, fp32 577.2 against 591.9, 2 x 32 clips 220.4 against 226.6, 2 x 64 at S = 864 480.9 against 485.0.  One
  // in flight.  (Beam search: one clip in flight whatever M2M_MC_CIF says.)
  launch_dec_attn_form(self, nt, a, [&](auto s, auto n, auto f, auto bm) {
    if constexpr (!s.value && !bm.value) {     // short cross streams (a clip's keys fit the prefetch window): two clips in flight
      if (cif == 2) {
        hipLaunchKernelGGL((dec_attn_mc_kernel<T, false, n.value, false, C, 2>), grid, dim3(1024), smem, st, a, nb);
        return;
      }
    }
    hipLaunchKernelGGL((dec_attn_mc_kernel<T, s.value, n.value, f.value, C, 1, bm.value>), grid, dim3(1024), smem, st, a, nb);
  });
}

static int launch_dec_attn(int precision, bool self, bool nt, int tab, DecAttnArgs a, int B, int clips, int cif, hipStream_t st) {
  size_t smem = ((size_t)a.d * (size_t)clips + (self ? (size_t)a.bias_stride : 0)) * sizeof(float);   // hn rows + (self) the bias row
  if (self && a.beam_nb > 0) smem += (size_t)clips * a.kv_stride;         // + the rows' ancestries (a byte per position)
  M2M_REQUIRE(tab == 0 || (self && clips == 1 && a.beam_nb == 0 && a.emb && a.q0_tab && a.k0_tab && a.v0_tab && a.tokens && a.tok_row),
              "decode attention: the token-table form %d needs the one-clip headless layer-0 self-attention, the model's tables and the row's tokens", tab);
  if (tab == 2) smem += ((size_t)a.kv_stride * 2 + 3) / 4 * 4;            // + the row's token history (16 bits per position)
  M2M_REQUIRE(smem <= 24 * 1024, "decode attention: max_dec_len=%d too long for the LDS bias row%s (<= %d)", a.bias_stride,
              self && a.beam_nb > 0 ? " and ancestries" : "",
              (24 * 1024 - a.d * 4 * clips) / (self && a.beam_nb > 0 ? 4 + clips : 4));
  const bool bf = precision == M2M_PREC_BF16;
  if (clips == 1) {
    dim3 grid((unsigned)a.H, (unsigned)B);
    if (bf) launch_dec_attn_t<bf16_t>(self, nt, tab, a, grid, smem, st);
    else launch_dec_attn_t<float>(self, nt, tab, a, grid, smem, st);
  } else if (clips == 2) {
    if (bf) launch_dec_attn_mc_t<bf16_t, 2>(self, nt, a, B, cif, smem, st);
    else launch_dec_attn_mc_t<float, 2>(self, nt, a, B, cif, smem, st);
  } else if (clips == 4) {
    if (bf) launch_dec_attn_mc_t<bf16_t, 4>(self, nt, a, B, cif, smem, st);
    else launch_dec_attn_mc_t<float, 4>(self, nt, a, B, cif, smem, st);
  } else {
    set_error("decode attention: %d clips per workgroup not instantiated (1, 2, 4)", clips);
    return M2M_ERR_INVALID;
  }
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

// ================================================================== head ====
struct DecHeadArgs {
  const float* logits;     // [B, ldl]
  int ldl, V, B, d;
  const float* shared;     // [V, d] embedding
  xq_t* x;                 // [B, d] next-step input (fixed-point residual stream, buffer A)
  xq_t* x_zero;            // [B, d] buffer B: zeroed by the init kernel (later by every FFN down projection)
  int64_t* tokens;         // [session rows, max_len] generated ids (col 0 = start): the whole matrix, row of slot b = tok_row[b]
  int* tok_row;            // [B] (chain view) clip decoded in slot b; written by the init kernel (identity: row0 + b)
  int row0;                // first slot of this chain in the session
  int max_len;
  int* finished;           // [B]
  unsigned long long* keys;// [B] (headless greedy loop; null otherwise)
  DecState* state;
  int pad_id, eos_id;
  // teacher forcing (nullptr for greedy)
  const int64_t* forced;   // [B, Ld] decoder input ids
  int Ld;
  float* logits_out;       // [B, Ld, V]
};

// 32 lanes per clip: with B <= 32 every row is handled concurrently (one pass of independent loads,
// then one dependent embedding fetch), so the kernel is two memory round trips long.
__global__ __launch_bounds__(1024) void dec_head_kernel(DecHeadArgs a) {
  __shared__ int s_unfinished;
  DecState* stp = a.state;
  M2M_STAMP_DECL
  M2M_STAMP(8, 0);
  const int t = stp->t;
  const int st_done = stp->done | (t >= stp->max_steps);
  const int tid = threadIdx.x, l32 = tid & 31, grp = tid >> 5;
  // first batch of logits of this lane group's first row: requested before the loop state is consumed
  constexpr int HK = 16;   // V <= 32 * HK columns are covered by the register batch (vocab 400 -> 13 used)
  float lg0[HK];
  {
    const float* lg = a.logits + (int64_t)min(grp, a.B - 1) * a.ldl;
#pragma unroll
    for (int j = 0; j < HK; ++j) lg0[j] = lg[min(l32 + 32 * j, a.V - 1)];
  }
  // no early exit on st_done (a branch here makes the compiler hoist the loop-state load in front of the logits
  // requests: two serial round trips; the state was written by this kernel one step ago, so it comes from HBM):
  // a finished chain runs the rest of its graph with every store below suppressed
  __builtin_amdgcn_sched_barrier(0);
  const bool live = !st_done;
  if (tid == 0) s_unfinished = 0;
  __syncthreads();
  for (int b = grp; b < a.B; b += 32) {
    const float* lg = a.logits + (int64_t)b * a.ldl;
    const int fin = a.forced ? 0 : a.finished[b];
    float best = -INFINITY;
    int bi = 0x7fffffff;
    bool bad = false;      // a non-finite logit (NaN weights ...): the reference would emit NaN logits, never a silent token
    if (b == grp) {
#pragma unroll
      for (int j = 0; j < HK; ++j) {
        const int v = l32 + 32 * j;
        const float x = lg0[j];
        if (v < a.V) bad |= !(fabsf(x) <= 3.0e38f);
        if (v < a.V && (x > best || (x == best && v < bi))) { best = x; bi = v; }
      }
    }
    for (int v = l32 + (b == grp ? 32 * HK : 0); v < a.V; v += 32) {
      const float x = lg[v];
      bad |= !(fabsf(x) <= 3.0e38f);
      if (x > best || (x == best && v < bi)) { best = x; bi = v; }
    }
    if (bad && live) stp->overflow = 1;
    auto take = [&](float ob, int oi) {
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    };
    // butterfly inside the 32-lane half (xor 16, 8, 4, 2, 1), LDS-free exchanges
    take(lane_xor<16>(best), __builtin_bit_cast(int, lane_xor<16>(__builtin_bit_cast(float, bi))));
    take(lane_xor<8>(best), __builtin_bit_cast(int, lane_xor<8>(__builtin_bit_cast(float, bi))));
    take(lane_xor<4>(best), __builtin_bit_cast(int, lane_xor<4>(__builtin_bit_cast(float, bi))));
    take(lane_xor<2>(best), __builtin_bit_cast(int, lane_xor<2>(__builtin_bit_cast(float, bi))));
    take(lane_xor<1>(best), __builtin_bit_cast(int, lane_xor<1>(__builtin_bit_cast(float, bi))));
    int next;
    if (a.forced) {
      if (a.logits_out && live)
        for (int v = l32; v < a.V; v += 32) a.logits_out[((int64_t)b * a.Ld + t) * a.V + v] = lg[v];
      next = (t + 1 < a.Ld) ? (int)a.forced[(int64_t)b * a.Ld + t + 1] : a.pad_id;
    } else {
      // hf generation/utils.py:2925-2937: argmax; finished rows emit pad; EOS finishes a row
      next = fin ? a.pad_id : (bi == 0x7fffffff ? 0 : bi);
      if (l32 == 0 && live) {
        if (t + 1 < a.max_len) a.tokens[(int64_t)a.tok_row[b] * a.max_len + t + 1] = next;
        const int nf = fin | (next == a.eos_id);
        a.finished[b] = nf;
        if (!nf) atomicAdd(&s_unfinished, 1);
      }
    }
    if (next < 0 || next >= a.V) next = a.pad_id;
    const float* emb = a.shared + (int64_t)next * a.d;
    for (int c = l32 * 4; c < a.d; c += 128) {
      const float4 e4 = *reinterpret_cast<const float4*>(emb + c);
      xq_t* xp = a.x + (int64_t)b * a.d + c;
      if (live) {
        *reinterpret_cast<longlong2*>(xp) = make_longlong2(xq_fix_guarded(e4.x, stp), xq_fix_guarded(e4.y, stp));
        *reinterpret_cast<longlong2*>(xp + 2) = make_longlong2(xq_fix_guarded(e4.z, stp), xq_fix_guarded(e4.w, stp));
      }
    }
  }
  __syncthreads();
  if (tid == 0 && live) {
    const int nt = t + 1;
    stp->t = nt;
    if (a.forced) {
      if (nt >= a.Ld) stp->done = 1;
    } else {
      stp->n_unfinished = s_unfinished;
      if (s_unfinished == 0 || nt >= stp->max_steps) { stp->done = 1; stp->out_len = nt + 1; }
    }
  }
  M2M_STAMP(8, 2);
}

__global__ void dec_init_kernel(DecHeadArgs a, int start_id, int max_steps) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  const int nthreads = gridDim.x * blockDim.x;
  if (tid == 0) {
    a.state->t = 0; a.state->done = (max_steps <= 0) ? 1 : 0; a.state->out_len = 1;
    a.state->n_unfinished = a.keys ? 0 : a.B; a.state->max_steps = max_steps; a.state->t_copy = 0;
  }
  for (int b = tid; b < a.B; b += nthreads) {
    a.finished[b] = 0;
    a.tok_row[b] = a.row0 + b;
    if (a.keys) a.keys[b] = amax_key(0.f, start_id);         // headless: step 0 "decodes" the start token
  }
  if (!a.forced) {
    int64_t* tk = a.tokens + (int64_t)a.row0 * a.max_len;
    for (int i = tid; i < a.B * a.max_len; i += nthreads) tk[i] = (i % a.max_len == 0) ? start_id : a.pad_id;
  }
  for (int i = tid; i < a.B * a.d; i += nthreads) {
    const int b = i / a.d, c = i - b * a.d;
    int tok = a.forced ? (int)a.forced[(int64_t)b * a.Ld] : start_id;
    if (tok < 0 || tok >= a.V) tok = a.pad_id;
    a.x[i] = xq_fix_guarded(a.shared[(int64_t)tok * a.d + c], a.state);
    a.x_zero[i] = 0;
  }
}

// after the loop: the last lm_head's keys are still pending (no later step consumed them) unless the chain ended on EOS
__global__ void dec_final_kernel(DecHeadArgs a) {
  DecState* st = a.state;
  const int t = st->t;
  if (st->done || !a.keys) return;
  for (int b = threadIdx.x; b < a.B; b += blockDim.x) {
    const int fin = a.finished[b];
    const int next = amax_key_token(a.keys[b], fin, a.V, a.pad_id);
    if (t < a.max_len) a.tokens[(int64_t)a.tok_row[b] * a.max_len + t] = next;
    a.finished[b] = fin | (next == a.eos_id);
  }
  __syncthreads();
  if (threadIdx.x == 0) { st->done = 1; st->out_len = t + 1; }
}

// =========================================================== select heads ====
// do_sample=True, the logits processors and the per-token outputs replace dec_head_kernel by dec_sample_kernel, dec_process_kernel
// or dec_scored_kernel (the step is otherwise the non-headless one, as with M2M_HEADLESS=0): one body, select_head, built from the
// helpers of this section; dec_beam_kernel shares the row load, the embedding write and the step close.  Sampling follows
// transformers 4.34's logits warpers in their order (hf: generation/utils.py _get_logits_warper, generation/logits_process.py):
//   TemperatureLogitsWarper  x / T (skipped for T == 1)
//   TopKLogitsWarper         remove every logit strictly below the k-th largest, k = min(top_k, V) (ties at the boundary stay)
//   TopPLogitsWarper         sorted ascending, remove the entries whose cumulative softmax is <= 1 - top_p, the largest always stays
// then draws from the softmax of what is left by inverse CDF over the vocabulary order with a uniform from a counter-based hash of
// (call seed, clip row tok_row[b], position t): a clip's ids do not depend on its slot, its chain or the kernel forms of the step.
// One wavefront per row (4 rows per workgroup, every row of the chain at once), the row in registers (lane l holds the NPL logits
// l*NPL ..), and no sort: the k-th largest logit is a radix select over the order-preserving 32-bit image of the logits (32
// ballot counts), the nucleus cutoff the largest key c whose strictly-smaller mass is <= (1 - top_p) * Z (32 wave-wide sums) - an
// entry is removed iff its cumulative mass, itself included, is <= (1 - top_p) * Z, i.e. iff its key is below c.  (Exact ties at
// the nucleus boundary are kept or removed together; HF removes them in torch.sort's order.)  Non-finite logits raise the chain's
// overflow flag (M2M_ERR_RANGE) as the greedy head does; the EOS / pad / finished bookkeeping, the token store and the embedding
// write are the greedy branch of dec_head_kernel.  The last workgroup of a step (a ticket in DecState) closes it.
// Per-token outputs (m2m_generate_scored): the processed head (with a neutral ProcessParams block when the call has no processor)
// also writes, for every live row, the fp32 row the token was selected from (HF's `scores`: raw, processed or warped logits, removed
// entries -inf) to scores[t][clip][0:V] and / or log_softmax(that row)[token] to logprobs[clip][t]: the row is in registers, so the
// log-probability costs one wave-wide max and sum and a 4-byte store, and the row itself is only written when asked for.  clip =
// tok_row[b]: the outputs follow the clip through live-row re-packing and chains of any size.  The output pointers come from the
// ScoreParams block of the workspace, so one captured graph serves every call.
static_assert(PROC_MAX_VOCAB == SAMPLE_MAX_VOCAB && SAMPLE_MAX_VOCAB == 64 * 64, "the register row: 64 lanes x at most 64 logits");
__device__ inline unsigned ord_key(float v) {
  unsigned u = __float_as_uint(v + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float wave_sum_uniform(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, wave_sum(v)))); }
constexpr int SAMPLE_ROWS = 4;   // rows (waves) per select-head workgroup: a chain's rows are spread over ceil(B / 4) workgroups
// this lane's NPL logits of a row (0 past V) -> x; true when one is not finite (the reference would emit NaN logits, never a token)
template <int NPL>
__device__ __forceinline__ bool load_row(const float* lg, int v0, int V, float (&x)[NPL]) {
  bool bad = false;
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    x[j] = (v0 + j < V) ? lg[v0 + j] : 0.f;
    bad |= !(fabsf(x[j]) <= 3.0e38f);
  }
  return bad;
}
template <int NPL>
__device__ inline unsigned long long lane_bits(const unsigned* w, int v0) {   // bits v0 .. v0 + NPL - 1 of a vocabulary bitmap
  if constexpr (NPL == 64) return (unsigned long long)w[v0 >> 5] | ((unsigned long long)w[(v0 >> 5) + 1] << 32);
  else return (w[v0 >> 5] >> (v0 & 31)) & ((1ull << NPL) - 1);
}
// Bits [lo, hi) of the vocabulary as they fall into this lane's ids v0 .. v0 + NPL - 1 (bit j = id v0 + j).
template <int NPL>
__device__ __forceinline__ unsigned long long lane_range_bits(int lo, int hi, int v0) {
  const int l = max(lo, v0) - v0, h = min(hi, v0 + NPL) - v0;
  if (h <= l) return 0ull;
  return (h - l >= 64 ? ~0ull : ((1ull << (h - l)) - 1)) << l;
}
// The per-lane body of the logits processors, shared by the select heads (apply_processors, on raw logits) and the processed beam
// head (dec_beam_kernel<NPL, true>, on log-probabilities): bit j of a mask is id v0 + j.  4.34's _get_logits_processor order:
// repetition (m_seen), n-gram and bad words (m_ban), min length, min new tokens, the token grammar (m_gram: PrefixConstrained-
// LogitsProcessor's place; one -inf set with the bans before it), forced BOS, forced EOS, suppress and begin-suppress (m_post).
template <int NPL>
__device__ __forceinline__ void apply_lane_processors(const ProcessParams* pp, float (&x)[NPL], int cur, int v0, int V, int eos_id,
                                                      unsigned long long m_seen, unsigned long long m_ban, unsigned long long m_gram,
                                                      unsigned long long m_post) {
  const float pen = pp->penalty;
  const bool eos_ban = cur < pp->min_length || cur - 1 < pp->min_new;
  const int fbos = cur == 1 ? pp->forced_bos : -1;
  const int feos = cur == pp->max_length - 1 ? pp->forced_eos : -1;
  // the processors after the penalty only write -inf or (the forced id) 0: they fold into two masks, in their order
  unsigned long long ninf = m_ban | m_gram | (eos_ban ? lane_range_bits<NPL>(eos_id, eos_id + 1, v0) : 0ull), zero = 0ull;
  if (fbos >= 0) { zero = lane_range_bits<NPL>(fbos, fbos + 1, v0); ninf = ~zero; }
  if (feos >= 0) { zero = lane_range_bits<NPL>(feos, feos + 1, v0); ninf = ~zero; }
  ninf |= m_post;
  zero &= ~m_post;
  ninf &= lane_range_bits<NPL>(0, V, v0);          // ids past the vocabulary keep their 0
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    if ((m_seen >> j) & 1) x[j] = x[j] < 0.f ? x[j] * pen : x[j] / pen;
    if ((ninf >> j) & 1) x[j] = -INFINITY;
    if ((zero >> j) & 1) x[j] = 0.f;
  }
}
// Logits processors (m2m_generate_processed; transformers 4.34 _get_logits_processor, see include/music2midi_amd.h) on the row in
// registers, before the select; every thread of the workgroup calls this (it holds barriers).  Per workgroup (4 rows) 16 KB of LDS
// hold the rows' histories (input_ids = the start token and t generated ids, cur = cur_len = t + 1) as 16-bit ids, staged from the
// token matrix (row tok_row[b]: the clip's own row whatever its slot), and 4 KB their bitmaps: one lane-strided pass each sets the
// "seen" bits (repetition penalty) and the ban bits (n-gram, bad words of two or more ids).  The ids that do not depend on the
// history (suppress, begin-suppress, one-id bad words) come as bitmaps of the parameter block.
// m_gram: the ids of this lane the token grammar bans (grammar_banned; 0 without it), applied where 4.34 puts
// PrefixConstrainedLogitsProcessor: after the two EOS bans, before forced BOS.
template <int NPL>
__device__ __forceinline__ void apply_processors(const DecHeadArgs& a, const ProcessParams* pp, float (&x)[NPL], int b, bool row,
                                                 bool live, int cur, int v0, unsigned long long m_gram) {
  __shared__ unsigned short s_hist[SAMPLE_ROWS][PROC_MAX_LEN];
  __shared__ unsigned s_bits[SAMPLE_ROWS][2][PROC_BITS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long m_seen = 0, m_ban = 0, m_post = 0;
  unsigned short* hist = s_hist[wave];
  unsigned *seen = s_bits[wave][0], *ban = s_bits[wave][1];
  bool scan = row && live && cur <= PROC_MAX_LEN && !a.finished[b];   // a finished row emits pad whatever its scores
  // no processor that looks at the history or at a bitmap (scores or the grammar over a neutral block, min_length alone): nothing to stage
  scan = scan && (pp->penalty != 1.0f || pp->ngram > 0 || pp->n_bad > 0 || pp->has_bad1 || pp->has_supp || pp->has_begin);
  for (int i = lane; i < PROC_BITS; i += 64) { seen[i] = 0u; ban[i] = 0u; }
  if (scan) {
    const int64_t* hr = a.tokens + (int64_t)a.tok_row[b] * a.max_len;
    for (int p = lane; p < cur; p += 64) hist[p] = (unsigned short)min((unsigned long long)hr[p], (unsigned long long)(PROC_MAX_VOCAB - 1));
  }
  __syncthreads();
  if (scan) {
    if (pp->penalty != 1.0f)
      for (int p = lane; p < cur; p += 64) atomicOr(&seen[hist[p] >> 5], 1u << (hist[p] & 31));
    // NoRepeatNGram: every complete window i .. i + n - 1 whose first n - 1 ids equal the last n - 1 ids bans its last id
    const int n = pp->ngram;
    if (n > 0) {
      const int pre = cur - n + 1;
      for (int i = lane; i + n <= cur; i += 64) {
        int k = 0;
        while (k < n - 1 && hist[i + k] == hist[pre + k]) ++k;
        if (k == n - 1) atomicOr(&ban[hist[i + n - 1] >> 5], 1u << (hist[i + n - 1] & 31));
      }
    }
    // NoBadWords (sequences of L >= 2 ids): the last id is banned when the history ends with the other L - 1; a sequence longer
    // than the history is skipped (4.34's SequenceBiasLogitsProcessor)
    for (int q = lane; q < pp->n_bad; q += 64) {
      const int o = pp->bad_off[q], L = pp->bad_off[q + 1] - o;
      if (L > cur) continue;
      int k = 0;
      while (k < L - 1 && (int)hist[cur - L + 1 + k] == pp->bad_ids[o + k]) ++k;
      const int last = pp->bad_ids[o + L - 1];
      if (k == L - 1) atomicOr(&ban[last >> 5], 1u << (last & 31));
    }
  }
  __syncthreads();
  if (scan) {
    m_seen = pp->penalty != 1.0f ? lane_bits<NPL>(seen, v0) : 0ull;
    m_ban = lane_bits<NPL>(ban, v0) | (pp->has_bad1 ? lane_bits<NPL>(pp->bad1, v0) : 0ull);
    m_post = (pp->has_supp ? lane_bits<NPL>(pp->supp, v0) : 0ull) |
             (pp->has_begin && cur == pp->begin_index ? lane_bits<NPL>(pp->begin, v0) : 0ull);
  }
  if (!row) return;
  apply_lane_processors<NPL>(pp, x, cur, v0, a.V, a.eos_id, m_seen, m_ban, m_gram, m_post);
}
// The MIDI token grammar (m2m_generate_grammar; music2midi_amd/grammar.py defines it, t5.h GrammarState holds a clip's state).
// The ids of this lane the grammar BANS after the clip's prefix.  The state is the same for the whole wavefront (one row): every
// lane loads the same 48 bytes and the first lane's values become scalars; the allowed set is range compares on them plus, for the
// pitch ids, a 64-bit window of the 128-bit pitch set.  No LDS, no history: the cost does not depend on the position.
template <int NPL>
__device__ __forceinline__ unsigned long long grammar_banned(const GrammarParams* gp, const GrammarState* st, int v0, int V) {
  auto uni = [](unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); };
  const uint4* q = reinterpret_cast<const uint4*>(st);
  const uint4 hd = q[0], o4 = q[1], n4 = q[2];
  const int phase = (int)uni(hd.x), next_time = (int)uni(hd.y);
  const unsigned o0 = uni(o4.x), o1 = uni(o4.y), o2 = uni(o4.z), o3 = uni(o4.w);
  const unsigned n0 = uni(n4.x), n1 = uni(n4.y), n2 = uni(n4.z), n3 = uni(n4.w);
  const int pitch0 = gp->pitch0, time0 = gp->time0, end = gp->end;
  const bool list_end = phase == GRAM_START || phase == GRAM_ONSET_LIST || phase == GRAM_OFFSET_LIST;   // a group may end here
  const bool onset = phase == GRAM_ONSET_OPEN || phase == GRAM_ONSET_LIST, offset = phase == GRAM_OFFSET_OPEN || phase == GRAM_OFFSET_LIST;
  const bool any_old = (o0 | o1 | o2 | o3) != 0u;
  unsigned long long ok = 0ull;
  if (list_end) ok |= lane_range_bits<NPL>(GRAM_EOS, GRAM_EOS + 1, v0) | lane_range_bits<NPL>(time0 + next_time, end, v0);
  if (phase == GRAM_TIME) ok |= lane_range_bits<NPL>(GRAM_ONSET, GRAM_ONSET + 1, v0);
  if ((phase == GRAM_TIME || phase == GRAM_ONSET_LIST) && any_old) ok |= lane_range_bits<NPL>(GRAM_OFFSET, GRAM_OFFSET + 1, v0);
  if (onset || offset) {
    // the pitch set the phase allows: not yet struck in this group, or sounding from an earlier one
    const unsigned long long w0 = onset ? ~(((unsigned long long)n1 << 32) | n0) : (((unsigned long long)o1 << 32) | o0);
    const unsigned long long w1 = onset ? ~(((unsigned long long)n3 << 32) | n2) : (((unsigned long long)o3 << 32) | o2);
    const int p0 = v0 - pitch0;          // pitch of this lane's first id (negative: the pitch ids start inside or past its ids)
    unsigned long long win = 0ull;       // bit j = pitch p0 + j of the set
    if (p0 <= -64 || p0 >= GRAM_MAX_PITCH) win = 0ull;
    else if (p0 < 0) win = w0 << (-p0);
    else if (p0 == 0) win = w0;
    else if (p0 < 64) win = (w0 >> p0) | (w1 << (64 - p0));
    else win = w1 >> (p0 - 64);
    ok |= win & lane_range_bits<NPL>(pitch0, time0, v0);
  }
  return ~ok & lane_range_bits<NPL>(0, V, v0);
}
// One lane, after the token store: the transition for the id the row actually emitted (forced, drawn or the arg-max), written back
// with plain stores.  The function is total: an id that is no time, mode or pitch id (PAD, BOS, EOS, the unused tail) changes nothing.
__device__ __forceinline__ void grammar_advance(const GrammarParams* gp, GrammarState* st, int tok) {
  const int phase = st->phase;
  if (tok >= gp->time0 && tok < gp->end) {
#pragma unroll
    for (int i = 0; i < GRAM_MAX_PITCH / 32; ++i) { st->open_old[i] |= st->open_new[i]; st->open_new[i] = 0u; }
    st->next_time = tok - gp->time0 + 1;
    st->phase = GRAM_TIME;
  } else if (tok == GRAM_ONSET) {
    st->phase = GRAM_ONSET_OPEN;
  } else if (tok == GRAM_OFFSET) {
    st->phase = GRAM_OFFSET_OPEN;
  } else if (tok >= gp->pitch0 && tok < gp->time0) {
    const int p = tok - gp->pitch0;      // < GRAM_MAX_PITCH (checked by m2m_generate_grammar)
    if (phase == GRAM_ONSET_OPEN || phase == GRAM_ONSET_LIST) { st->open_new[p >> 5] |= 1u << (p & 31); st->phase = GRAM_ONSET_LIST; }
    else if (phase == GRAM_OFFSET_OPEN || phase == GRAM_OFFSET_LIST) { st->open_old[p >> 5] &= ~(1u << (p & 31)); st->phase = GRAM_OFFSET_LIST; }
  }
}
// arg-max of the row, ties to the lower id (dec_head_kernel; an all -inf row gives id 0, as torch.argmax)
template <int NPL>
__device__ __forceinline__ int argmax_row(const float (&x)[NPL], int v0, int V) {
  float best = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < NPL; ++j)
    if (v0 + j < V && (x[j] > best || (x[j] == best && v0 + j < bi))) { best = x[j]; bi = v0 + j; }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  return bi == 0x7fffffff ? 0 : bi;
}
// TopK: the k-th largest key, bit by bit from the top (the largest thr with count(key >= thr) >= k); counts are ballots
template <int NPL>
__device__ __forceinline__ unsigned topk_threshold(const unsigned (&kk)[NPL], int k, int V) {
  unsigned thr = 0;
  if (k < V) {
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned cand = thr | (1u << bit);
      int cnt = 0;
#pragma unroll
      for (int j = 0; j < NPL; ++j) cnt += __popcll(__ballot(kk[j] >= cand));
      if (cnt >= k) thr = cand;
    }
  }
  return thr;
}
// TopP: the largest key c with mass(key < c) <= (1 - top_p) * Z, capped at the key of the maximum m (which always stays); the
// weights below c are zeroed.  -> c (0: no nucleus filter)
template <int NPL>
__device__ __forceinline__ unsigned topp_cutoff(const unsigned (&kk)[NPL], float (&w)[NPL], float top_p, float z, float m) {
  unsigned c = 0;
  if (top_p < 1.0f) {
    const float R = (1.0f - top_p) * z;
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned cand = c | (1u << bit);
      float lm = 0.f;
#pragma unroll
      for (int j = 0; j < NPL; ++j) lm += kk[j] < cand ? w[j] : 0.f;
      if (wave_sum_uniform(lm) <= R) c = cand;
    }
    c = min(c, ord_key(m));
#pragma unroll
    for (int j = 0; j < NPL; ++j) if (kk[j] < c) w[j] = 0.f;
  }
  return c;
}
// draw: the first kept entry (vocabulary order) whose inclusive cumulative weight exceeds u * total, u the top 24 bits of h;
// total = the sum of the weights in the draw's own order
template <int NPL>
__device__ __forceinline__ int draw_token(const float (&w)[NPL], unsigned long long h, int v0, int pad_id, float& total) {
  const int lane = threadIdx.x & 63;
  float ls = 0.f;
#pragma unroll
  for (int j = 0; j < NPL; ++j) ls += w[j];
  float incl = ls;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  total = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, incl), 63));
  const float target = (float)(h >> 40) * 0x1p-24f * total;
  const unsigned long long over = __ballot(incl > target && ls > 0.f);
  const unsigned long long any = __ballot(ls > 0.f);
  const int sel = over ? __ffsll((long long)over) - 1 : (any ? 63 - __clzll((long long)any) : 0);
  float acc = __shfl_up(incl, 1, 64);
  if (lane == 0) acc = 0.f;
  int tok = -1, last = -1;
#pragma unroll
  for (int j = 0; j < NPL; ++j) {
    if (w[j] > 0.f) {
      acc += w[j];
      last = v0 + j;
      if (tok < 0 && acc > target) tok = v0 + j;
    }
  }
  if (tok < 0) tok = last;           // rounding put the target past this lane's last kept entry
  tok = __shfl(tok, sel, 64);
  return tok < 0 ? pad_id : tok;     // no finite weight at all (the overflow flag is raised)
}
// hf generation/utils.py (greedy_search, sample): finished rows emit pad; EOS finishes a row.  `store`: one lane of the row's
// wavefront in a live chain.  -> the id the next step is fed
__device__ __forceinline__ int emit_token(const DecHeadArgs& a, int b, int t, int fin, int tok, bool store, int* s_unfinished) {
  const int next = fin ? a.pad_id : tok;
  if (store) {
    if (t + 1 < a.max_len) a.tokens[(int64_t)a.tok_row[b] * a.max_len + t + 1] = next;
    const int nf = fin | (next == a.eos_id);
    a.finished[b] = nf;
    if (!nf) atomicAdd(s_unfinished, 1);
  }
  return next;
}
// one wavefront: the embedding of id `next` (pad for an id outside the vocabulary) into slot b's row of the fixed-point residual
// stream; a finished chain (!live) stores nothing
__device__ __forceinline__ void write_embedding_row(const DecHeadArgs& a, int b, int next, bool live) {
  if (next < 0 || next >= a.V) next = a.pad_id;
  const float* emb = a.shared + (int64_t)next * a.d;
  for (int c = (threadIdx.x & 63) * 4; c < a.d; c += 256) {
    const float4 e4 = *reinterpret_cast<const float4*>(emb + c);
    xq_t* xp = a.x + (int64_t)b * a.d + c;
    if (live) {
      *reinterpret_cast<longlong2*>(xp) = make_longlong2(xq_fix_guarded(e4.x, a.state), xq_fix_guarded(e4.y, a.state));
      *reinterpret_cast<longlong2*>(xp + 2) = make_longlong2(xq_fix_guarded(e4.z, a.state), xq_fix_guarded(e4.w, a.state));
    }
  }
}
// One thread per workgroup of a live chain, after the workgroup's barrier, with the workgroup's count of unfinished rows (beam
// search: clips).  The step closes when the last workgroup is through: every workgroup has read t / done before it takes its ticket.
__device__ __forceinline__ void close_step(DecState* stp, int t, int unfinished) {
  if (unfinished) atomicAdd(&stp->smp_unfinished, unfinished);
  __threadfence();
  if (atomicAdd(&stp->smp_ticket, 1) == (int)gridDim.x - 1) {
    __threadfence();
    const int nu = atomicExch(&stp->smp_unfinished, 0);
    stp->smp_ticket = 0;
    const int nt = t + 1;
    stp->t = nt;
    stp->n_unfinished = nu;
    if (nu == 0 || nt >= stp->max_steps) { stp->done = 1; stp->out_len = nt + 1; }
  }
}

// The select step, one row per wavefront.  GREEDY: arg-max, else the warpers and the draw (sp).  PROCESSED: the logits processors
// first (pp); without it no ProcessParams is read and no LDS beyond the s_unfinished word is used.  SCORED: the outputs too (sc).
// PROCESSED heads also read the GrammarParams block (gp): with its enable flag set (m2m_generate_grammar) a live row masks its logits
// with the token grammar and advances its clip's state (gs, by clip) with the id it emitted; a finished row does neither.
template <int NPL, bool GREEDY, bool PROCESSED, bool SCORED>
__device__ __forceinline__ void select_head(const DecHeadArgs& a, const SampleParams* sp, const ProcessParams* pp, const ScoreParams* sc,
                                            const GrammarParams* gp = nullptr, GrammarState* gs = nullptr) {
  static_assert(PROCESSED || !SCORED, "the scored head is the processed head (a neutral ProcessParams block without processors)");
  __shared__ int s_unfinished;
  DecState* stp = a.state;
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = blockIdx.x * SAMPLE_ROWS + (tid >> 6);
  const int V = a.V, v0 = lane * NPL;
  const bool row = b < a.B;
  // the row's logits are requested before the loop state is consumed (as in dec_head_kernel)
  float x[NPL];
  const bool bad = load_row<NPL>(a.logits + (int64_t)(row ? b : 0) * a.ldl, v0, V, x);   // the RAW logits: the processors' -inf is legal
  const float temp = GREEDY ? 1.0f : sp->temperature, top_p = GREEDY ? 1.0f : sp->top_p;
  const int top_k = GREEDY ? 0 : sp->top_k;
  const unsigned long long seed_h = GREEDY ? 0ull : splitmix64(sp->seed);
  const int t = stp->t;
  const bool live = !(stp->done | (t >= stp->max_steps));
  if (tid == 0) s_unfinished = 0;
  __syncthreads();
  bool gram = false;
  if constexpr (PROCESSED) {
    unsigned long long m_gram = 0ull;
    gram = gp->enable && row && live && !a.finished[b];
    if (gram) m_gram = grammar_banned<NPL>(gp, gs + a.tok_row[b], v0, V);
    apply_processors<NPL>(a, pp, x, b, row, live, t + 1, v0, m_gram);
  }
  const int k = top_k > 0 ? min(top_k, V) : V;
  if (row) {
    const int fin = a.finished[b];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < NPL; ++j)
      if (v0 + j < V) { if (temp != 1.0f) x[j] = x[j] / temp; m = fmaxf(m, x[j]); }
    int tok;
    float zsum = 0.f;          // SCORED: the sum of exp(x - m) over the entries the select saw (m: their maximum)
    if constexpr (GREEDY) {
      tok = argmax_row<NPL>(x, v0, V);
      if constexpr (SCORED) {
        m = wave_max(m);
        float zl = 0.f;
#pragma unroll
        for (int j = 0; j < NPL; ++j) zl += (v0 + j < V) ? expf(x[j] - m) : 0.f;
        zsum = wave_sum_uniform(zl);
      }
    } else {
      m = wave_max(m);          // exact: every lane holds the same maximum
      unsigned kk[NPL];         // order-preserving keys; 0 (below every finite logit's) past the vocabulary
#pragma unroll
      for (int j = 0; j < NPL; ++j) kk[j] = (v0 + j < V) ? ord_key(x[j]) : 0u;
      const unsigned thr = topk_threshold<NPL>(kk, k, V);
      float w[NPL];
      float z = 0.f;
#pragma unroll
      for (int j = 0; j < NPL; ++j) {
        w[j] = (v0 + j < V && kk[j] >= thr) ? expf(x[j] - m) : 0.f;
        z += w[j];
      }
      z = wave_sum_uniform(z);
      const unsigned cut = topp_cutoff<NPL>(kk, w, top_p, z, m);
      const unsigned long long h = splitmix64(seed_h ^ (((unsigned long long)(unsigned)a.tok_row[b] << 32) | (unsigned)t));
      // the log-probability's sum is over what both filters kept - the draw's total, not z, which still holds the mass top-p removed
      tok = draw_token<NPL>(w, h, v0, a.pad_id, zsum);
      if constexpr (SCORED) {
        // HF's warped row: what top-k and top-p removed is -inf (by the keys, not by w: a kept entry's weight may underflow to 0)
#pragma unroll
        for (int j = 0; j < NPL; ++j) if (kk[j] < thr || kk[j] < cut) x[j] = -INFINITY;
      }
    }
    if (__ballot(bad) && live && lane == 0) stp->overflow = 1;
    // a row that finished before this step writes nothing (the caller's buffers are zeroed); t < steps and the clip < rows while live
    if (SCORED && live && !fin) {
      const int clip = a.tok_row[b];
      if (sc->scores) {
        float* dst = sc->scores + ((int64_t)t * sc->rows + clip) * V;
        if (sc->vec4) {            // V % 4 == 0 and an aligned base: 16-byte stores, NPL / 4 per lane over NPL contiguous floats
#pragma unroll
          for (int q = 0; q < NPL; q += 4)
            if (v0 + q < V) *reinterpret_cast<float4*>(dst + v0 + q) = make_float4(x[q], x[q + 1], x[q + 2], x[q + 3]);
        } else {
#pragma unroll
          for (int j = 0; j < NPL; ++j) if (v0 + j < V) dst[v0 + j] = x[j];
        }
      }
      if (sc->logprobs) {          // log_softmax(row)[token]: NaN for a row without a finite entry, as torch's
        const int tk = (tok >= 0 && tok < V) ? tok : 0;
        float xs = 0.f;
#pragma unroll
        for (int j = 0; j < NPL; ++j) if (v0 + j == tk) xs = x[j];
        xs = __shfl(xs, tk / NPL, 64);
        if (lane == 0) sc->logprobs[(int64_t)clip * sc->steps + t] = (xs - m) - logf(zsum);
      }
    }
    const int next = emit_token(a, b, t, fin, tok, lane == 0 && live, &s_unfinished);
    if constexpr (PROCESSED)
      if (gram && lane == 0) grammar_advance(gp, gs + a.tok_row[b], next);
    write_embedding_row(a, b, next, live);
  }
  __syncthreads();
  if (tid == 0 && live) close_step(stp, t, s_unfinished);
}

template <int NPL>
__global__ __launch_bounds__(64 * SAMPLE_ROWS) void dec_sample_kernel(DecHeadArgs a, const SampleParams* sp) {
  select_head<NPL, false, false, false>(a, sp, nullptr, nullptr);
}
template <int NPL, bool GREEDY>
__global__ __launch_bounds__(64 * SAMPLE_ROWS) void dec_process_kernel(DecHeadArgs a, const SampleParams* sp, const ProcessParams* pp,
                                                                       const GrammarParams* gp, GrammarState* gs) {
  select_head<NPL, GREEDY, true, false>(a, sp, pp, nullptr, gp, gs);
}
template <int NPL, bool GREEDY>
__global__ __launch_bounds__(64 * SAMPLE_ROWS) void dec_scored_kernel(DecHeadArgs a, const SampleParams* sp, const ProcessParams* pp,
                                                                      const ScoreParams* sc, const GrammarParams* gp, GrammarState* gs) {
  select_head<NPL, GREEDY, true, true>(a, sp, pp, sc, gp, gs);
}

// launch(integral_constant NPL) for a head that keeps a row in one wavefront's registers: NPL logits per lane, the smallest of 8, 16,
// 32, 64 with V <= 64 NPL
template <typename F>
static int launch_vocab_band(const char* kernel, int V, F launch) {
  M2M_REQUIRE(V >= 1 && V <= SAMPLE_MAX_VOCAB, "%s: vocab_size %d outside [1, %d]", kernel, V, SAMPLE_MAX_VOCAB);
  if (V <= 64 * 8) launch(std::integral_constant<int, 8>());
  else if (V <= 64 * 16) launch(std::integral_constant<int, 16>());
  else if (V <= 64 * 32) launch(std::integral_constant<int, 32>());
  else launch(std::integral_constant<int, 64>());
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

// head_mode: HEAD_SAMPLE, HEAD_PROCESSED | select, HEAD_SCORED | HEAD_PROCESSED | select (select: HEAD_GREEDY or HEAD_SAMPLE)
static int launch_dec_select(const DecHeadArgs& h, int head_mode, const SampleParams* sp, const ProcessParams* pp, const ScoreParams* sc,
                             const GrammarParams* gp, GrammarState* gs, hipStream_t st) {
  const bool scored = head_mode & HEAD_SCORED, processed = head_mode & HEAD_PROCESSED, greedy = !(head_mode & HEAD_SAMPLE);
  const dim3 grid((unsigned)ceil_div(h.B, SAMPLE_ROWS)), block(64 * SAMPLE_ROWS);
  return launch_vocab_band(scored ? "dec_scored_kernel" : processed ? "dec_process_kernel" : "dec_sample_kernel", h.V, [&](auto npl) {
    constexpr int NPL = decltype(npl)::value;
    if (scored && greedy) hipLaunchKernelGGL((dec_scored_kernel<NPL, true>), grid, block, 0, st, h, sp, pp, sc, gp, gs);
    else if (scored) hipLaunchKernelGGL((dec_scored_kernel<NPL, false>), grid, block, 0, st, h, sp, pp, sc, gp, gs);
    else if (processed && greedy) hipLaunchKernelGGL((dec_process_kernel<NPL, true>), grid, block, 0, st, h, sp, pp, gp, gs);
    else if (processed) hipLaunchKernelGGL((dec_process_kernel<NPL, false>), grid, block, 0, st, h, sp, pp, gp, gs);
    else hipLaunchKernelGGL(dec_sample_kernel<NPL>, grid, block, 0, st, h, sp);
  });
}

// ============================================================== beam head ====
// Beam search (m2m_generate_beam) replaces dec_head_kernel by this kernel, one workgroup per clip (its beam_nb rows), and follows
// transformers 4.34 (hf: generation/utils.py _beam_search, generation/beam_search.py BeamSearchScorer.process / BeamHypotheses):
//   scores = log_softmax(logits) + running beam score (fp32); the clip's top 2 nb over nb x V, ties to the lower flat (beam-major)
//   index; walked in rank order, an EOS candidate of rank < nb becomes a hypothesis (score sum / len^lp in double, len = t + 1:
//   the start token and the generated ones, not EOS; at most nb kept, BeamHypotheses.add's worst-score bookkeeping), an EOS of
//   rank >= nb is dropped, every other candidate is the next running beam until there are nb; then is_done.
// A beam is a path through the self K/V caches (DecAttnArgs::anc): new beam i of parent p gets p's ancestry plus p at position t,
// double-buffered by the parity of t; the token fed at position j of slot s stays in the token matrix at [s][j] (written once).
// A hypothesis keeps a snapshot of its tokens.  The rows of a done clip are marked finished (their K/V streams stop); the step
// closes when the last workgroup is through (close_step, the select heads' ticket), the chain is done when every clip is.
struct DecBeamArgs {
  BeamParams* p;           // the call's parameters (device block; max_hyp_len is written by the finalize kernel)
  BeamClip* clip;          // [clips of the view]
  BeamRow* row;            // [rows of the view]: running beams, and hypothesis slot h of clip c in row c * nb + h
  unsigned char* anc;      // [rows][anc_ld] ancestries of the view, parity 0; parity 1 at + anc_par
  int64_t anc_par;
  int anc_ld;
  int64_t* hyp_tok;        // [rows][max_len] hypothesis snapshots (slot as in `row`)
};
// The processed beam head (m2m_generate_beam_processed, dec_beam_kernel<NPL, true>) also reads the ProcessParams and GrammarParams
// blocks of the call and keeps one grammar state PER ROW (a clip's beams diverge), which follows its parent when the beams reorder.
struct DecBeamProcArgs : DecBeamArgs {
  const ProcessParams* pp;
  const GrammarParams* gp;
  GrammarState* gs;        // [rows of the view]
};

__device__ inline float ord_key_inv(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}
__device__ inline unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
// one hypothesis into the clip's store (BeamHypotheses.add); slots [r0, r0 + nb) of the row block; returns the slot or -1
__device__ inline int beam_hyp_add(BeamClip* bc, BeamRow* row, int r0, int nb, double score) {
  if (!(bc->n_hyp < nb || score > bc->worst)) return -1;
  int slot;
  if (bc->n_hyp < nb) {
    slot = bc->n_hyp++;
    bc->worst = fmin(score, bc->worst);
  } else {                 // full: the new one replaces the worst (the earliest added among equal scores), worst = the new minimum
    slot = 0;
    for (int h = 1; h < nb; ++h) {
      const BeamRow& a = row[r0 + h];
      const BeamRow& b = row[r0 + slot];
      if (a.hyp_score < b.hyp_score || (a.hyp_score == b.hyp_score && a.hyp_stamp < b.hyp_stamp)) slot = h;
    }
  }
  row[r0 + slot].hyp_score = score;
  row[r0 + slot].hyp_stamp = bc->stamp++;
  if (bc->n_hyp == nb) {
    double w = row[r0].hyp_score;
    for (int h = 1; h < nb; ++h) w = fmin(w, row[r0 + h].hyp_score);
    bc->worst = w;
  }
  return slot;
}

// PROCESSED (HEAD_BEAM | HEAD_PROCESSED): hf _beam_search with a non-empty logits_processor - the row's log-probabilities are
// processed (apply_lane_processors: the EOS bans, the grammar of the row's own state, the forced ids, the bitmaps of the block)
// BEFORE the running score is added, so a forced id scores 0 + the beam score and a banned one -inf.  The processors that read a
// row's history are not part of this head (m2m_generate_beam_processed refuses them).  Candidates at -inf rank behind every finite
// one and among themselves by the flat index (ord_key(-inf) is above the key 0 of an exhausted lane), so a clip with fewer than nb
// finite non-EOS candidates fills its beams from them, in the restatement's order; such a beam carries -inf from there on (-inf +
// a finite log-probability), and nothing becomes NaN: the raw logits are finite and no +inf arises.  The false form is the kernel
// as it was: the same arguments, the same instructions.
template <int NPL, bool PROCESSED = false>
__global__ __launch_bounds__(1024) void dec_beam_kernel(DecHeadArgs a, std::conditional_t<PROCESSED, DecBeamProcArgs, DecBeamArgs> bm) {
  __shared__ unsigned long long cand[BEAM_MAX][2 * BEAM_MAX];   // per beam: its top 2 nb keys, descending
  __shared__ unsigned long long top[2 * BEAM_MAX];              // the clip's top 2 nb
  __shared__ int s_par[BEAM_MAX], s_tok[BEAM_MAX], s_src[BEAM_MAX];
  __shared__ float s_score[BEAM_MAX];
  __shared__ int s_bad, s_done;
  DecState* stp = a.state;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nb = bm.p->nb, K = 2 * nb, V = a.V, r0 = blockIdx.x * nb;
  const int t = stp->t;
  const bool live = !(stp->done | (t >= stp->max_steps));
  BeamClip* bc = bm.clip + blockIdx.x;
  const int was_done = bc->done;
  const bool work = live && !was_done;
  if (tid == 0) { s_bad = 0; s_done = was_done; }
  if (tid < BEAM_MAX) s_src[tid] = -1;
  // the clip's nb grammar states to LDS before any is written (phase D): a parent may feed several children and be overwritten by another
  unsigned* s_gs = nullptr;
  bool gram = false;
  if constexpr (PROCESSED) {
    __shared__ unsigned s_gs_words[BEAM_MAX * (sizeof(GrammarState) / 4)];
    s_gs = s_gs_words;
    gram = bm.gp->enable != 0;
    if (work && gram && tid < nb * (int)(sizeof(GrammarState) / 4)) s_gs[tid] = reinterpret_cast<const unsigned*>(bm.gs + r0)[tid];
  }
  __syncthreads();
  if (work) {
    // A. per beam (one wave): fp32 log-softmax plus the running score, then the beam's own top 2 nb by repeated arg-max
    for (int r = wave; r < nb; r += 16) {
      const float* lg = a.logits + (int64_t)(r0 + r) * a.ldl;
      const int v0 = lane * NPL;
      float x[NPL];
      const bool bad = load_row<NPL>(lg, v0, V, x);
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < NPL; ++j) if (v0 + j < V) m = fmaxf(m, x[j]);
      m = wave_max(m);
      float z = 0.f;
#pragma unroll
      for (int j = 0; j < NPL; ++j) if (v0 + j < V) z += expf(x[j] - m);
      z = wave_sum(z);                    // butterfly: the same bits in every lane
      const float lz = logf(z), bs = bm.row[r0 + r].score;
      if constexpr (PROCESSED) {
        const ProcessParams* pp = bm.pp;
        const int cur = t + 1;
#pragma unroll
        for (int j = 0; j < NPL; ++j) x[j] = (x[j] - m) - lz;
        const unsigned long long m_gram = gram ? grammar_banned<NPL>(bm.gp, bm.gs + r0 + r, v0, V) : 0ull;
        const unsigned long long m_ban = pp->has_bad1 ? lane_bits<NPL>(pp->bad1, v0) : 0ull;
        const unsigned long long m_post = (pp->has_supp ? lane_bits<NPL>(pp->supp, v0) : 0ull) |
                                          (pp->has_begin && cur == pp->begin_index ? lane_bits<NPL>(pp->begin, v0) : 0ull);
        apply_lane_processors<NPL>(pp, x, cur, v0, V, a.eos_id, 0ull, m_ban, m_gram, m_post);
#pragma unroll
        for (int j = 0; j < NPL; ++j) x[j] += bs;
      } else {
#pragma unroll
        for (int j = 0; j < NPL; ++j) x[j] = ((x[j] - m) - lz) + bs;
      }
      if (__ballot(bad) && lane == 0) s_bad = 1;
      unsigned long long taken = 0ull;
      for (int k = 0; k < K; ++k) {
        float bv = 0.f;
        int bj = -1;
#pragma unroll
        for (int j = 0; j < NPL; ++j)
          if (v0 + j < V && !((taken >> j) & 1ull) && (bj < 0 || x[j] > bv)) { bv = x[j]; bj = j; }
        const unsigned long long key = bj < 0 ? 0ull
            : ((unsigned long long)ord_key(bv) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)(r * V + v0 + bj));
        const unsigned long long w = wave_max_u64(key);
        if (bj >= 0 && key == w) taken |= 1ull << bj;      // keys are unique (the flat index is part of them)
        if (lane == 0) cand[r][k] = w;
      }
    }
  }
  __syncthreads();
  if (work && wave == 0) {          // B. merge the nb sorted lists (lane i walks beam i's) into the clip's top 2 nb
    int ptr = 0;
    for (int k = 0; k < K; ++k) {
      const unsigned long long h = (lane < nb && ptr < K) ? cand[lane][ptr] : 0ull;
      const unsigned long long w = wave_max_u64(h);
      if (lane < nb && h == w) ++ptr;
      if (lane == 0) top[k] = w;
    }
  }
  __syncthreads();
  if (work && tid == 0) {           // C. BeamSearchScorer.process for this clip (serial: 2 nb candidates)
    const BeamParams P = *bm.p;
    const int cur_len = t + 1;
    int bi = 0;
    for (int k = 0; k < K && bi < nb; ++k) {
      const unsigned long long key = top[k];
      const float sc = ord_key_inv((unsigned)(key >> 32));
      const int flat = (int)(0xFFFFFFFFu - (unsigned)key);
      const int beam = flat / V, tok = flat - beam * V;
      if (tok == a.eos_id) {
        if (k >= nb) continue;
        const int slot = beam_hyp_add(bc, bm.row, r0, nb, (double)sc / pow((double)cur_len, (double)P.lp));
        if (slot >= 0) { bm.row[r0 + slot].hyp_len = cur_len; s_src[slot] = beam; }
      } else {
        s_par[bi] = beam; s_tok[bi] = tok; s_score[bi] = sc; ++bi;
      }
    }
    bool done = false;              // BeamHypotheses.is_done(best running score of the step, cur_len)
    if (bc->n_hyp >= nb) {
      if (P.early == 1) done = true;
      else {
        const double best = (double)ord_key_inv((unsigned)(top[0] >> 32));
        const double len = (P.early == 2 && P.lp > 0.f) ? (double)P.max_length : (double)cur_len;
        done = bc->worst >= best / pow(len, (double)P.lp);
      }
    }
    if (done) bc->done = 1;
    s_done = done ? 1 : 0;
  }
  __syncthreads();
  if (work) {                        // D. hypothesis snapshots, the new beams' ancestries and tokens, the next input rows
    const unsigned char* ac = bm.anc + (int64_t)(t & 1) * bm.anc_par;
    unsigned char* an = bm.anc + (int64_t)((t + 1) & 1) * bm.anc_par;
    int64_t* tk = a.tokens + (int64_t)a.row0 * a.max_len;          // the view's rows of the token matrix (no re-packing: identity)
    for (int h = 0; h < nb; ++h) {
      const int p = s_src[h];
      if (p < 0) continue;
      for (int j = tid; j <= t; j += 1024) {
        const int sl = j < t ? min((int)ac[(int64_t)(r0 + p) * bm.anc_ld + j], nb - 1) : p;
        bm.hyp_tok[(int64_t)(r0 + h) * a.max_len + j] = tk[(int64_t)(r0 + sl) * a.max_len + j];
      }
    }
    const bool dn = s_done != 0;
    if constexpr (PROCESSED) {
      // new beam i: its parent's state (the LDS copy) advanced by its token, with plain stores; a clip done at this step writes nothing
      if (gram && !dn && tid < nb) {
        constexpr int W = (int)(sizeof(GrammarState) / 4);
        unsigned* dst = reinterpret_cast<unsigned*>(bm.gs + r0 + tid);
        const unsigned* src = s_gs + min(max(s_par[tid], 0), nb - 1) * W;
#pragma unroll
        for (int w = 0; w < W; ++w) dst[w] = src[w];
        grammar_advance(bm.gp, bm.gs + r0 + tid, s_tok[tid]);
      }
    }
    for (int i = wave; i < nb; i += 16) {
      const int p = dn ? i : s_par[i];
      if (!dn) {
        for (int j = lane; j < t; j += 64) an[(int64_t)(r0 + i) * bm.anc_ld + j] = ac[(int64_t)(r0 + p) * bm.anc_ld + j];
        if (lane == 0) {
          an[(int64_t)(r0 + i) * bm.anc_ld + t] = (unsigned char)p;
          if (t + 1 < a.max_len) tk[(int64_t)(r0 + i) * a.max_len + t + 1] = s_tok[i];
          bm.row[r0 + i].score = s_score[i];
        }
      } else if (lane == 0) {
        a.finished[r0 + i] = 1;     // a done clip: its rows stop streaming K/V
      }
      write_embedding_row(a, r0 + i, dn ? a.pad_id : s_tok[i], true);
    }
  }
  // E. the step closes by the select heads' ticket; the count is of clips, not rows
  __syncthreads();
  if (tid == 0 && live) {
    if (s_bad) stp->overflow = 1;
    close_step(stp, t, s_done ? 0 : 1);
  }
}

// pp == nullptr: the plain head (HEAD_BEAM); otherwise the processed one (HEAD_BEAM | HEAD_PROCESSED) with the blocks and the rows' states
static int launch_dec_beam(const DecHeadArgs& h, const DecBeamArgs& bm, int nbeams, const ProcessParams* pp, const GrammarParams* gp,
                           GrammarState* gs, hipStream_t st) {
  M2M_REQUIRE(nbeams >= 2 && nbeams <= BEAM_MAX && h.B % nbeams == 0, "dec_beam_kernel: %d rows are not clips of %d beams", h.B, nbeams);
  const dim3 grid((unsigned)(h.B / nbeams)), block(1024);
  if (pp) {
    DecBeamProcArgs bp{};
    static_cast<DecBeamArgs&>(bp) = bm;
    bp.pp = pp; bp.gp = gp; bp.gs = gs;
    return launch_vocab_band("dec_beam_kernel", h.V, [&](auto npl) {
      hipLaunchKernelGGL((dec_beam_kernel<decltype(npl)::value, true>), grid, block, 0, st, h, bp);
    });
  }
  return launch_vocab_band("dec_beam_kernel", h.V, [&](auto npl) {
    hipLaunchKernelGGL(dec_beam_kernel<decltype(npl)::value>, grid, block, 0, st, h, bm);
  });
}

// before the first step of a chain: beam 0 of every clip starts at score 0, the others at -1e9 (hf _beam_search), empty stores
__global__ void dec_beam_init_kernel(DecBeamArgs bm, int rows) {
  const int nb = bm.p->nb;
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) {
    BeamRow br{};
    br.score = (r % nb == 0) ? 0.f : -1e9f;
    bm.row[r] = br;
    if (r % nb == 0) {
      BeamClip c{};
      c.worst = 1e9;
      bm.clip[r / nb] = c;
    }
  }
}

// after every chain: BeamSearchScorer.finalize, one workgroup per clip.  A clip that is not done adds its running beams at length
// T + 1 (= max_length); the best n hypotheses, highest score first and the later-added first among equal scores (sorted(...).pop()),
// go to the output rows clip * n + j: their tokens, EOS at column len when len < max_length, pad after.  The longest picked
// hypothesis goes to BeamParams::max_hyp_len (the host trims the width to min(it + 1, max_length)).
__global__ __launch_bounds__(256) void dec_beam_final_kernel(DecBeamArgs bm, const int64_t* tokens, int max_len, int T, int64_t* out,
                                                             float* scores, int max_length, int pad_id, int eos_id) {
  __shared__ int s_src[BEAM_MAX], s_pick[BEAM_MAX];
  const int tid = threadIdx.x, nb = bm.p->nb, n = bm.p->n, clip = blockIdx.x, r0 = clip * nb;
  BeamClip* bc = bm.clip + clip;
  if (tid < BEAM_MAX) s_src[tid] = -1;
  __syncthreads();
  if (tid == 0) {
    if (!bc->done) {
      for (int i = 0; i < nb; ++i) {
        const int slot = beam_hyp_add(bc, bm.row, r0, nb, (double)bm.row[r0 + i].score / pow((double)(T + 1), (double)bm.p->lp));
        if (slot >= 0) { bm.row[r0 + slot].hyp_len = T + 1; s_src[slot] = i; }
      }
    }
    unsigned taken = 0;
    int longest = 0;
    for (int j = 0; j < n; ++j) {
      int b = -1;
      for (int h = 0; h < bc->n_hyp; ++h) {
        if ((taken >> h) & 1u) continue;
        const BeamRow& x = bm.row[r0 + h];
        if (b < 0 || x.hyp_score > bm.row[r0 + b].hyp_score ||
            (x.hyp_score == bm.row[r0 + b].hyp_score && x.hyp_stamp > bm.row[r0 + b].hyp_stamp)) b = h;
      }
      if (b < 0) b = 0;              // (never: a finalized clip holds nb >= n hypotheses)
      taken |= 1u << b;
      s_pick[j] = b;
      longest = max(longest, bm.row[r0 + b].hyp_len);
    }
    atomicMax(&bm.p->max_hyp_len, longest);
  }
  __syncthreads();
  const unsigned char* ac = bm.anc + (int64_t)(T & 1) * bm.anc_par;
  for (int h = 0; h < nb; ++h) {     // snapshots of the running beams that became hypotheses here
    const int p = s_src[h];
    if (p < 0) continue;
    for (int j = tid; j <= T; j += blockDim.x) {
      const int sl = j < T ? min((int)ac[(int64_t)(r0 + p) * bm.anc_ld + j], nb - 1) : p;
      bm.hyp_tok[(int64_t)(r0 + h) * max_len + j] = tokens[(int64_t)(r0 + sl) * max_len + j];
    }
  }
  __syncthreads();
  for (int j = 0; j < n; ++j) {
    const int h = s_pick[j];
    const int len = bm.row[r0 + h].hyp_len;
    const int64_t* src = bm.hyp_tok + (int64_t)(r0 + h) * max_len;
    int64_t* dst = out + (int64_t)(clip * n + j) * max_length;
    for (int c = tid; c < max_length; c += blockDim.x) dst[c] = c < len ? src[c] : (c == len ? eos_id : pad_id);
    if (tid == 0 && scores) scores[clip * n + j] = (float)bm.row[r0 + h].hyp_score;
  }
}

// ============================================================ live-row re-packing ====
// Clips end at different steps (a real checkpoint ends a 3 s segment after tens to hundreds of its 1 024 tokens).  The finished-row
// early-out above stops a finished row's K/V stream, but its workgroups still launch and the chain still pays its latency floor for
// every slot.  At a host poll the decode loop (t5_api.hip) therefore RE-PACKS the live rows into the first slots and relaunches
// smaller chains: every per-clip buffer has the clip index outermost, so a row is moved by copying its planes — self K/V up to the
// current position, cross K/V, the pending arg-max key, the residual row — from a slot behind the packed range into the slot of a
// finished row in front of it (source and destination sets are disjoint: one launch, no ordering).  Token rows do NOT move: slot ->
// clip is the tok_row table.  Nothing of this changes an id: a row's arithmetic never depended on its slot.
struct MoveArgs {
  int n;                        // moves in this launch (<= 64)
  short src[64], dst[64];
  unsigned char* self_k; unsigned char* self_v; unsigned char* cross_kv;
  int64_t self_row, self_layer;     // bytes between rows / layers of the self caches ([L][maxB][H][Lmax][64])
  int64_t self_head; int self_len_bytes;   // bytes between heads, bytes of the t valid keys of one head
  int H;
  int64_t cross_row, cross_plane;   // bytes of one row's [H][S][64] block, bytes between (layer, k|v) planes ([L][2][B][H][S][64])
  int L;
  unsigned long long* keys; int* finished; int* tok_row;
  xq_t* x0; int d;                  // residual buffer A
};

__global__ __launch_bounds__(256) void dec_move_rows_kernel(MoveArgs a) {
  const int mv = blockIdx.x, plane = blockIdx.y, part = blockIdx.z, nparts = gridDim.z;
  const int src = a.src[mv], dst = a.dst[mv];
  const int tid = threadIdx.x;
  if (plane < 2 * a.L) {                              // self K (even) / V (odd) of layer plane / 2: H pieces of self_len_bytes
    unsigned char* base = (plane & 1) ? a.self_v : a.self_k;
    const int64_t lo = (int64_t)(plane >> 1) * a.self_layer;
    const int per_head = a.self_len_bytes / 16;       // 16-byte units (64 elements * es is a multiple of 16)
    const int total = a.H * per_head;
    for (int i = part * 256 + tid; i < total; i += nparts * 256) {
      const int hh = i / per_head, u = i - hh * per_head;
      const int64_t off = lo + (int64_t)hh * a.self_head + (int64_t)u * 16;
      *reinterpret_cast<uint4*>(base + off + (int64_t)dst * a.self_row) = *reinterpret_cast<const uint4*>(base + off + (int64_t)src * a.self_row);
    }
  } else if (plane < 4 * a.L) {                       // cross K/V plane (layer, k|v): one contiguous block per row
    const int64_t lo = (int64_t)(plane - 2 * a.L) * a.cross_plane;
    const int64_t total = a.cross_row / 16;
    for (int64_t i = part * 256 + tid; i < total; i += nparts * 256)
      *reinterpret_cast<uint4*>(a.cross_kv + lo + (int64_t)dst * a.cross_row + i * 16) =
          *reinterpret_cast<const uint4*>(a.cross_kv + lo + (int64_t)src * a.cross_row + i * 16);
  } else if (part == 0) {                             // the row's small state
    for (int c = tid; c < a.d; c += 256) a.x0[(int64_t)dst * a.d + c] = a.x0[(int64_t)src * a.d + c];
    if (tid == 0) { a.keys[dst] = a.keys[src]; a.finished[dst] = a.finished[src]; a.tok_row[dst] = a.tok_row[src]; }
  }
}

// src[i] -> dst[i] for i < n (slots of the session; the sets are disjoint); t = keys already cached per row
int decode_move_rows(m2m_session* s, const int* src, const int* dst, int n, int t, hipStream_t st) {
  const m2m_model* m = s->m;
  const m2m_t5_geometry& g = m->g;
  const int64_t es = (int64_t)m->esize;
  for (int at = 0; at < n; at += 64) {
    MoveArgs a{};
    a.n = n - at < 64 ? n - at : 64;
    for (int i = 0; i < a.n; ++i) { a.src[i] = (short)src[at + i]; a.dst[i] = (short)dst[at + i]; }
    a.self_k = (unsigned char*)s->self_k; a.self_v = (unsigned char*)s->self_v; a.cross_kv = (unsigned char*)s->cross_kv;
    a.self_head = (int64_t)s->max_dec * DK * es; a.self_row = (int64_t)g.num_heads * a.self_head;
    a.self_layer = (int64_t)s->max_batch * a.self_row; a.self_len_bytes = (int)((int64_t)t * DK * es);
    a.H = g.num_heads; a.L = g.num_decoder_layers;
    a.cross_row = (int64_t)g.num_heads * s->S * DK * es; a.cross_plane = (int64_t)s->B * a.cross_row;
    a.keys = s->keys; a.finished = s->finished; a.tok_row = s->tok_row;
    a.x0 = reinterpret_cast<xq_t*>(s->x_dec); a.d = g.d_model;
    hipLaunchKernelGGL(dec_move_rows_kernel, dim3((unsigned)a.n, (unsigned)(4 * a.L + 1), 8), dim3(256), 0, st, a);
    M2M_CHECK_HIP(hipGetLastError());
  }
  return M2M_OK;
}

// Zero the self K/V positions [t0, t1) of every row of the view, all layers (the decode loop: rows of a chain that ended before the
// step count at which they are re-packed).  A row's block is [H][max_dec][64]; rows of a view are contiguous: one 2-D fill per plane.
int decode_clear_self(m2m_session* s, const DecView& v, int t0, int t1, hipStream_t st) {
  const m2m_model* m = s->m;
  const m2m_t5_geometry& g = m->g;
  const size_t es = m->esize;
  if (t1 > s->max_dec) t1 = s->max_dec;
  if (t0 < 0 || t0 >= t1 || v.nb <= 0) return M2M_OK;
  const size_t head = (size_t)s->max_dec * DK * es, row = (size_t)g.num_heads * head, layer = (size_t)s->max_batch * row;
  for (int l = 0; l < g.num_decoder_layers; ++l)
    for (unsigned char* base : {(unsigned char*)s->self_k, (unsigned char*)s->self_v})
      M2M_CHECK_HIP(hipMemset2DAsync(base + (size_t)l * layer + (size_t)v.b0 * row + (size_t)t0 * DK * es, head, 0,
                                     (size_t)(t1 - t0) * DK * es, (size_t)v.nb * g.num_heads, st));
  return M2M_OK;
}

// ============================================================ step driver ====
static xq_t* xbuf(m2m_session* s, const DecView& v, int which);
// the headless fold is a greedy-only form: the sampling and processed heads keep their own kernel (the step of M2M_HEADLESS=0)
static bool headless_for(const m2m_session* s, bool forced) { return !forced && s->head_mode == HEAD_GREEDY && s->sw.headless; }
// All per-clip buffers are [B][...] with the clip index outermost, so a view is a pointer offset.
static DecHeadArgs head_args(m2m_session* s, const DecView& v, bool forced, float* logits_out, int Ld) {
  const m2m_model* m = s->m;
  DecHeadArgs h{};
  h.logits = s->logits + (int64_t)v.b0 * m->vocab_pad; h.ldl = m->vocab_pad; h.V = m->g.vocab_size; h.B = v.nb;
  h.d = m->g.d_model; h.shared = m->shared; h.x = xbuf(s, v, 0); h.x_zero = xbuf(s, v, 1);
  h.tokens = s->tokens; h.tok_row = s->tok_row + v.b0; h.row0 = v.b0; h.max_len = s->max_dec;
  h.finished = s->finished + v.b0; h.state = v.state; h.pad_id = m->g.pad_token_id; h.eos_id = m->g.eos_token_id;
  h.keys = headless_for(s, forced) ? s->keys + v.b0 : nullptr;
  h.forced = forced ? s->forced_ids + (int64_t)v.b0 * Ld : nullptr; h.Ld = Ld;
  h.logits_out = logits_out ? logits_out + (int64_t)v.b0 * Ld * m->g.vocab_size : nullptr;
  return h;
}

static DecBeamArgs beam_args(m2m_session* s, const DecView& v) {
  DecBeamArgs b{};
  const int nb = s->beam_nb > 0 ? s->beam_nb : 1;
  b.p = s->beam_dev; b.clip = s->beam_clip + v.b0 / nb; b.row = s->beam_row + v.b0;
  b.anc = s->anc + (int64_t)v.b0 * s->max_dec; b.anc_par = (int64_t)s->max_batch * s->max_dec; b.anc_ld = s->max_dec;
  b.hyp_tok = s->hyp_tok + (int64_t)v.b0 * s->max_dec;
  return b;
}

int decode_beam_init(m2m_session* s, const DecView& v, hipStream_t st) {
  hipLaunchKernelGGL(dec_beam_init_kernel, dim3((unsigned)ceil_div(v.nb, 256)), dim3(256), 0, st, beam_args(s, v), v.nb);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

int decode_beam_finalize(m2m_session* s, int rows, int steps, int64_t* out, float* scores, int max_length, hipStream_t st) {
  const DecView all{0, rows, nullptr};
  const m2m_t5_geometry& g = s->m->g;
  hipLaunchKernelGGL(dec_beam_final_kernel, dim3((unsigned)(rows / s->beam_nb)), dim3(256), 0, st, beam_args(s, all), s->tokens,
                     s->max_dec, steps, out, scores, max_length, g.pad_token_id, g.eos_token_id);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

int decode_finalize(m2m_session* s, const DecView& v, hipStream_t st) {
  if (!headless_for(s, false)) return M2M_OK;
  DecHeadArgs h = head_args(s, v, false, nullptr, 0);
  hipLaunchKernelGGL(dec_final_kernel, dim3(1), dim3(256), 0, st, h);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

int decode_init(m2m_session* s, const DecView& v, int max_steps, bool forced, hipStream_t st) {
  DecHeadArgs h = head_args(s, v, forced, nullptr, forced ? max_steps : 0);
  // the sticky range flag is cleared here, not by the init kernel: that kernel's own embedding conversions may raise it
  M2M_CHECK_HIP(hipMemsetAsync(v.state, 0, sizeof(DecState), st));
  hipLaunchKernelGGL(dec_init_kernel, dim3(32), dim3(256), 0, st, h, s->m->g.decoder_start_token_id, max_steps);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

static size_t kv_layer_elems(const m2m_session* s, int len) {
  return (size_t)s->max_batch * s->m->g.num_heads * len * DK;
}

// rotation of the residual-stream buffers inside a layer: A (x_dec[0]) holds the layer input
static xq_t* xbuf(m2m_session* s, const DecView& v, int which) {
  const size_t stride = (size_t)ceil_div(s->max_batch, 32) * 32 * s->m->g.d_model;
  return reinterpret_cast<xq_t*>(s->x_dec) + (size_t)which * stride + (size_t)v.b0 * s->m->g.d_model;
}

// Clips of one head per attention workgroup for a chain of nb clips: the multi-clip form (dec_attn_mc_kernel) from the chain sizes at
// which the launches stop being single latency chains and become rounds of workgroups (measured: tools/native_chain_sweep.py, DESIGN
// 4.3); s->sw.attn_clips > 0 forces a value (M2M_DA_CLIPS, latched when the session is created; tests and A/B runs).
int decode_attn_clips(const m2m_session* s, int nb) {
  if (s->sw.attn_clips > 0) return s->sw.attn_clips;
  // same-box sweeps (tools/native_mc_sweep.py, us per step, C = 1 / 2 / 4): 2 x 16 clips, S = 864: 195 / 238 / -; 2 x 24: 264 / 266 / 363;
  // 2 x 32: 329 / 300 / 386; 2 x 64, S = 864: 595 / 522 / 512; 2 x 64, S = 190 (the reference's chunk): 446 / 383 / 362;
  // S = 190: 2 x 32: 256 / 226 / 289; 2 x 40: - / 276 / 299; 2 x 48: - / 316 / 313
  return nb >= 48 ? 4 : (nb >= 32 ? 2 : 1);
}

// residual rows per feed-forward workgroup for a chain of nb clips (M2M_DEC_FF_ROWS forces 8 or 16, latched per session).  16 rows
// measured no different from 8 at 2 x 64 clips (365.5 / 366.3 us per step): 8 everywhere.
int decode_ff_rows(const m2m_session* s, int nb) {
  (void)nb;
  return s->sw.ff_rows > 0 ? s->sw.ff_rows : 8;
}
// hidden slices per feed-forward workgroup (dec_ff_multi_kernel from 2; M2M_DEC_FF_SLICES forces 1, 2 or 4, latched per session)
int decode_ff_slices(const m2m_session* s, int nb) {
  if (s->sw.ff_slices > 0) return s->sw.ff_slices;
  // same-box sweeps (tools/native_mc_sweep.py, us per step, 1 / 2 / 4 slices): 2 x 16 clips 196 / 204 / -; 2 x 32: 301 / 292 / 312;
  // 2 x 48, S = 190: - / 313 / 326; 2 x 64 (the reference's chunk): 362 / 349-353 / 345-347
  return nb >= 56 ? 4 : (nb >= 32 ? 2 : 1);
}

// The cache policy of the session's K/V loads: non-temporal once the K/V working set of one decode step (all layers, cross + self
// at the session's maximum length) is beyond what the 256 MB Infinity Cache can keep between steps, with as many whole layers of
// cross K/V as fit a 180 MB budget (or M2M_KV_RESIDENT_LAYERS) left on the default policy.  B = 32: 3 of 6 layers, 271.0 -> 266.6 ms
// per batch.
KvPolicy decode_kv_policy(const m2m_session* s) {
  const m2m_model* m = s->m;
  const m2m_t5_geometry& g = m->g;
  const double es = (double)m->esize;
  const double kv_step_bytes = (double)g.num_decoder_layers * 2.0 * s->B * m->inner * ((double)s->S + s->max_dec) * es;
  const double per_layer = 2.0 * s->B * m->inner * (double)s->S * es;
  KvPolicy p;
  p.nt = kv_step_bytes > 200e6;
  p.resident = s->sw.kv_resident_layers >= 0 ? s->sw.kv_resident_layers : (int)(180e6 / per_layer);
  return p;
}

// May `chains` chains run on without the re-alignment that a draining host poll gives them (the decode loop's poll look-ahead)?
// Not two chains that stream the same cross-K/V layers from HBM: left to drift they measured 2.9 % (bf16) / 3.6 % (fp32) SLOWER than
// with the draining polls, and only windows that together hold every layer (2 x resident >= layers: the headline's 3 + 3) turned
// the look-ahead into a gain (profiles/poll_lookahead_ab.txt).
bool decode_chains_may_drift(const m2m_session* s, int chains) {
  const KvPolicy p = decode_kv_policy(s);
  const int L = s->m->g.num_decoder_layers;
  if (chains != 2 || !p.nt || p.resident >= L) return true;
  return s->sw.kv_resident_stagger && 2 * p.resident >= L;
}

int decode_launch_attn(m2m_session* s, const DecView& v, bool self, int layer, int self_len, hipStream_t st, bool headless, bool skip_finished) {
  const m2m_model* m = s->m;
  const m2m_t5_geometry& g = m->g;
  const size_t es = m->esize;
  const int H = g.num_heads;
  const DecLayerPacked& L = m->dec[layer];
  DecAttnArgs a{};
  const KvPolicy kp = decode_kv_policy(s);
  bool nt = kp.nt;
  // ... but `resident` whole layers of cross K/V keep the default policy and stay cache-resident from step to step (they are
  // re-read every step; the rest streams past them non-temporally): which ones is the chain's window, t5.h kv_layer_resident
  if (nt && !self && kv_layer_resident(layer, g.num_decoder_layers, kp.resident, v.ord, v.count, s->sw.kv_resident_stagger)) nt = false;
  int clips = decode_attn_clips(s, v.nb);
  if (self && s->sw.attn_clips_self > 0) clips = s->sw.attn_clips_self;      // diagnostic: another width for the self-attention launches
  // self: A -> B (zero C); cross: B -> C (zero A)
  a.x = xbuf(s, v, self ? 0 : 1); a.x_out = xbuf(s, v, self ? 1 : 2); a.x_zero = xbuf(s, v, self ? 2 : 0);
  a.eps = g.layer_norm_eps; a.d = g.d_model;
  a.H = H; a.inner = m->inner; a.state = v.state;
  if (skip_finished && s->sw.finished_skip) { a.fin_skip = s->finished + v.b0; a.fin_stride = 1; }
  else { a.fin_skip = &v.state->zero; a.fin_stride = 0; }
  // beam search: the view's rows are clips x beam_nb beams (the view starts at a clip boundary)
  const bool beam = (s->head_mode & HEAD_BEAM) && s->beam_nb > 0;
  if (beam) {
    a.beam_nb = s->beam_nb;
    a.anc = s->anc + (int64_t)v.b0 * s->max_dec; a.anc_par = (int64_t)s->max_batch * s->max_dec; a.anc_ld = s->max_dec;
  }
  if (headless && layer == 0) {            // the greedy loop without the head kernel: layer 0 takes over its work
    a.keys = s->keys + v.b0; a.finished = s->finished + v.b0; a.tokens = s->tokens; a.tok_row = s->tok_row + v.b0;
    a.max_len = s->max_dec; a.V = g.vocab_size; a.pad_id = g.pad_token_id; a.eos_id = g.eos_token_id;
    if (self) a.emb = m->shared; else a.book = 1;
  }
  if (self) {
    const size_t off = ((size_t)layer * kv_layer_elems(s, s->max_dec) + (size_t)v.b0 * H * s->max_dec * DK) * es;
    a.ln_w = L.ln0; a.Wp = L.wqkv; a.Wo = L.wo_img;
    a.Kc = (unsigned char*)s->self_k + off;
    a.Vc = (unsigned char*)s->self_v + off;
    a.kv_stride = s->max_dec; a.n_keys = 0; a.self_len_override = self_len;
    a.bias = s->dec_bias_tab; a.bias_stride = s->max_dec;
    // Layer 0 from the token tables (M2M_DEC_TOKEN_TABLES, latched per session): the one-clip kernel of the headless greedy step,
    // on a model that has tables.  Every other form (several clips per workgroup, the teacher-forced, beam, sampled, processed and
    // scored steps, M2M_HEADLESS=0, the bench's length override) projects and streams the cache, which the table form keeps
    // appending to.
    int tab = 0;
    if (layer == 0 && clips == 1 && !beam && self_len <= 0 && m->q0_tab && a.emb) tab = s->sw.token_tables;
    if (tab) { a.q0_tab = m->q0_tab; a.k0_tab = m->k0_tab; a.v0_tab = m->v0_tab; }
    return launch_dec_attn(m->precision, true, nt, tab, a, v.nb, clips, s->sw.mc_cif, st);
  }
  // cross K/V: [L][2][B][H][S][64] with B, S = the encoded problem
  const size_t per = (size_t)s->B * H * s->S * DK;
  const size_t voff = (size_t)(beam ? v.b0 / s->beam_nb : v.b0) * H * s->S * DK;
  a.ln_w = L.ln1; a.Wp = L.wcq; a.Wo = L.wco_img;
  a.Kc = (unsigned char*)s->cross_kv + (((size_t)layer * 2 + 0) * per + voff) * es;
  a.Vc = (unsigned char*)s->cross_kv + (((size_t)layer * 2 + 1) * per + voff) * es;
  a.kv_stride = s->S; a.n_keys = s->S; a.self_len_override = 0; a.bias = nullptr; a.bias_stride = 0;
  return launch_dec_attn(m->precision, false, nt, 0, a, v.nb, clips, s->sw.mc_cif, st);
}

int decode_launch_step(m2m_session* s, const DecView& v, bool forced, float* logits_out, int Ld, hipStream_t st) {
  const m2m_model* m = s->m;
  const m2m_t5_geometry& g = m->g;
  const int P = m->precision;
  xq_t* xA = xbuf(s, v, 0);
  xq_t* xB = xbuf(s, v, 1);
  xq_t* xC = xbuf(s, v, 2);
  int rc;
  const bool headless = headless_for(s, forced);
  for (int l = 0; l < g.num_decoder_layers; ++l) {
    const DecLayerPacked& L = m->dec[l];
    // 1. RMSNorm + per-head QKV projection + KV-cache append + causal self-attention + per-head
    //    output projection accumulated into the residual stream (one kernel)
    if ((rc = decode_launch_attn(s, v, true, l, 0, st, headless, !forced))) return rc;
    // 2. the same for cross-attention over the S encoder positions (query projection only)
    if ((rc = decode_launch_attn(s, v, false, l, 0, st, headless, !forced))) return rc;
    // 3. feed-forward sub-layer, one kernel: reads C (the stream after both attention sub-layers),
    //    accumulates C + FF(C) into A (zeroed by the cross-attention kernel) and leaves B zeroed for
    //    the next layer's self-attention
    DecFfArgs f{};
    f.x = xC; f.x_out = xA; f.x_zero = xB; f.ln_w = L.ln2; f.eps = g.layer_norm_eps;
    f.Wimg = L.ff_img; f.d = g.d_model; f.d_ff = g.d_ff; f.B = v.nb; f.state = v.state;
    f.check_done = (headless && l == 0) ? 1 : 0;
    if ((rc = launch_dec_ff(P, f, decode_ff_rows(s, v.nb), decode_ff_slices(s, v.nb), st))) return rc;
  }
  // final RMSNorm + lm_head (untied, no d_model**-0.5 scaling: transformers 4.34 semantics)
  DecGemmArgs a{};
  a.eps = g.layer_norm_eps; a.B = v.nb; a.state = v.state;
  a.x = xA; a.ldx = g.d_model; a.ln_w = m->dec_final_ln; a.W = m->lm_head; a.K = g.d_model; a.N = g.vocab_size;
  a.out = s->logits + (int64_t)v.b0 * m->vocab_pad; a.ldo = m->vocab_pad;
  a.keys = headless ? s->keys + v.b0 : nullptr;
  if ((rc = launch_dec_gemm(P, a, st))) return rc;
  if (headless) return M2M_OK;             // the arg-max key is consumed by the next step's layer 0 (or by decode_finalize)
  DecHeadArgs h = head_args(s, v, forced, logits_out, Ld);
  if (!forced && (s->head_mode & HEAD_BEAM)) {
    const bool processed = s->head_mode & HEAD_PROCESSED;       // the grammar states of a beam call are by row: the view's start at b0
    return launch_dec_beam(h, beam_args(s, v), s->beam_nb, processed ? s->proc_dev : nullptr, s->gram_dev, s->gram_state + v.b0, st);
  }
  if (!forced && s->head_mode != HEAD_GREEDY) return launch_dec_select(h, s->head_mode, s->sample_dev, s->proc_dev, s->score_dev, s->gram_dev, s->gram_state, st);
  hipLaunchKernelGGL(dec_head_kernel, dim3(1), dim3(1024), 0, st, h);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

}  // namespace m2m

#ifdef M2M_STAMPS
// diagnostic builds only: copy the stamp log to the host and reset it (not declared in the public header)
extern "C" int m2m_debug_read_stamps(unsigned long long* out_host, int max_n) {
  unsigned int n = 0;
  if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(m2m::g_stamp_n), sizeof(n)) != hipSuccess) return -1;
  if ((int)n > max_n) n = (unsigned)max_n;
  if (n > (1u << 18)) n = 1u << 18;
  if (n && hipMemcpyFromSymbol(out_host, HIP_SYMBOL(m2m::g_stamps), (size_t)n * 8) != hipSuccess) return -1;
  unsigned int z = 0;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(m2m::g_stamp_n), &z, sizeof(z));
  void* p = nullptr;
  if (hipGetSymbolAddress(&p, HIP_SYMBOL(m2m::g_stamps)) == hipSuccess) (void)hipMemset(p, 0, sizeof(unsigned long long) << 18);
  return (int)n;
}
#endif
