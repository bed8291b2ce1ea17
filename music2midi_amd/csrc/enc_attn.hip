// Encoder-side attention (one shot per clip batch; also the batched teacher-forced decoder pass): the two flash-attention forms
// with the T5 relative-position bias, and the V transpose that feeds them.  Part of what replaces the HF T5 encoder stack
// (hf: models/t5/modeling_t5.py:663-750); the products around it are in enc_gemm.hip.
//
// attn_kernel is templated on the storage type T of the precision mode: float (f32-input MFMA, exact fp32 FMA chains: parity
// mode) or bf16 (bf16 MFMA, fp32 accumulate: throughput mode); attn_wide_kernel is bf16 only.
#include "mma.h"
#include "t5.h"

namespace m2m {

// =========================================================== attention ====
// Flash-style bidirectional self-attention with T5's additive relative-position bias and NO
// 1/sqrt(d) scaling (hf: modeling_t5.py:159-170,197).  Workgroup = 4 waves = 128 query rows
// of one (clip, head); keys/values stream through LDS in 64-key tiles.
//
// Orientation: S^T = K * Q^T, so a lane owns ONE query column and 16 keys in registers
// (row-softmax is 15 in-lane ops + one cross-half exchange) and the running rescale factor
// is a per-lane scalar.  P^T then feeds O^T = V^T * P^T directly as the MFMA B operand with
// no lane movement; V^T is staged in LDS with key slots permuted to match (vt_pos).
constexpr int AQ = 128, AK = 64;
constexpr int TB_PAD = AQ;        // spare bias-table entries below index 0 (query rows of the last tile past Sq)

template <typename T> struct AttnCfg;
template <> struct AttnCfg<bf16_t> { static constexpr int KP = DK + 8, VP = AK + 8; };
template <> struct AttnCfg<float> { static constexpr int KP = DK + 4, VP = AK + 4; };

// slot of key kk (0..31) inside a 32-key group of the V^T image: swap bits 2 and 3, so that
// the 8 contiguous slots [16s + 8h, +8) hold keys 16s + 8(j>>2) + 4h + (j&3), j = 0..7 —
// the k-order in which accumulator registers 8s..8s+7 of S^T present P^T (see mma.h).
__device__ inline int vt_pos(int kk) { return (kk & ~0xC) | ((kk & 4) << 1) | ((kk & 8) >> 1); }

// keep the first `nvalid` elements of a 16-byte chunk, zero the rest (nvalid may be <= 0 or >= the chunk size)
template <typename T> __device__ inline uint4 zero_tail(uint4 v, int nvalid);
template <> __device__ inline uint4 zero_tail<float>(uint4 v, int nvalid) {
  return make_uint4(nvalid > 0 ? v.x : 0u, nvalid > 1 ? v.y : 0u, nvalid > 2 ? v.z : 0u, nvalid > 3 ? v.w : 0u);
}
template <> __device__ inline uint4 zero_tail<bf16_t>(uint4 v, int nvalid) {
  auto pair = [&](uint32_t w, int first) {   // elements `first` (low half) and `first + 1` (high half)
    return (nvalid > first ? (w & 0x0000FFFFu) : 0u) | (nvalid > first + 1 ? (w & 0xFFFF0000u) : 0u);
  };
  return make_uint4(pair(v.x, 0), pair(v.y, 2), pair(v.z, 4), pair(v.w, 6));
}

template <typename T, bool CAUSAL, bool BIAS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 3))) void attn_kernel(AttnArgs a) {
  using Cfg = AttnCfg<T>;
  constexpr int EPC = 16 / sizeof(T);
  extern __shared__ __align__(16) unsigned char smem[];
  T* Ks = reinterpret_cast<T*>(smem);                       // [AK][KP]
  T* Vt = Ks + AK * Cfg::KP;                                // [DK][VP]  (transposed, permuted key slots)
  float* tb = reinterpret_cast<float*>(Vt + DK * Cfg::VP) + TB_PAD;  // [-TB_PAD, Sq+Sk-1) bias by (key - q) + Sq - 1

  const int B = a.B, H = a.H, Sq = a.Sq, Sk = a.Sk, Sp = a.Sp;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  // XCD-aware block order (workgroup id -> XCD is id % 8, each XCD has its own L2): all query tiles of a
  // (clip, head) run on ONE XCD, back to back, so its K/V is fetched into that L2 once instead of once per
  // query tile (PMC: 433 MB fetched per launch against 85 MB of Q/K/V with the row-major order).
  const int nq = (Sq + AQ - 1) / AQ;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int bh = xcd + 8 * (slot / nq), qt = slot - (slot / nq) * nq;
  if (bh >= B * H) return;          // grid is padded to a multiple of 8 (clip, head) pairs
  const int b = bh / H, hh = bh - b * H;
  const int q0 = qt * AQ + wave * 32;
  const T* Q = reinterpret_cast<const T*>(a.Q) + (int64_t)bh * Sq * DK;
  const T* Kg = reinterpret_cast<const T*>(a.K) + (int64_t)bh * Sk * DK;
  const T* Vtg = reinterpret_cast<const T*>(a.Vt) + (int64_t)bh * DK * Sp;      // V^T of this (clip, head): [64][Sp]

  if constexpr (BIAS) {
    // 8 entries per thread in flight at once (the plain loop compiles to one load -> wait -> store round trip per iteration)
    const float* tabg = a.bias_tab + (int64_t)hh * a.tab_stride + a.tab_center - (Sq - 1);
    const int ntab = Sq + Sk - 1;
    float tv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) tv[j] = tabg[min(tid + j * 256, ntab - 1)];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (tid + j * 256 < ntab) tb[tid + j * 256] = tv[j];
    for (int i = tid + 2048; i < ntab; i += 256) tb[i] = tabg[i];
    if (tid < TB_PAD) tb[tid - TB_PAD] = 0.f;     // only reached by query rows past Sq, which are never stored
  }

  // Q fragments (B operand): lane (r,h) holds Q[q0 + r][16 s + 8 h + j]
  const int qrow = min(q0 + r, Sq - 1);
  Frag<T> qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = load_frag(Q + (int64_t)qrow * DK + s * 16 + 8 * h);

  f32x16 o[2] = {zero_acc(), zero_acc()};
  float m_run = -1e30f, l_run = 0.f;
  const int my_q = q0 + r;

  // causal: keys beyond the last query of this workgroup's tile are never needed
  const int kend = CAUSAL ? min(Sk, qt * AQ + AQ) : Sk;
  const int ntiles = ceil_div(kend, AK);
  // K / V^T tiles are prefetched into registers one tile ahead (the loads of tile kt+1 are in flight while
  // tile kt is multiplied): staged straight from global memory to LDS every tile paid a full memory round trip
  // between its two barriers.  bf16: 2 + 2 chunks of 16 bytes per thread; fp32: 4 + 4.
  constexpr int KCH = AK * (DK / EPC) / 256;                    // K chunks per thread
  constexpr int VCH = DK * (AK / EPC) / 256;                    // V^T chunks per thread
  static_assert(KCH == VCH && (KCH == 2 || KCH == 4), "tile staging below is written for 2 or 4 chunks per thread");
  // named scalars, not arrays: hipcc 7.2 demotes register arrays that live across the loop to scratch
  uint4 kr0, kr1, kr2, kr3, vr0, vr1, vr2, vr3;
  kr2 = kr3 = vr2 = vr3 = make_uint4(0, 0, 0, 0);
#define M2M_AT_LDK(i, kt)                                                                     \
  {                                                                                           \
    const int c = tid + (i) * 256;                                                            \
    const int key = c / (DK / EPC), dc = c % (DK / EPC);                                      \
    const int gk = min((kt) * AK + key, Sk - 1);                                              \
    kr##i = *reinterpret_cast<const uint4*>(Kg + (int64_t)gk * DK + dc * EPC);                \
  }
#define M2M_AT_LDV(i, kt)                                                                     \
  {                                                                                           \
    const int c = tid + (i) * 256;                                                            \
    const int d = c / (AK / EPC), kc = c % (AK / EPC);                                        \
    vr##i = *reinterpret_cast<const uint4*>(Vtg + (int64_t)d * Sp + (kt) * AK + kc * EPC);    \
  }
#define M2M_AT_FETCH(kt)                                                                      \
  {                                                                                           \
    M2M_AT_LDK(0, kt) M2M_AT_LDK(1, kt) if constexpr (KCH == 4) { M2M_AT_LDK(2, kt) M2M_AT_LDK(3, kt) } \
    M2M_AT_LDV(0, kt) M2M_AT_LDV(1, kt) if constexpr (VCH == 4) { M2M_AT_LDV(2, kt) M2M_AT_LDV(3, kt) } \
  }
#define M2M_AT_STK(i)                                                                         \
  {                                                                                           \
    const int c = tid + (i) * 256;                                                            \
    const int key = c / (DK / EPC), dc = c % (DK / EPC);                                      \
    *reinterpret_cast<uint4*>(Ks + key * Cfg::KP + dc * EPC) = kr##i;                         \
  }
  // columns past Sk of the V^T rows are uninitialised memory: zero them (0 * NaN would poison P.V) — in the one tile that
  // holds the end of the keys only (wave-uniform `tail`): done for every tile the masking was 50 of ~450 VALU instructions per tile
#define M2M_AT_STV(i, kt)                                                                     \
  {                                                                                           \
    const int c = tid + (i) * 256;                                                            \
    const int d = c / (AK / EPC), kc = c % (AK / EPC);                                        \
    const int nvalid = Sk - ((kt) * AK + kc * EPC);               /* valid elements of this chunk */ \
    const uint4 vv = tail ? zero_tail<T>(vr##i, nvalid) : vr##i;                              \
    const int kl = kc * EPC;                                                                  \
    T* dst = Vt + d * Cfg::VP + (kl & 32);                                                    \
    if constexpr (EPC == 8) {                                                                 \
      *reinterpret_cast<uint2*>(dst + vt_pos(kl & 31)) = make_uint2(vv.x, vv.y);              \
      *reinterpret_cast<uint2*>(dst + vt_pos((kl & 31) + 4)) = make_uint2(vv.z, vv.w);        \
    } else {                                                                                  \
      *reinterpret_cast<uint4*>(dst + vt_pos(kl & 31)) = vv;                                  \
    }                                                                                         \
  }
  if (ntiles > 0) M2M_AT_FETCH(0)
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();
    // ---- stage K (row-major) and V^T (already transposed in memory; key slots permuted to the
    //      accumulator k-order in whole 4-key groups, so it is 8/16-byte copies) ----
    const bool tail = (kt + 1) * AK > Sk;
    M2M_AT_STK(0) M2M_AT_STK(1) if constexpr (KCH == 4) { M2M_AT_STK(2) M2M_AT_STK(3) }
    M2M_AT_STV(0, kt) M2M_AT_STV(1, kt) if constexpr (VCH == 4) { M2M_AT_STV(2, kt) M2M_AT_STV(3, kt) }
    __syncthreads();
    if (kt + 1 < ntiles) M2M_AT_FETCH(kt + 1)
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int kbase = kt * AK + sub * 32;
      if (kbase >= kend) break;  // uniform
      f32x16 st = zero_acc();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        Frag<T> kf = load_frag(Ks + (sub * 32 + r) * Cfg::KP + s * 16 + 8 * h);
        mma16(st, kf, qf[s]);
      }
      // scores for query my_q: element i is key kbase + acc_row(i, lane)
      float p[16];
      float mx = -1e30f;
      // interior sub-tiles (every key exists and, when causal, lies at or below every query of this wave) need
      // neither the masks nor the index clamps: the bias is then 16 LDS reads at compile-time offsets from one
      // per-lane base (the table has TB_PAD spare entries below index 0 for the query rows past Sq)
      const bool interior = kbase + 32 <= Sk && (!CAUSAL || kbase + 31 <= q0);
      if (interior) {
        const float* tbp = tb + (kbase - my_q + (Sq - 1) + 4 * h);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float sc = st[i];
          if constexpr (BIAS) sc += tbp[(i & 3) + 8 * (i >> 2)];
          p[i] = sc;
          mx = fmaxf(mx, sc);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int key = kbase + acc_row(i, lane);
          float sc = -1e30f;
          if (key < Sk && (!CAUSAL || key <= my_q)) {
            sc = st[i];
            if constexpr (BIAS) {
              int rel = key - my_q + (Sq - 1);
              rel = min(max(rel, -TB_PAD), Sq + Sk - 2);  // rows beyond Sq (clamped q) are discarded later
              sc += tb[rel];
            }
          }
          p[i] = sc;
          mx = fmaxf(mx, sc);
        }
      }
      mx = fmaxf(mx, lane_xor<32>(mx));
      const float m_new = fmaxf(m_run, mx);
      // exp(x - m) as ONE fma + the hardware exp2: exp2(x * log2(e) - m * log2(e))  (the sub / mul / exp2 form of
      // __expf(x - m) costs one more VALU op per score, and this loop is VALU-bound: ~3x its MFMA time)
      constexpr float L2E = 1.4426950408889634f;
      const float mneg = -m_new * L2E;
      const float alpha = __builtin_amdgcn_exp2f(fmaf(m_run, L2E, mneg));
      float psum = 0.f;
      if constexpr (sizeof(T) == 2) {
        // bf16 mode: the exponents' arguments as 8 packed fmas (the same values as 16 scalar ones) and the row sum as two
        // interleaved partial sums (8 packed adds; the fp32 mode keeps the sequential order its ids were pinned with)
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        const f32x2 l2 = {L2E, L2E}, mn = {mneg, mneg};
        f32x2 ps = {0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 16; i += 2) {
          f32x2 v = {p[i], p[i + 1]};
          v = __builtin_elementwise_fma(v, l2, mn);
          v.x = __builtin_amdgcn_exp2f(v.x);
          v.y = __builtin_amdgcn_exp2f(v.y);
          ps += v;
          p[i] = v.x;
          p[i + 1] = v.y;
        }
        psum = ps.x + ps.y;
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          p[i] = __builtin_amdgcn_exp2f(fmaf(p[i], L2E, mneg));
          psum += p[i];
        }
      }
      psum += lane_xor<32>(psum);
      l_run = l_run * alpha + psum;
      m_run = m_new;
      // the running maximum rarely moves after the first tiles: when no lane of the wave saw a new maximum every alpha
      // is exactly 1 and the 32 rescaling multiplies are skipped (wave-uniform branch, results unchanged)
      if (__ballot(alpha != 1.0f) != 0ull) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          o[0][i] *= alpha;
          o[1][i] *= alpha;
        }
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float pp[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) pp[j] = p[8 * s2 + j];
        const Frag<T> pf = pack_frag<T>(pp);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          Frag<T> vf = load_frag(Vt + (db * 32 + r) * Cfg::VP + sub * 32 + s2 * 16 + 8 * h);
          mma16(o[db], vf, pf);
        }
      }
    }
  }
#undef M2M_AT_LDK
#undef M2M_AT_LDV
#undef M2M_AT_FETCH
#undef M2M_AT_STK
#undef M2M_AT_STV
  // ---- normalise and store: O^T element i of block db is d = db*32 + acc_row(i), query my_q ----
  if (my_q < Sq) {
    const float inv = 1.0f / l_run;
    T* orow = reinterpret_cast<T*>(a.out) + ((int64_t)b * Sq + my_q) * (H * DK) + hh * DK;
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int i = 0; i < 16; ++i) orow[db * 32 + acc_row(i, lane)] = from_f32<T>(o[db][i] * inv);
  }
}

// ---- bf16 form, round 5: 64 keys per softmax step, double-buffered tiles ----
// The kernel above is bound by neither pipe (PMC at B = 32, S = 864: VALU issue 51 %, matrix core 23 %, 2.3 waves per SIMD
// resident, each alive for 2 550 cycles per 32-key step against ~600 cycles of its own instructions): a wave's 32-key step is ONE
// dependent chain — four K-fragment reads -> four MFMAs into one accumulator -> maximum -> exponentials -> pack -> four MFMAs —
// and a tile costs two workgroup barriers.  This form (bf16 only: the running maximum moves every 64 keys instead of 32 and the
// row sum is kept per half-wave until the end, so results differ in the last bits, and the fp32 mode's ids are pinned to the
// arithmetic above) gives a wave two independent score chains per step (keys 0-31 and 32-63 of the tile, the accumulators
// initialised WITH the bias, so there is no add after the product), one maximum / exchange / rescale per 64 keys, and one barrier
// per tile: tile kt + 1 is written to the other LDS buffer at the top of step kt (every wave has left step kt - 1, which was the
// last reader of that buffer) while tile kt + 2 travels from memory to registers.
#ifdef M2M_AW_STAMP       // diagnostic builds only (tools/aw_stamps.py): shader-clock stamps of wave 0 of one workgroup, pinned in program order
__device__ unsigned long long g_aw_stamp[64];
#define AW_STAMP(i)                                                                               \
  do {                                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                            \
    if (threadIdx.x == 0 && blockIdx.x == 801 && (i) >= 0 && (i) < 64) g_aw_stamp[i] = clock64(); \
    __builtin_amdgcn_sched_barrier(0);                                                            \
  } while (0)
#else
#define AW_STAMP(i) do {} while (0)
#endif

#ifndef M2M_AW_CUT        // diagnostic builds only (tools/aw_variants.sh): bit i leaves a phase of the wide step out at COMPILE time
#define M2M_AW_CUT 0      // (a run-time mask distorted the code: 177 registers, accumulator copies); results are garbage, times are not.
#endif                    // bits: 1 exponentials, 2 P.V MFMAs + V reads, 8 the tile barrier, 16 staging, 64 the maximum's cross-half exchange
#define AW_KEEP(bit) (!((M2M_AW_CUT) & (1 << (bit))))

template <bool CAUSAL, bool BIAS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 3))) void attn_wide_kernel(AttnArgs a) {
  using T = bf16_t;
  using Cfg = AttnCfg<T>;
  constexpr int EPC = 8;
  constexpr int KBUF = AK * Cfg::KP, VBUF = DK * Cfg::VP;
  extern __shared__ __align__(16) unsigned char smem[];
  T* Ks0 = reinterpret_cast<T*>(smem);                      // [2][AK][KP]
  T* Vt0 = Ks0 + 2 * KBUF;                                  // [2][DK][VP]  (transposed, permuted key slots)
  float* tb = reinterpret_cast<float*>(Vt0 + 2 * VBUF) + TB_PAD;

  const int B = a.B, H = a.H, Sq = a.Sq, Sk = a.Sk, Sp = a.Sp;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int nq = (Sq + AQ - 1) / AQ;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int bh = xcd + 8 * (slot / nq), qt = slot - (slot / nq) * nq;
  if (bh >= B * H) return;
  const int b = bh / H, hh = bh - b * H;
  const int q0 = __builtin_amdgcn_readfirstlane(qt * AQ + wave * 32);       // scalar: the branches on it below are wave-uniform
  const T* Q = reinterpret_cast<const T*>(a.Q) + (int64_t)bh * Sq * DK;
  const T* Kg = reinterpret_cast<const T*>(a.K) + (int64_t)bh * Sk * DK;
  const T* Vtg = reinterpret_cast<const T*>(a.Vt) + (int64_t)bh * DK * Sp;
  AW_STAMP(0);

  // the bias table of this head, 8 entries per thread in flight at once (a plain `for (i = tid; i < n; i += 256) tb[i] = tab[i]`
  // compiles to one load -> wait -> store round trip per iteration when the trip count (7 at S = 864) is below the unroll factor:
  // 6 600 of a wave's 56 700 cycles, stamped); Q and the first tile are requested before any of it is waited for
  const float* tabg = a.bias_tab + (int64_t)hh * a.tab_stride + a.tab_center - (Sq - 1);
  const int ntab = Sq + Sk - 1;
  float tv[8];
  if constexpr (BIAS) {
#pragma unroll
    for (int j = 0; j < 8; ++j) tv[j] = tabg[min(tid + j * 256, ntab - 1)];
  }
  const int qrow = min(q0 + r, Sq - 1);
  Frag<T> qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = load_frag(Q + (int64_t)qrow * DK + s * 16 + 8 * h);

  f32x16 o[2] = {zero_acc(), zero_acc()};
  float m_run = -1e30f, l_run = 0.f;       // l_run: this half-wave's keys only; the halves meet after the loop
  const int my_q = q0 + r;
  const int kend = CAUSAL ? min(Sk, qt * AQ + AQ) : Sk;
  const int ntiles = ceil_div(kend, AK);
  constexpr float L2E = 1.4426950408889634f;
  const int far = a.bias_far;

  // One register set of staged tiles: tile t + 1 goes to LDS at the top of step t and the set is re-issued for tile t + 2 at once.
  // (Measured and dropped, twice: two sets, a tile requested two steps ahead, the loop unrolled by two — 87.1 against 85.0 us on
  // the same box at 163 registers; after the wait-count fix below 196 registers = two waves per SIMD, and forced to three it
  // spills: 88.3 against 82.3 us.)
  uint4 ka0, ka1, va0, va1;
  // thread -> chunk maps of the two staging copies (256 threads x 2 chunks of 16 bytes each for K and for V^T)
  const int kkey0 = tid / (DK / EPC), kdc = tid % (DK / EPC);            // K chunk 0: key kkey0, chunk 1: key kkey0 + 32
  const int vd0 = tid / (AK / EPC), vkc = tid % (AK / EPC);              // V^T chunk 0: row vd0, chunk 1: row vd0 + 32
  const int vslot = (vkc * EPC & 32) + vt_pos(vkc * EPC & 31);
  auto fetch = [&](int kt, uint4& k0, uint4& k1, uint4& v0, uint4& v1) __attribute__((always_inline)) {
    k0 = *reinterpret_cast<const uint4*>(Kg + (int64_t)min(kt * AK + kkey0, Sk - 1) * DK + kdc * EPC);
    k1 = *reinterpret_cast<const uint4*>(Kg + (int64_t)min(kt * AK + kkey0 + 32, Sk - 1) * DK + kdc * EPC);
    v0 = *reinterpret_cast<const uint4*>(Vtg + (int64_t)vd0 * Sp + kt * AK + vkc * EPC);
    v1 = *reinterpret_cast<const uint4*>(Vtg + (int64_t)(vd0 + 32) * Sp + kt * AK + vkc * EPC);
  };
  // V^T columns past Sk are uninitialised memory: zeroed in the one tile that holds the end of the keys (0 * NaN would poison P.V)
  auto store = [&](int kt, const uint4& k0, const uint4& k1, uint4 v0, uint4 v1) __attribute__((always_inline)) {
    T* kb = Ks0 + (kt & 1) * KBUF;
    T* vb = Vt0 + (kt & 1) * VBUF;
    *reinterpret_cast<uint4*>(kb + kkey0 * Cfg::KP + kdc * EPC) = k0;
    *reinterpret_cast<uint4*>(kb + (kkey0 + 32) * Cfg::KP + kdc * EPC) = k1;
    if ((kt + 1) * AK > Sk) {
      const int nvalid = Sk - (kt * AK + vkc * EPC);
      v0 = zero_tail<T>(v0, nvalid);
      v1 = zero_tail<T>(v1, nvalid);
    }
    *reinterpret_cast<uint2*>(vb + vd0 * Cfg::VP + vslot) = make_uint2(v0.x, v0.y);
    *reinterpret_cast<uint2*>(vb + vd0 * Cfg::VP + vslot + 8) = make_uint2(v0.z, v0.w);
    *reinterpret_cast<uint2*>(vb + (vd0 + 32) * Cfg::VP + vslot) = make_uint2(v1.x, v1.y);
    *reinterpret_cast<uint2*>(vb + (vd0 + 32) * Cfg::VP + vslot + 8) = make_uint2(v1.z, v1.w);
  };
  // top of step kt: tile kt + 1 to the buffer step kt - 1 read last, the set re-issued for tile kt + 2
  // (measured: the same placed after the step's Q.K MFMAs, so that the wait for the staged registers sits under the matrix core:
  // 74.1 / 75.0 against 74.7 / 75.5 us on the same box — inside the spread; left at the top)
#define M2M_AW_TOP(kt)                                             \
  if ((kt) + 1 < ntiles) {                                         \
    store((kt) + 1, ka0, ka1, va0, va1);                           \
    if ((kt) + 2 < ntiles) fetch((kt) + 2, ka0, ka1, va0, va1);    \
  }
  if (ntiles > 0) fetch(0, ka0, ka1, va0, va1);
  if constexpr (BIAS) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (tid + j * 256 < ntab) tb[tid + j * 256] = tv[j];
    for (int i = tid + 2048; i < ntab; i += 256) tb[i] = tabg[i];      // tables past 2 048 entries (Sq + Sk > 2 049)
    if (tid < TB_PAD) tb[tid - TB_PAD] = 0.f;
  }
  if (ntiles > 0) {
    store(0, ka0, ka1, va0, va1);
    if (ntiles > 1) fetch(1, ka0, ka1, va0, va1);
  }
  __syncthreads();
  // Q must have ARRIVED here, as far as the compiler's wait-count bookkeeping goes: without this it kept the four Q loads pending
  // into the loop and put s_waitcnt vmcnt(3) .. vmcnt(0) in front of the Q.K MFMAs — which in the steady state wait for the four
  // tile loads issued a moment earlier, a full memory latency inside every step (found in the ISA; cut-variant timings: the Q.K
  // phase 17.6 us and the staging 12 us of a 92 us kernel)
#pragma unroll
  for (int s = 0; s < 4; ++s) asm volatile("" : "+v"(qf[s].v.x), "+v"(qf[s].v.y), "+v"(qf[s].v.z), "+v"(qf[s].v.w));
  AW_STAMP(1);
  const bool live = q0 < Sq;      // a wave whose 32 queries all lie past Sq (S = 864: one of 28) stages and synchronises, nothing else

  // ---- 64 keys, every one of them exists and is visible to every query of this wave ----
  auto wide_step = [&](int kt) __attribute__((always_inline)) {
    const T* Kb = Ks0 + (kt & 1) * KBUF;
    const T* Vb = Vt0 + (kt & 1) * VBUF;
    const int kbase = kt * AK;
    f32x16 s0, s1;
    // T5's bias is one value per side beyond `far` positions (the last bucket): a tile that far from all 32 queries of the wave
    // (8 or 9 of the 13 at S = 864) adds a constant c to every score, which moves into the exponent's offset — exp2((s + c - m) log2e)
    // — and into the maximum; such a step reads no table and starts its accumulators from the literal zero
    float cfar = 0.f;
    bool near = true;
    if constexpr (BIAS) near = far == 0 || (kbase + AK - 1 - q0 > -far && kbase - (q0 + 31) < far);      // wave-uniform (q0 is scalar)
    {
      const Frag<T> kf0 = load_frag(Kb + r * Cfg::KP + 8 * h);
      const Frag<T> kf1 = load_frag(Kb + (32 + r) * Cfg::KP + 8 * h);
      if (BIAS && near) {
        const float* tbp = tb + (kbase - my_q + (Sq - 1) + 4 * h);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          s0[i] = tbp[(i & 3) + 8 * (i >> 2)];
          s1[i] = tbp[32 + (i & 3) + 8 * (i >> 2)];
        }
        mma16(s0, kf0, qf[0]);
        mma16(s1, kf1, qf[0]);
      } else {
        if constexpr (BIAS) cfar = tb[kbase - my_q + (Sq - 1) + 4 * h];
        s0 = zero_acc();
        s1 = zero_acc();
        mma16(s0, kf0, qf[0]);       // the zero is the instruction's literal operand: no register is written for it
        mma16(s1, kf1, qf[0]);
      }
    }
#pragma unroll
    for (int s = 1; s < 4; ++s) {
      const Frag<T> kf0 = load_frag(Kb + r * Cfg::KP + s * 16 + 8 * h);
      const Frag<T> kf1 = load_frag(Kb + (32 + r) * Cfg::KP + s * 16 + 8 * h);
      mma16(s0, kf0, qf[s]);
      mma16(s1, kf1, qf[s]);
    }
    AW_STAMP(kt >= 4 && kt < 8 ? 4 + (kt - 4) * 8 : -1);
    // two running chains of max3 (a pair-wise tree makes the compiler canonicalise every matrix-core output first: 3 ops per pair)
    float mx = s0[0], my = s1[0];
#pragma unroll
    for (int i = 1; i < 16; i += 2) {
      mx = fmaxf(fmaxf(mx, s0[i]), s0[(i + 1) & 15]);
      my = fmaxf(fmaxf(my, s1[i]), s1[(i + 1) & 15]);
    }
    mx = fmaxf(mx, my) + cfar;
    if constexpr (AW_KEEP(6)) mx = fmaxf(mx, lane_xor<32>(mx));
    // m_run is the REFERENCE the exponentials are taken against, not necessarily the running maximum: it moves (and the 32 output
    // accumulators and the row sum are rescaled) only when some row's new maximum exceeds its reference by more than AW_TAU — with
    // 32 rows per wave SOME row sets a new maximum in almost every tile (1 - (12/13)^32 = 92 % at the 13th), so rescaling at every
    // new maximum meant 16 packed multiplies + an exponential in nearly every step.  Until a row is re-referenced its weights may
    // reach e^AW_TAU = 245: nothing to fp32 accumulators or to bf16's exponent, and the quotient o / l does not see the reference.
    constexpr float AW_TAU = 5.5f;
    if (__ballot(mx > m_run + AW_TAU) != 0ull) {
      const float m_new = fmaxf(m_run, mx);
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * L2E);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        o[0][i] *= alpha;
        o[1][i] *= alpha;
      }
    }
    const float mneg = (cfar - m_run) * L2E;
    AW_STAMP(kt >= 4 && kt < 8 ? 5 + (kt - 4) * 8 : -1);
    float ps0 = 0.f, ps1 = 0.f, ps2 = 0.f, ps3 = 0.f;
    float p[32];
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
#if (M2M_AW_CUT) & 1
      const float u0 = fmaf(s0[i], L2E, mneg), u1 = fmaf(s0[i + 1], L2E, mneg), v0 = fmaf(s1[i], L2E, mneg), v1 = fmaf(s1[i + 1], L2E, mneg);
#else
      const float u0 = __builtin_amdgcn_exp2f(fmaf(s0[i], L2E, mneg)), u1 = __builtin_amdgcn_exp2f(fmaf(s0[i + 1], L2E, mneg));
      const float v0 = __builtin_amdgcn_exp2f(fmaf(s1[i], L2E, mneg)), v1 = __builtin_amdgcn_exp2f(fmaf(s1[i + 1], L2E, mneg));
#endif
      ps0 += u0;
      ps1 += u1;
      ps2 += v0;
      ps3 += v1;
      p[i] = u0;
      p[i + 1] = u1;
      p[16 + i] = v0;
      p[16 + i + 1] = v1;
    }
    // (measured and dropped, twice: the row sums from the matrix core — a block of ones times P^T, 4 more MFMAs per step instead of
    // 32 adds: 88.7 against 86.6 us on the same box, and 77.5 against 76.6 on the final kernel)
    l_run += (ps0 + ps1) + (ps2 + ps3);
    AW_STAMP(kt >= 4 && kt < 8 ? 6 + (kt - 4) * 8 : -1);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float pp[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pp[j] = p[8 * g + j];
      const Frag<T> pf = pack_frag<T>(pp);
      if constexpr (AW_KEEP(1)) {
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const Frag<T> vf = load_frag(Vb + (db * 32 + r) * Cfg::VP + g * 16 + 8 * h);
          mma16(o[db], vf, pf);
        }
      } else {
        o[0][g] += __builtin_bit_cast(float, pf.v.x ^ pf.v.y ^ pf.v.z ^ pf.v.w);
      }
    }
  };
  // ---- a last tile of exactly 32 keys, all visible (S = 864 = 13 x 64 + 32): one chain of the wide step, no masks ----
  auto half_step = [&](int kt) __attribute__((always_inline)) {
    const T* Kb = Ks0 + (kt & 1) * KBUF;
    const T* Vb = Vt0 + (kt & 1) * VBUF;
    f32x16 s0;
    if constexpr (BIAS) {
      const float* tbp = tb + (kt * AK - my_q + (Sq - 1) + 4 * h);
#pragma unroll
      for (int i = 0; i < 16; ++i) s0[i] = tbp[(i & 3) + 8 * (i >> 2)];
    } else {
      s0 = zero_acc();
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) mma16(s0, load_frag(Kb + r * Cfg::KP + s * 16 + 8 * h), qf[s]);
    float mx = s0[0];
#pragma unroll
    for (int i = 1; i < 16; i += 2) mx = fmaxf(fmaxf(mx, s0[i]), s0[(i + 1) & 15]);
    mx = fmaxf(mx, lane_xor<32>(mx));
    const float m_new = fmaxf(m_run, mx);
    const float mneg = -m_new * L2E;
    const float alpha = __builtin_amdgcn_exp2f(fmaf(m_run, L2E, mneg));
    float ps0 = 0.f, ps1 = 0.f;
    float p[16];
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
      p[i] = __builtin_amdgcn_exp2f(fmaf(s0[i], L2E, mneg));
      p[i + 1] = __builtin_amdgcn_exp2f(fmaf(s0[i + 1], L2E, mneg));
      ps0 += p[i];
      ps1 += p[i + 1];
    }
    l_run = fmaf(l_run, alpha, ps0 + ps1);
    m_run = m_new;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      o[0][i] *= alpha;
      o[1][i] *= alpha;
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      float pp[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pp[j] = p[8 * g + j];
      const Frag<T> pf = pack_frag<T>(pp);
#pragma unroll
      for (int db = 0; db < 2; ++db) mma16(o[db], load_frag(Vb + (db * 32 + r) * Cfg::VP + g * 16 + 8 * h), pf);
    }
  };
  // ---- the tile with the end of the keys (and, causal, the tiles on the diagonal): 32 keys at a time, masked ----
  auto masked_step = [&](int kt) __attribute__((always_inline)) {
    const T* Kb = Ks0 + (kt & 1) * KBUF;
    const T* Vb = Vt0 + (kt & 1) * VBUF;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      const int kb32 = kt * AK + sub * 32;
      if (kb32 >= kend) break;  // uniform
      f32x16 st = zero_acc();
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const Frag<T> kf = load_frag(Kb + (sub * 32 + r) * Cfg::KP + s * 16 + 8 * h);
        mma16(st, kf, qf[s]);
      }
      float p[16];
      float mx = -1e30f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int key = kb32 + acc_row(i, lane);
        float sc = -1e30f;
        if (key < Sk && (!CAUSAL || key <= my_q)) {
          sc = st[i];
          if constexpr (BIAS) {
            int rel = key - my_q + (Sq - 1);
            rel = min(max(rel, -TB_PAD), Sq + Sk - 2);
            sc += tb[rel];
          }
        }
        p[i] = sc;
        mx = fmaxf(mx, sc);
      }
      mx = fmaxf(mx, lane_xor<32>(mx));
      const float m_new = fmaxf(m_run, mx);
      const float mneg = -m_new * L2E;
      const float alpha = __builtin_amdgcn_exp2f(fmaf(m_run, L2E, mneg));
      float psum = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        p[i] = __builtin_amdgcn_exp2f(fmaf(p[i], L2E, mneg));
        psum += p[i];
      }
      l_run = fmaf(l_run, alpha, psum);
      m_run = m_new;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        o[0][i] *= alpha;
        o[1][i] *= alpha;
      }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float pp[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) pp[j] = p[8 * s2 + j];
        const Frag<T> pf = pack_frag<T>(pp);
#pragma unroll
        for (int db = 0; db < 2; ++db) {
          const Frag<T> vf = load_frag(Vb + (db * 32 + r) * Cfg::VP + sub * 32 + s2 * 16 + 8 * h);
          mma16(o[db], vf, pf);
        }
      }
    }
  };

  // Leading tiles whose 64 keys all exist and are visible to every query of this wave take the wide step, the rest follow in a loop of
  // their own (two loops, not one with a branch: with both bodies in one loop the compiler copied the 32 output accumulators between
  // two register sets every step).  Every wave of the workgroup passes ntiles barriers whichever loop it is in.
  int n_wide = min(ntiles, Sk / AK);
  if constexpr (CAUSAL) n_wide = min(n_wide, max(0, (q0 + 1) / AK));
  if (!live) n_wide = 0;
  int kt = 0;
  for (; kt < n_wide; ++kt) {
    AW_STAMP(kt >= 4 && kt < 8 ? 2 + (kt - 4) * 8 : -1);
    if constexpr (AW_KEEP(4)) {
      M2M_AW_TOP(kt)
    }
    AW_STAMP(kt >= 4 && kt < 8 ? 3 + (kt - 4) * 8 : -1);
    wide_step(kt);
    AW_STAMP(kt >= 4 && kt < 8 ? 7 + (kt - 4) * 8 : -1);
    if constexpr (AW_KEEP(3)) __syncthreads();
    AW_STAMP(kt >= 4 && kt < 8 ? 8 + (kt - 4) * 8 : -1);
  }
  AW_STAMP(40);
  if (live && kt == ntiles - 1 && Sk - kt * AK == 32 && (!CAUSAL || kt * AK + 31 <= q0)) {
    half_step(kt);          // the last tile: nothing left to stage
    __syncthreads();
    ++kt;
  }
  for (; kt < ntiles; ++kt) {
    M2M_AW_TOP(kt)
    if (live) masked_step(kt);      // (a branch inside the wide loop made the compiler copy the output accumulators every step)
    __syncthreads();
  }
#undef M2M_AW_TOP
#undef AW_KEEP
  AW_STAMP(41);
  l_run += lane_xor<32>(l_run);
  // ---- normalise, transpose through LDS, store whole rows: a lane owns 32 values of ONE query at a 2-byte granularity spread over
  // the row (stored directly: 32 store instructions per lane, each touching 64 lines); its wave's [32 queries][64] block goes to
  // LDS (the K buffers are free: every wave has passed the last barrier; a wave reads only what it wrote) and leaves as 16-byte
  // pieces, 8 lanes per 128-byte row ----
  {
    const float inv = 1.0f / l_run;
    T* Ow = Ks0 + wave * (32 * Cfg::KP);                  // [32][KP] of this wave (4 x 32 x 72 x 2 B = the two K buffers exactly)
#pragma unroll
    for (int db = 0; db < 2; ++db)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        *reinterpret_cast<uint2*>(Ow + r * Cfg::KP + db * 32 + 8 * j + 4 * h) =
            make_uint2(pack2_bf16(o[db][4 * j] * inv, o[db][4 * j + 1] * inv), pack2_bf16(o[db][4 * j + 2] * inv, o[db][4 * j + 3] * inv));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    T* obase = reinterpret_cast<T*>(a.out) + ((int64_t)b * Sq + q0) * (H * DK) + hh * DK;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int c = it * 64 + lane, row = c >> 3, col = (c & 7) * 8;
      const uint4 v = *reinterpret_cast<const uint4*>(Ow + row * Cfg::KP + col);
      if (q0 + row < Sq) *reinterpret_cast<uint4*>(obase + (int64_t)row * (H * DK) + col) = v;
    }
  }
  AW_STAMP(42);
}

// M2M_ATTN_WIDE=0: the bf16 mode runs the first kernel as well (A/B, and the test that holds the two forms to each other)
static bool attn_wide_on() { return enc_switches_now().attn_wide != 0; }

template <typename T, bool CAUSAL, bool BIAS>
static int launch_attn_tt(const AttnArgs& a, hipStream_t st) {
  using Cfg = AttnCfg<T>;
  const size_t tiles = (size_t)(AK * Cfg::KP + DK * Cfg::VP) * sizeof(T);
  const size_t table = BIAS ? (size_t)(a.Sq + a.Sk - 1 + TB_PAD) * sizeof(float) : 0;
  size_t smem = tiles + table;
  M2M_REQUIRE(smem <= 150 * 1024, "attention: Sq=%d, Sk=%d too long for the LDS bias table", a.Sq, a.Sk);
  dim3 grid((unsigned)(ceil_div(a.Sq, AQ) * ceil_div(a.B * a.H, 8) * 8));
  if constexpr (sizeof(T) == 2) {
    if (attn_wide_on() && 2 * tiles + table <= 150 * 1024) {
      smem = 2 * tiles + table;
      M2M_OPT_IN_LDS((attn_wide_kernel<CAUSAL, BIAS>), 160 * 1024);
      hipLaunchKernelGGL((attn_wide_kernel<CAUSAL, BIAS>), grid, dim3(256), smem, st, a);
      M2M_CHECK_HIP(hipGetLastError());
      return M2M_OK;
    }
  }
  M2M_OPT_IN_LDS((attn_kernel<T, CAUSAL, BIAS>), 160 * 1024);
  hipLaunchKernelGGL((attn_kernel<T, CAUSAL, BIAS>), grid, dim3(256), smem, st, a);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

template <typename T>
static int launch_attn_t(const AttnArgs& a, bool causal, hipStream_t st) {
  if (causal) {
    M2M_REQUIRE(a.bias_tab != nullptr && a.Sq == a.Sk, "attention: the causal form is the decoder self-attention (bias table, Sq == Sk)");
    return launch_attn_tt<T, true, true>(a, st);
  }
  return a.bias_tab ? launch_attn_tt<T, false, true>(a, st) : launch_attn_tt<T, false, false>(a, st);
}

int launch_attn(int precision, const AttnArgs& a, bool causal, hipStream_t st) {
  M2M_REQUIRE(a.Sq >= 1 && a.Sk >= 1 && a.Sp >= a.Sk && a.Sp % 4 == 0, "attention: bad geometry Sq=%d Sk=%d Sp=%d", a.Sq, a.Sk, a.Sp);
  return precision == M2M_PREC_BF16 ? launch_attn_t<bf16_t>(a, causal, st) : launch_attn_t<float>(a, causal, st);
}

// V [B*H][S][64] -> V^T [B*H][64][Sp] (the cross-attention values are stored row-major for the decode
// kernels; the batched teacher-forced pass wants them as the MFMA A operand of O^T = V^T P^T)
template <typename T>
__global__ __launch_bounds__(256) void transpose_v_kernel(const T* __restrict__ v, T* __restrict__ vt, int S, int Sp) {
  __shared__ T tile[64][DK + 2];
  const int bh = blockIdx.y, s0 = blockIdx.x * 64;
  const T* src = v + (int64_t)bh * S * DK;
  T* dst = vt + (int64_t)bh * DK * Sp;
  for (int i = threadIdx.x; i < 64 * DK; i += 256) {
    const int sl = i / DK, d = i % DK;
    tile[sl][d] = (s0 + sl < S) ? src[(int64_t)(s0 + sl) * DK + d] : from_f32<T>(0.f);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * DK; i += 256) {
    const int d = i / 64, sl = i % 64;
    if (s0 + sl < Sp) dst[(int64_t)d * Sp + s0 + sl] = tile[sl][d];
  }
}

int launch_transpose_v(int precision, const void* v, void* vt, int BH, int S, int Sp, hipStream_t st) {
  dim3 grid((unsigned)ceil_div(Sp, 64), (unsigned)BH);
  if (precision == M2M_PREC_BF16) hipLaunchKernelGGL(transpose_v_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)v, (bf16_t*)vt, S, Sp);
  else hipLaunchKernelGGL(transpose_v_kernel<float>, grid, dim3(256), 0, st, (const float*)v, (float*)vt, S, Sp);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

}  // namespace m2m

#ifdef M2M_AW_STAMP
extern "C" int m2m_debug_aw_stamps(unsigned long long* out_host) {      // diagnostic builds only (not declared in the public header)
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(m2m::g_aw_stamp), sizeof(unsigned long long) * 64) == hipSuccess ? 0 : -1;
}
#endif
