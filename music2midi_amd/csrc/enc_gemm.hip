// Encoder-side MFMA products: gemm_kernel with its fused epilogues, the row-panel residual product (resid_panel_kernel) and the
// fused RMSNorm + GEMM (norm_gemm_kernel), their launchers, and the latched switches that choose between them (EncSwitches, t5.h).
// Inference (t5_api.hip) and training (train.hip) both go through launch_gemm / launch_norm_gemm.
//
// The kernels are templated on the storage type T of the precision mode: float (f32-input MFMA, exact fp32 FMA chains: parity mode)
// or bf16 (bf16 MFMA, fp32 accumulate: throughput mode).
#include "env.h"
#include "mma.h"
#include "rms.h"
#include "t5.h"

#include <utility>

namespace m2m {

// ================================================================= GEMM ====
// C[M,N] = A[M,K] * W[N,K]^T.  128x128 output tile per 256-thread workgroup, BK = 64 (bf16) / 32 (fp32),
// 2x2 waves each owning 64x64 (2x2 MFMA 32x32 tiles), register-prefetched LDS staging.
// TF = 1 is the small-problem variant: 64x64 tiles (one 32x32 MFMA tile per wave, 18 KB of LDS, ~8 workgroups per CU).
// A product whose 128x128 tiling gives fewer workgroups than two rounds of the 256 CUs (the N = 384 residual / dX
// products of a 16-clip training step: 33 x 3 = 99 tiles) is bound by ONE workgroup's load -> LDS -> MFMA latency
// chain per CU; four times the tiles at eight per CU hide it.  Same k order per output element: bit-identical results.
//
// gemm_kernel is ONE function on purpose: as a body over inlined pieces (tile map, loops, one function per epilogue) its products
// of a 16-clip training step measured 1 - 8 % slower against the same machine code's parent.  Its parts, in order: the
// tile map, the prologue prefetches of two epilogues, one of the two main loops, the LDS-staged epilogues (bf16: heads, gate gradient,
// training gate, gated), which leave by return, and the per-element store that serves the rest (store, store-f32, resid, and the
// fp32 gated / gated16 / heads).

template <typename T> struct TileCfg;
template <> struct TileCfg<bf16_t> {
  static constexpr int BK = 64;                              // 16 MFMAs per wave between barriers
  static constexpr int PITCH = BK + 8;                       // elements per LDS row (144 B)
  static constexpr int CPR = BK * 2 / 16;                    // 16-byte chunks per row = 8
};
template <> struct TileCfg<float> {
  static constexpr int BK = 32;
  static constexpr int PITCH = BK + 4;                       // 144 B
  static constexpr int CPR = BK * 4 / 16;                    // 8
};

// k extent per step: the small-tile variant stages twice the k of the big one (same 35 KB of LDS): its products are the
// latency-bound ones, and half the steps halve the dependent load -> LDS -> MFMA chain of a workgroup
template <typename T, int TF> struct TileCfgT {
  static constexpr int BK = TileCfg<T>::BK * (TF == 1 ? 2 : 1);
  static constexpr int PITCH = BK + (TileCfg<T>::PITCH - TileCfg<T>::BK);
  static constexpr int CPR = BK * (int)sizeof(T) / 16;
};

// Which gemm_kernel<T, EPI, TF, NS> exist — the one statement of it: the kernel asserts it, the launcher instantiates exactly these
// and words its errors by it.  The LDS-staged epilogues are written for 128x128 tiles (TF = 2), the small tile (TF = 1) has the plain
// ones and the gate-gradient epilogue, which is a bf16 small-tile path; the training gate epilogue is a bf16 path.
constexpr bool gemm_epi_plain(int epi) { return epi == EPI_STORE || epi == EPI_STORE_F32 || epi == EPI_RESID; }
constexpr bool gemm_variant_exists(bool bf16, int epi, int tf) {
  if (epi == EPI_GATED_BWD) return bf16 && tf == 1;
  if (tf == 1) return gemm_epi_plain(epi);
  if (epi == EPI_GATED_TRAIN) return bf16;
  return tf == 2 && (gemm_epi_plain(epi) || epi == EPI_GATED || epi == EPI_GATED16 || epi == EPI_HEADS);
}
// ... and with which ring depth NS (0: the register-staged loop; the LDS-DMA loop is written for bf16 operands)
constexpr int gemm_ring_deep(int tf) { return tf == 1 ? 4 : 3; }
constexpr int gemm_ring_shallow(int tf) { return tf == 1 ? 3 : 2; }
constexpr bool gemm_ring_exists(bool bf16, int tf, int ns) { return ns == 0 || (bf16 && (ns == gemm_ring_deep(tf) || ns == gemm_ring_shallow(tf))); }

// operand tiles in LDS: one block (the staged epilogues re-use all of it)
template <typename T, int TF, int NS> constexpr int gemm_lds_elems() {
  return NS > 0 ? NS * (64 * TF + 64 * TF) * 64 : (64 * TF + 64 * TF) * TileCfgT<T, TF>::PITCH;
}

#ifdef M2M_GEMM_STAMP      // diagnostic builds only (tools/gemm_stamps.py): phase times of one workgroup (100 MHz s_memrealtime), per (EPI, TF)
__device__ unsigned long long g_gemm_stamp[8][3][8];
#define GEMM_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x == 77) g_gemm_stamp[EPI][TF][i] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define GEMM_WAITLOADS() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define GEMM_STAMP(i) do {} while (0)
#define GEMM_WAITLOADS() do {} while (0)
#endif

// NS > 0 (bf16 only) is the LDS-DMA form of the main loop.  The register-staged loop keeps ONE k-step of loads in flight (a
// second register set costs the occupancy that hides the rest), so every k-step of a workgroup pays a memory round trip:
// ~0.45 us per 64 k, measured with stamps — and the products of a 16-clip training step run 6 - 36 such steps with one or two
// workgroups per CU.  Here the operand tiles go global -> LDS directly (global_load_lds_dwordx4: no VGPRs, 1 KiB = 8 rows x 128 B
// per wave instruction) into a ring of NS stages of 64 k, NS - 1 stages requested ahead, retired by a COUNTED s_waitcnt
// vmcnt + one raw s_barrier per step (a __syncthreads() would drain the ring: its fence waits vmcnt(0)).  The LDS image is
// lane-linear per instruction, so the bank swizzle sits on the SOURCE address: 16-byte chunk c of tile row r is stored at slot
// c ^ ((r >> 1) & 7) of its 128-byte row, and the fragment reads apply the same involution (16 lanes then cover all 64 banks).
// Same k order per output element as the register-staged loop: bit-identical results (tests/test_gemm_dma_gpu.py).
template <int N> __device__ inline void m2m_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

template <typename T, int EPI, int TF = 2, int NS = 0>
__global__ __launch_bounds__(256) void gemm_kernel(GemmArgs g) {
  using Cfg = TileCfgT<T, TF>;
  constexpr int BM = 64 * TF, BN = 64 * TF, WT = 32 * TF;      // tile, and the square each of the 2x2 waves owns
  static_assert(gemm_variant_exists(sizeof(T) == 2, EPI, TF) && gemm_ring_exists(sizeof(T) == 2, TF, NS), "no such gemm_kernel (gemm_variant_exists, gemm_ring_exists)");
  constexpr int BK = NS > 0 ? 64 : Cfg::BK;
  constexpr int EPC = 16 / sizeof(T);                          // elements per 16-byte chunk
  constexpr int CHUNKS = BM * Cfg::CPR;                        // per operand tile
  constexpr int PER_THREAD = CHUNKS / 256;
  constexpr int LDS_ELEMS = NS > 0 ? NS * (BM + BN) * 64 : (BM + BN) * Cfg::PITCH;
  __shared__ __align__(1024) T AB[LDS_ELEMS];             // one block: the head-major epilogue re-uses all of it
  T* const As = AB;
  T* const Bs = AB + BM * Cfg::PITCH;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // XCD-aware tile order (workgroup id % 8 picks the XCD, each has its own L2): all column tiles of a row
  // block run back to back on ONE XCD, so the [128 x K] activation tile is fetched into that L2 once instead
  // of once per XCD (PMC: 176-187 MB fetched per launch against 21-28 MB of activations with the row-major
  // order); the weights are small and every XCD keeps its own copy.
  // Column tiles go in groups of g.ng (chosen on the host so that a group's weight rows are <= 2 MB): they stay
  // in the 4 MB L2 while the XCD walks its row blocks, then the next group starts (the 48 column tiles of the
  // cross-K/V projection would otherwise push their own weights out between two row blocks: 850 MB fetched).
  const int ntn = (g.N + BN - 1) / BN, ntm = (g.M + BM - 1) / BM;
  const int mtx = (ntm + 7) / 8;                                 // row blocks per XCD (padded)
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int grp = slot / (mtx * g.ng), rem_ = slot - grp * (mtx * g.ng);
  const int mt = xcd + 8 * (rem_ / g.ng), nt = grp * g.ng + rem_ % g.ng;
  if (mt >= ntm || nt >= ntn) return;   // padding workgroups (uniform)
  const int m0 = mt * BM, n0 = nt * BN;
  const T* A = reinterpret_cast<const T*>(g.A);
  const T* W = reinterpret_cast<const T*>(g.W);
  const int K = g.K;

  f32x16 acc[TF][TF];
#pragma unroll
  for (int i = 0; i < TF; ++i)
#pragma unroll
    for (int j = 0; j < TF; ++j) acc[i][j] = zero_acc();

  const int r = lane & 31, h = lane >> 5;
  // small-tile residual products: the 16 residual values a lane adds to are requested before the k loop (their round trip
  // would otherwise sit between the last MFMA and the store of a workgroup that lives for three k-steps)
  float rpre[16];
  if constexpr (EPI == EPI_RESID && TF == 1) {
    const float* rsrc = g.resid ? g.resid : reinterpret_cast<const float*>(g.out);
    const int col = n0 + wn * WT + r;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = m0 + wm * WT + acc_row(e, lane);
      rpre[e] = (row < g.M && col < g.N) ? rsrc[(int64_t)row * g.ldo + col] : 0.f;
    }
  }
  // gate-gradient epilogue: the tile's a | b chunks (two 16-byte chunks of a, two of b per thread) are requested before the k loop too
  uint4 ga0 = make_uint4(0, 0, 0, 0), ga1 = ga0, gb0 = ga0, gb1 = ga0;
  if constexpr (EPI == EPI_GATED_BWD) {
    const T* abp = reinterpret_cast<const T*>(g.ab_out);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = tid + 256 * u, rl = idx >> 3, ch = idx & 7;
      const int64_t at = (int64_t)min(m0 + rl, g.M - 1) * (2 * g.N) + min(n0 + ch * 8, g.N - 8);
      const uint4 va = *reinterpret_cast<const uint4*>(abp + at), vb = *reinterpret_cast<const uint4*>(abp + at + g.N);
      if (u == 0) { ga0 = va; gb0 = vb; } else { ga1 = va; gb1 = vb; }
    }
  }
  if constexpr (NS > 0) {
    // ---- LDS-DMA ring (see above) ----
    constexpr int IPO = BM / 32;                               // wave instructions per operand per stage (8 rows each, 4 waves)
    constexpr int PER = 2 * IPO;                               // ... per wave per stage
    constexpr int STAGE = (BM + BN) * 64;                      // elements per stage: A tile [BM][64], then B tile [BN][64]
    static_assert(NS >= 2 && NS <= 4 && (NS - 1) * PER <= 63, "ring depth: the vmcnt field counts 63 loads");
    const int lrow = lane >> 3, slot = lane & 7;
    const T* ap[IPO];
    const T* bp[IPO];
#pragma unroll
    for (int j = 0; j < IPO; ++j) {
      const int row = (wave * IPO + j) * 8 + lrow;             // tile row this lane fetches a chunk of
      const int chunk = slot ^ ((row >> 1) & 7);
      ap[j] = A + (int64_t)min(m0 + row, g.M - 1) * K + chunk * 8;
      bp[j] = W + (int64_t)min(n0 + row, g.N - 1) * K + chunk * 8;
    }
    // The DMA instructions are inline asm ON PURPOSE: through __builtin_amdgcn_global_load_lds hipcc (ROCm 7.2) knows the LDS is
    // being written and puts s_waitcnt vmcnt(0) in front of the first ds_read of every k-step — the whole ring drains each step.
    // In asm the loads are invisible to its bookkeeping; their completion is counted by hand below (vmcnt is in-order, the only
    // compiler-issued loads — the residual prefetch — are older than every DMA).  M0 = wave-uniform LDS byte address of the piece.
    typedef __attribute__((address_space(3))) T* lds_ptr_t;
    const unsigned lds0 = (unsigned)(uintptr_t)(lds_ptr_t)AB;
    const unsigned wave_u = (unsigned)__builtin_amdgcn_readfirstlane(wave);
    auto glds16 = [](const T* gsrc, unsigned lds_dst) {
      unsigned keep;
      asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                   : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
    };
    auto issue = [&](int kt) {                                 // stage kt -> ring slot kt % NS
      const unsigned base = lds0 + 2u * ((unsigned)(kt % NS) * STAGE + wave_u * (IPO * 8 * 64));
#pragma unroll
      for (int j = 0; j < IPO; ++j) {
        glds16(ap[j] + (int64_t)kt * 64, base + 2u * (j * 8 * 64));
        glds16(bp[j] + (int64_t)kt * 64, base + 2u * (BM * 64 + j * 8 * 64));
      }
    };
    const int nk = K / 64;
#pragma unroll
    for (int s0 = 0; s0 < NS - 1; ++s0)
      if (s0 < nk) issue(s0);
    GEMM_STAMP(0);
    const int sw = (r >> 1) & 7;                               // the read side of the swizzle: tile row & 31 == r for every fragment
    for (int kt = 0; kt < nk; ++kt) {
      if (kt == 1) GEMM_STAMP(2);
      // stage kt has landed when at most `ahead` younger stages of this wave are still outstanding ...
      const int ahead = min(nk, kt + NS - 1) - kt - 1;
      if (ahead >= NS - 2) m2m_wait_vmcnt<(NS - 2) * PER>();
      else if (NS > 3 && ahead == 1) m2m_wait_vmcnt<PER>();
      else m2m_wait_vmcnt<0>();
      __builtin_amdgcn_s_barrier();                            // ... and when every wave has seen its own land: all of stage kt is in LDS
      asm volatile("" ::: "memory");
      if (kt + NS - 1 < nk) issue(kt + NS - 1);                // into the slot stage kt - 1 was read from (every wave is past that read)
      const T* Asg = AB + (kt % NS) * STAGE;
      const T* Bsg = Asg + BM * 64;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        Frag<T> fa[TF], fb[TF];
#pragma unroll
        for (int i = 0; i < TF; ++i) {
          fa[i] = load_frag(Asg + (wm * WT + i * 32 + r) * 64 + (((2 * s + h) ^ sw) << 3));
          fb[i] = load_frag(Bsg + (wn * WT + i * 32 + r) * 64 + (((2 * s + h) ^ sw) << 3));
        }
#pragma unroll
        for (int i = 0; i < TF; ++i)
#pragma unroll
          for (int j = 0; j < TF; ++j) mma16(acc[i][j], fa[i], fb[j]);
      }
    }
    GEMM_STAMP(3);
  } else {
  // register staging in NAMED scalars: arrays here (uint4 ra[PER_THREAD]) are demoted to scratch by
  // hipcc 7.2 across the k-loop even when every index is a compile-time constant
  static_assert(PER_THREAD == 2 || PER_THREAD == 4, "staging below is written for 2 or 4 chunks per thread");
  static_assert(BM == BN, "one chunk table serves both operand tiles");
#define M2M_CHUNK(i)                                                                         \
  const int c##i = tid + (i) * 256;                                                          \
  const T* ap##i = A + (int64_t)min(m0 + c##i / Cfg::CPR, g.M - 1) * K + (c##i % Cfg::CPR) * EPC; \
  const T* bp##i = W + (int64_t)min(n0 + c##i / Cfg::CPR, g.N - 1) * K + (c##i % Cfg::CPR) * EPC; \
  const int so##i = (c##i / Cfg::CPR) * Cfg::PITCH + (c##i % Cfg::CPR) * EPC;                 \
  uint4 ra##i, rb##i;
  M2M_CHUNK(0) M2M_CHUNK(1) M2M_CHUNK(2) M2M_CHUNK(3)
#undef M2M_CHUNK
#define M2M_LD(i, k0) ra##i = *reinterpret_cast<const uint4*>(ap##i + (k0)); rb##i = *reinterpret_cast<const uint4*>(bp##i + (k0));
#define M2M_ST(i) *reinterpret_cast<uint4*>(As + so##i) = ra##i; *reinterpret_cast<uint4*>(Bs + so##i) = rb##i;
#define M2M_GLOAD(k0) { M2M_LD(0, k0) M2M_LD(1, k0) if constexpr (PER_THREAD == 4) { M2M_LD(2, k0) M2M_LD(3, k0) } }
#define M2M_SSTORE() { M2M_ST(0) M2M_ST(1) if constexpr (PER_THREAD == 4) { M2M_ST(2) M2M_ST(3) } }
  ra2 = rb2 = ra3 = rb3 = make_uint4(0, 0, 0, 0);

  const int nk = K / BK;
  M2M_GLOAD(0)
  GEMM_STAMP(0);
  GEMM_WAITLOADS();
  GEMM_STAMP(1);
  for (int kt = 0; kt < nk; ++kt) {
    if (kt == 1) GEMM_STAMP(2);
    __syncthreads();
    M2M_SSTORE()
    __syncthreads();
    if (kt + 1 < nk) { M2M_GLOAD((kt + 1) * BK) }
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      Frag<T> fa[TF], fb[TF];
#pragma unroll
      for (int i = 0; i < TF; ++i) {
        fa[i] = load_frag(As + (wm * WT + i * 32 + r) * Cfg::PITCH + s * 16 + 8 * h);
        fb[i] = load_frag(Bs + (wn * WT + i * 32 + r) * Cfg::PITCH + s * 16 + 8 * h);
      }
#pragma unroll
      for (int i = 0; i < TF; ++i)
#pragma unroll
        for (int j = 0; j < TF; ++j) mma16(acc[i][j], fa[i], fb[j]);
    }
  }

  GEMM_STAMP(3);
  }
#undef M2M_GLOAD
#undef M2M_SSTORE
#undef M2M_LD
#undef M2M_ST
  // ---- epilogue ----
  if constexpr (EPI == EPI_HEADS) {
    // Head-major scatter through LDS, so that every store instruction writes whole 128-byte lines: a (row, head)
    // pair of q / k is exactly one line, and the transposed V is contiguous along the rows.  Written straight
    // from the accumulators the same data goes out as 64-byte halves and 2-byte scatters, and the write-allocate
    // fetches of those partial lines were 3/4 of the kernel's HBM reads (PMC: 157 MB per launch for 21 MB of
    // activations).  A 128-column tile never straddles q / k / v (inner % 128 == 0).
    constexpr int CP = BN + 8;                                  // LDS pitch of the staged tile (elements)
    static_assert(BM * CP <= (BM + BN) * Cfg::PITCH || sizeof(T) == 4, "staged tile must fit the operand buffers");
    const int which = n0 / g.inner;
    const bool transposed = (which == g.vt_which);
    __syncthreads();                                            // every wave is done with As / Bs
    if constexpr (sizeof(T) == 2) {
      T* Cs = AB;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int rl = wm * 64 + mi * 32 + acc_row(e, lane), cl = wn * 64 + ni * 32 + r;
            Cs[transposed ? cl * CP + rl : rl * CP + cl] = from_f32<T>(acc[mi][ni][e]);
          }
      __syncthreads();
      constexpr int EPC8 = 8;                                   // bf16 elements per 16-byte store
      for (int idx = tid; idx < BM * (BN / EPC8); idx += 256) {
        if (!transposed) {
          const int rl = idx / (BN / EPC8), ch = idx % (BN / EPC8);
          const int row = m0 + rl, col = n0 + ch * EPC8;
          if (row < g.M && col < g.N) {
            const int rem = col - which * g.inner, hh = rem / DK, dd = rem - hh * DK;
            const int b = row / g.S, sq = row - b * g.S;
            *reinterpret_cast<uint4*>(reinterpret_cast<T*>(g.out) + ((((int64_t)which * g.Bsz + b) * g.H + hh) * g.S + sq) * DK + dd) =
                *reinterpret_cast<const uint4*>(Cs + rl * CP + ch * EPC8);
          }
        } else {
          const int cl = idx / (BM / EPC8), rc = idx % (BM / EPC8);
          const int col = n0 + cl, row0 = m0 + rc * EPC8;
          if (col < g.N && row0 < g.M) {
            const int rem = col - which * g.inner, hh = rem / DK, dd = rem - hh * DK;
            const int b = row0 / g.S, s0 = row0 - b * g.S;
            T* dst = reinterpret_cast<T*>(g.vt_out) + (((int64_t)b * g.H + hh) * DK + dd) * g.Sp;
            const T* src = Cs + cl * CP + rc * EPC8;
            if (s0 + EPC8 <= g.S && row0 + EPC8 <= g.M && (s0 & 7) == 0) {
              *reinterpret_cast<uint4*>(dst + s0) = *reinterpret_cast<const uint4*>(src);
            } else {                                            // chunk straddles a clip boundary / is misaligned
              for (int j = 0; j < EPC8; ++j) {
                const int row = row0 + j;
                if (row < g.M) {
                  const int bj = row / g.S, sj = row - bj * g.S;
                  reinterpret_cast<T*>(g.vt_out)[(((int64_t)bj * g.H + hh) * DK + dd) * g.Sp + sj] = src[j];
                }
              }
            }
          }
        }
      }
      return;
    }
  }
  if constexpr (EPI == EPI_GATED_BWD) {
    // Training backward of the gated feed-forward: the tile of dmid goes to LDS in bf16 (the rounding the stored dmid had), then every
    // thread turns two 8-column chunks into da | db — 16-byte reads of a | b (requested before the k loop), 16-byte stores of both
    // halves of dab, the dropout mask of the forward hashed once per four columns.  What gated_bwd_kernel did in a launch of its own
    // (12 per step, 12 us each, 38 MB read + 19 MB written per launch) minus the dmid round trip through memory.
    constexpr int CP = 64 + 8;
    __syncthreads();
    T* Cs = AB;
#pragma unroll
    for (int e = 0; e < 16; ++e) Cs[(wm * 32 + acc_row(e, lane)) * CP + wn * 32 + r] = from_f32<T>(acc[0][0][e]);
    __syncthreads();
    const uint64_t dkey = g.drop_thresh ? splitmix64(*g.drop_step + g.drop_key) : 0ull;
    T* dab = reinterpret_cast<T*>(g.out);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = tid + 256 * u, rl = idx >> 3, ch = idx & 7;
      const int row = m0 + rl, col = n0 + ch * 8;
      if (row >= g.M || col >= g.N) continue;
      const uint4 vd = *reinterpret_cast<const uint4*>(Cs + rl * CP + ch * 8);
      const uint4 va = u == 0 ? ga0 : ga1, vb = u == 0 ? gb0 : gb1;
      const uint32_t wd[4] = {vd.x, vd.y, vd.z, vd.w}, wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
      uint32_t oa[4], ob[4];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const uint32_t kb = g.drop_thresh ? drop_keep4(dkey, (int64_t)row * g.N + col + 4 * q, g.drop_thresh) : 0xFu;
#pragma unroll
        for (int p2 = 0; p2 < 2; ++p2) {
          const int w = 2 * q + p2;
          float da[2], db[2];
#pragma unroll
          for (int hl = 0; hl < 2; ++hl) {
            const float dm0 = __uint_as_float(hl ? (wd[w] & 0xFFFF0000u) : (wd[w] << 16));
            const float av = __uint_as_float(hl ? (wa[w] & 0xFFFF0000u) : (wa[w] << 16)), bv = __uint_as_float(hl ? (wb[w] & 0xFFFF0000u) : (wb[w] << 16));
            float dm = dm0;
            if (g.drop_thresh) dm = ((kb >> (2 * p2 + hl)) & 1u) ? dm0 * g.drop_scale : 0.f;
            float gg, dg;
            gelu_new_both_t<T>(av, &gg, &dg);
            da[hl] = dm * bv * dg;
            db[hl] = dm * gg;
          }
          oa[w] = pack2_bf16(da[0], da[1]);
          ob[w] = pack2_bf16(db[0], db[1]);
        }
      }
      *reinterpret_cast<uint4*>(dab + (int64_t)row * g.ldo + col) = make_uint4(oa[0], oa[1], oa[2], oa[3]);
      *reinterpret_cast<uint4*>(dab + (int64_t)row * g.ldo + g.N + col) = make_uint4(ob[0], ob[1], ob[2], ob[3]);
    }
    return;
  }
  if constexpr (EPI == EPI_GATED_TRAIN) {
    // Training forward of the gated feed-forward: the gate pair a | b (needed again by the backward pass) and
    // mid = dropout(gelu_new(a) * b), both from the bf16-ROUNDED a and b — exactly what the separate gated_fwd_kernel computed
    // from the stored pair — in two LDS-staged rounds so that memory sees whole 128-byte lines.
    constexpr int GP = BN / 2 + 8, AP = BN + 8;
    static_assert(BM * AP <= LDS_ELEMS, "the staged gate pair must fit the operand buffers");
    const int half = g.N / 2;
    const float dscale = g.drop_thresh ? g.drop_scale : 1.0f;
    __syncthreads();
    T* Cs = AB;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int rl = wm * 64 + mi * 32 + acc_row(e, lane);
        const float av = to_f32(from_f32<T>(acc[mi][0][e])), bv = to_f32(from_f32<T>(acc[mi][1][e]));
        Cs[rl * GP + wn * 32 + r] = from_f32<T>(gelu_new_t<T>(av) * bv * dscale);      // (one rounding, after the dropout scale)
      }
    __syncthreads();
    {
      const uint64_t dkey = g.drop_thresh ? splitmix64(*g.drop_step + g.drop_key) : 0ull;
      for (int idx = tid; idx < BM * (BN / 16); idx += 256) {
        const int rl = idx / (BN / 16), ch = idx % (BN / 16);
        const int row = m0 + rl, oc = n0 / 2 + ch * 8;
        if (row < g.M && oc < half) {
          uint4 v = *reinterpret_cast<const uint4*>(Cs + rl * GP + ch * 8);
          if (g.drop_thresh) {
            uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 2; ++q) {
              const uint32_t kb = drop_keep4(dkey, (int64_t)row * half + oc + 4 * q, g.drop_thresh);
#pragma unroll
              for (int p2 = 0; p2 < 2; ++p2)                  // dropped elements to zero (the scale is in the staged value already)
                w[2 * q + p2] &= (((kb >> (2 * p2)) & 1u) ? 0x0000FFFFu : 0u) | (((kb >> (2 * p2 + 1)) & 1u) ? 0xFFFF0000u : 0u);
            }
            v = make_uint4(w[0], w[1], w[2], w[3]);
          }
          *reinterpret_cast<uint4*>(reinterpret_cast<T*>(g.out) + (int64_t)row * g.ldo + oc) = v;
        }
      }
    }
    __syncthreads();
    // the pair: staged as [row][a of chunk wn=0 | a of chunk wn=1 | b of chunk wn=0 | b of chunk wn=1] — two 128-byte lines per row
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int rl = wm * 64 + mi * 32 + acc_row(e, lane);
        Cs[rl * AP + wn * 32 + r] = from_f32<T>(acc[mi][0][e]);
        Cs[rl * AP + 64 + wn * 32 + r] = from_f32<T>(acc[mi][1][e]);
      }
    __syncthreads();
    for (int idx = tid; idx < BM * (BN / 8); idx += 256) {
      const int rl = idx / (BN / 8), ch = idx % (BN / 8);       // ch 0..7: a, 8..15: b
      const int row = m0 + rl, oc = n0 / 2 + (ch & 7) * 8;
      if (row < g.M && oc < half)
        *reinterpret_cast<uint4*>(reinterpret_cast<T*>(g.ab_out) + (int64_t)row * g.N + (ch >= 8 ? half : 0) + oc) =
            *reinterpret_cast<const uint4*>(Cs + rl * AP + ch * 8);
    }
    return;
  }
  if constexpr ((EPI == EPI_GATED || EPI == EPI_GATED16) && sizeof(T) == 2) {
    // gated up projection, bf16: the 128-column tile yields 64 outputs per row = one 128-byte line; staged in
    // LDS so that 8 lanes write a whole line with 16-byte stores (straight from the accumulators it is 64-byte
    // halves of 2-byte elements)
    constexpr int GP = BN / 2 + 8;
    __syncthreads();
    T* Cs = AB;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int rl = wm * 64 + mi * 32 + acc_row(e, lane);
        if constexpr (EPI == EPI_GATED) {       // the wave's 64 columns are [32 of wi_0 | the matching 32 of wi_1]
          Cs[rl * GP + wn * 32 + r] = from_f32<T>(gelu_new_t<T>(acc[mi][0][e]) * acc[mi][1][e]);
        } else {                                // 16-column groups: 8 of wi_0 then the matching 8 of wi_1
#pragma unroll
          for (int ni = 0; ni < 2; ++ni) {
            const float v = acc[mi][ni][e], partner = lane_xor<8>(v);
            const int cl = wn * 64 + ni * 32 + r;
            if ((cl & 8) == 0) Cs[rl * GP + (cl >> 4) * 8 + (cl & 7)] = from_f32<T>(gelu_new_t<T>(v) * partner);
          }
        }
      }
    __syncthreads();
    for (int idx = tid; idx < BM * (BN / 16); idx += 256) {
      const int rl = idx / (BN / 16), ch = idx % (BN / 16);
      const int row = m0 + rl, oc = n0 / 2 + ch * 8;
      if (row < g.M && 2 * oc < g.N)
        *reinterpret_cast<uint4*>(reinterpret_cast<T*>(g.out) + (int64_t)row * g.ldo + oc) =
            *reinterpret_cast<const uint4*>(Cs + rl * GP + ch * 8);
    }
    return;
  }
  uint64_t dkey = 0;
  if constexpr (EPI == EPI_RESID) { if (g.drop_thresh) dkey = splitmix64(*g.drop_step + g.drop_key); }
#pragma unroll
  for (int mi = 0; mi < TF; ++mi) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = m0 + wm * WT + mi * 32 + acc_row(e, lane);
      if (row >= g.M) continue;
      if constexpr (EPI == EPI_GATED) {
        // the wave's 64 columns are [32 of wi_0 | the matching 32 of wi_1]
        const int col = (n0 + wn * 64) / 2 + r;
        if (n0 + wn * 64 < g.N) {
          const float v = gelu_new_t<T>(acc[mi][0][e]) * acc[mi][TF - 1][e];
          reinterpret_cast<T*>(g.out)[(int64_t)row * g.ldo + col] = from_f32<T>(v);
        }
      } else {
#pragma unroll
        for (int ni = 0; ni < TF; ++ni) {
          const int col = n0 + wn * WT + ni * 32 + r;
          if constexpr (EPI != EPI_GATED16) {
            if (col >= g.N) continue;       // (GATED16: N is a multiple of 16 and every lane takes part in the exchange)
          }
          const float v = acc[mi][ni][e];
          if constexpr (EPI == EPI_STORE) {
            reinterpret_cast<T*>(g.out)[(int64_t)row * g.ldo + col] = from_f32<T>(v);
          } else if constexpr (EPI == EPI_STORE_F32) {
            reinterpret_cast<float*>(g.out)[(int64_t)row * g.ldo + col] = v;
          } else if constexpr (EPI == EPI_GATED16) {
            // decoder packing of the gated up projection: 16-row groups, 8 rows of wi_0 then the matching 8 of
            // wi_1 (repack.hip), so the gate partner of column c sits 8 lanes away
            const float partner = lane_xor<8>(v);
            if ((col & 8) == 0 && col < g.N) {
              const int oc = (col >> 4) * 8 + (col & 7);
              reinterpret_cast<T*>(g.out)[(int64_t)row * g.ldo + oc] = from_f32<T>(gelu_new_t<T>(v) * partner);
            }
          } else if constexpr (EPI == EPI_RESID) {
            const int64_t at = (int64_t)row * g.ldo + col;
            float* p = reinterpret_cast<float*>(g.out) + at;
            float u = v;
            if (g.drop_thresh) u = drop_keep(dkey, at, g.drop_thresh) ? v * g.drop_scale : 0.f;   // training only
            if constexpr (TF == 1) *p = rpre[e] + u;
            else *p = (g.resid ? g.resid[at] : *p) + u;
          } else {  // EPI_HEADS (fp32)
            const int which = col / g.inner, rem = col - which * g.inner;
            const int hh = rem / DK, dd = rem - hh * DK;
            const int b = row / g.S, s = row - b * g.S;
            if (which == g.vt_which)
              reinterpret_cast<T*>(g.vt_out)[(((int64_t)b * g.H + hh) * DK + dd) * g.Sp + s] = from_f32<T>(v);
            else
              reinterpret_cast<T*>(g.out)[((((int64_t)which * g.Bsz + b) * g.H + hh) * g.S + s) * DK + dd] = from_f32<T>(v);
          }
        }
      }
    }
  }
  GEMM_WAITLOADS();
  GEMM_STAMP(4);
}

// Tile choice: the 128x128 kernel unless its grid is smaller than `M2M_GEMM_SMALL_BELOW` tiles (default 512 = two rounds
// of the chip) and the epilogue is one of the plain ones; then 64x64 tiles (see the note above gemm_kernel).
static int gemm_small_below() { return enc_switches_now().gemm_small_below; }

// Which main loop (bf16).  Measured per launch shape on MI355X (tools/r3_gemm_bygrid.sh, 16-clip training step, rocprofv3, us,
// register-staged -> LDS-DMA ring of 4): the long reductions with few workgroups win — N = 384 outputs, 384-432 small tiles,
// K = 512 ... 2304: residual products 13.9 -> 12.3 / 12.5 -> 11.3, dX into fp32 18.3 -> 15.5 / 15.3 -> 13.1 — and the short ones
// with many workgroups lose — K = 384, 576-1728 small tiles: 7.6 -> 8.6, 11.8 -> 12.6, 12.4 -> 13.7, 14.5 -> 16.1 (64 KiB of
// LDS per workgroup leaves two per CU where the register-staged loop runs four; six k-steps never fill a ring) — as do the
// 128x128 tiles (18.1 -> 24.8: 96 KiB, one workgroup per CU).  So: the ring for small tiles with K >= M2M_GEMM_DMA_MINK (512),
// the register-staged loop otherwise.  M2M_GEMM_DMA=0 / =all force one or the other; M2M_GEMM_DMA_NS1 / _NS2 pick the depths
// (a depth that has no kernel becomes the deep ring of its tile).  All latched (EncSwitches).
static int gemm_dma_ns(int tf, int K, int tiles) {
  const EncSwitches& sw = enc_switches_now();
  int ns = 0;
  if (sw.gemm_dma == 2) ns = tf == 1 ? sw.gemm_dma_ns1 : sw.gemm_dma_ns2;
  else if (sw.gemm_dma == 1 && tf == 1 && K >= sw.gemm_dma_mink && tiles <= sw.gemm_dma_maxt) ns = sw.gemm_dma_ns1;
  return gemm_ring_exists(true, tf, ns) ? ns : gemm_ring_deep(tf);
}

// one launch: the kernel of (T, EPI, TF) with the ring depth `ns` (a variant that does not exist is not instantiated: the callers
// have refused it)
template <typename T, int EPI, int TF, int NS>
static void gemm_go(dim3 grid, const GemmArgs& a, hipStream_t st) {
  if constexpr (gemm_variant_exists(sizeof(T) == 2, EPI, TF) && gemm_ring_exists(sizeof(T) == 2, TF, NS))
    hipLaunchKernelGGL((gemm_kernel<T, EPI, TF, NS>), grid, dim3(256), 0, st, a);
}
template <typename T, int EPI, int TF>
static void gemm_go_ns(int ns, dim3 grid, const GemmArgs& a, hipStream_t st) {
  if (ns == gemm_ring_deep(TF)) gemm_go<T, EPI, TF, gemm_ring_deep(TF)>(grid, a, st);
  else if (ns == gemm_ring_shallow(TF)) gemm_go<T, EPI, TF, gemm_ring_shallow(TF)>(grid, a, st);
  else gemm_go<T, EPI, TF, 0>(grid, a, st);
}
template <typename T, int TF, int... EPIS>
static void gemm_go_epi(int epi, int ns, dim3 grid, const GemmArgs& a, hipStream_t st, std::integer_sequence<int, EPIS...>) {
  ((epi == EPIS ? gemm_go_ns<T, EPIS, TF>(ns, grid, a, st) : (void)0), ...);
}

template <typename T, int TF>
static int launch_gemm_tt(int epi, const GemmArgs& a_in, hipStream_t st) {
  constexpr int BM = 64 * TF, BN = 64 * TF;
  constexpr bool bf16 = sizeof(T) == 2;
  if (!gemm_variant_exists(bf16, epi, TF)) {
    if (epi == EPI_GATED_BWD) set_error("launch_gemm: the gate-gradient epilogue is a bf16 small-tile path");
    else if (TF == 1) set_error("launch_gemm: epilogue %d has no small-tile variant", epi);
    else if (epi == EPI_GATED_TRAIN) set_error("launch_gemm: the training gate epilogue is a bf16 path");
    else set_error("launch_gemm: bad epilogue %d", epi);
    return M2M_ERR_INVALID;
  }
  GemmArgs a = a_in;
  const int ntn = ceil_div(a.N, BN);
  const int ng_max = (int)((2 << 20) / ((size_t)BN * a.K * sizeof(T)));          // column tiles whose weight rows fit 2 MB
  const int ngroups = ceil_div(ntn, ng_max < 1 ? 1 : ng_max);
  a.ng = ceil_div(ntn, ngroups);
  dim3 grid((unsigned)(8 * ngroups * ceil_div(ceil_div(a.M, BM), 8) * a.ng));
  const int ns = bf16 ? gemm_dma_ns(TF, a.K, ceil_div(a.M, BM) * ntn) : 0;
  gemm_go_epi<T, TF>(epi, ns, grid, a, st, std::make_integer_sequence<int, EPI_GATED_BWD + 1>());
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

template <typename T>
static int launch_gemm_t(int epi, const GemmArgs& a, hipStream_t st) {
  const int tiles128 = ceil_div(a.M, 128) * ceil_div(a.N, 128);
  if (epi == EPI_GATED_BWD) return launch_gemm_tt<T, 1>(epi, a, st);           // (always the small tile: launch_gemm checked the shape)
  if (gemm_epi_plain(epi) && tiles128 < gemm_small_below() && a.K % TileCfgT<T, 1>::BK == 0) return launch_gemm_tt<T, 1>(epi, a, st);      // (K % 128: the register-staged small tile's step)
  return launch_gemm_tt<T, 2>(epi, a, st);
}

bool gemm_takes_gated_train(int precision, int M, int N, int K) {     // bf16, and a grid the 128x128 tile is chosen for anyway
  return precision == M2M_PREC_BF16 && N % 128 == 0 && K % 64 == 0 && ceil_div(M, 128) * ceil_div(N, 128) >= gemm_small_below();
}

bool gemm_takes_gated_bwd(int precision, int M, int N, int K) { return precision == M2M_PREC_BF16 && N % 64 == 0 && K % 128 == 0 && M >= 1; }


// ===================================================== row-panel residual product ====
// x[M][N] += A[M][K] . W[N][K]^T with N = d_model (the attention output projection and the feed-forward down projection:
// hf modeling_t5.py:363-369, :128-141 + the residual adds of :403 / :135).  The 128 x 128 tiling runs these as three column tiles per
// row block, each streaming the same A tile again (0.33 of HBM, 12 % matrix-core busy: profiles/r5_a).  N = 384 is one row of the
// residual stream: here a workgroup of 8 waves owns 128 COMPLETE rows — A streams through LDS once, in [128 x 64] chunks beside the
// [N x 64] weight chunks (W is 0.4-0.9 MB and comes from L2), two chunks in flight in registers and two stages in LDS (one barrier
// per chunk); 2 x 4 waves of 64 rows x N/4 columns each, so every A fragment feeds N/128 MFMAs and every weight fragment two
// (0.83 KB of LDS reads per MFMA at N = 384); the fp32 rows are read, added to and written back straight from the accumulators.
// Same k order per output element and the same operand roles as gemm_kernel<bf16, EPI_RESID>: bit-identical (tests).
// Shader-clock stamps of one workgroup (-DM2M_RP_STAMP, tools/rp_stamps.py; down projection, 18 chunks): prologue 9 %, 18 x ~2 800
// ticks per chunk 65 %, epilogue 27 %.  Same-box A/Bs (tools/ab_resid.sh) of what the stamps suggested: a 16-wave form (4 x 4 waves
// of 32 rows: four waves per SIMD against the fragment reads' LDS round trips) spends the SAME 2 600 ticks per chunk (kernel 40.2
// against 37.7 us) — a chunk waits neither for LDS nor for the matrix core but for its 64 KB of operands: ~25 GB/s per CU, the
// ingest rate of every one-workgroup-per-CU stream on this chip (DESIGN_HISTORY 4.3-4.5); the weights as the MFMA's A operand, so
// that a lane adds into four consecutive columns with 16-byte accesses (32 rows x 32 bytes per instruction instead of 2 rows x
// 128): 40.5 against 37.7 us — the scalar form's whole-line accesses win.
// (Measured and dropped: chunk-tiled copies of the weights — every [128 x 64] chunk one contiguous 16 KB block, 1 KB runs per wave
// load instead of eight 128-byte pieces at a 0.8-2.3 KB stride — for this kernel and norm_gemm_kernel: no change (QKV 54.0, gated 72.4,
// O-proj 28.3, down-proj 51.1 us): the weight stream is served by L2 hits at 14 % of that cache's peak either way — TCC hit / miss
// counters in tools/pmc_enc_l2.sh — so neither its layout nor L2 channel camping is what these kernels wait for.)
constexpr int RP_BM = 128, RP_BK = 64, RP_THREADS = 512, RP_P = RP_BK + 8;
#ifdef M2M_RP_STAMP       // diagnostic builds only (tools/rp_stamps.py): shader-clock stamps of one workgroup at every chunk boundary
__device__ unsigned long long g_rp_stamp[64];
#define RP_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x == 77 && (i) < 64) g_rp_stamp[i] = clock64(); } while (0)
#else
#define RP_STAMP(i) do {} while (0)
#endif

template <int NB>      // NB = N / 128: 32-column MFMA blocks per wave (N = 128 / 256 / 384)
__global__ __launch_bounds__(RP_THREADS) void resid_panel_kernel(GemmArgs g) {
  using T = bf16_t;
  constexpr int N = 128 * NB, STAGE = (RP_BM + N) * RP_P;
  extern __shared__ __align__(16) unsigned char rp_smem[];
  T* const lds = reinterpret_cast<T*>(rp_smem);                 // [2 stages][A 128 x 72 | W N x 72]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 2, wn = wave & 3;                       // 2 x 4 waves
  const int r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * RP_BM, K = g.K, nk = K / RP_BK;
  const T* A = reinterpret_cast<const T*>(g.A);
  const T* W = reinterpret_cast<const T*>(g.W);
  // staging pieces of this thread: row tid >> 3 (+ 64 j), 16-byte piece tid & 7
  const int pr = tid >> 3, pc = (tid & 7) * 8;
  const T* const ap0 = A + (int64_t)min(m0 + pr, g.M - 1) * K + pc;
  const T* const ap1 = A + (int64_t)min(m0 + pr + 64, g.M - 1) * K + pc;
  const T* const wp = W + (int64_t)pr * K + pc;                  // rows pr + 64 j, j < 2 NB (N is a multiple of 128: no clamp)
  // two register sets (chunk c lives in set c & 1 and goes to stage c & 1); named scalars: arrays across the loop go to scratch
  uint4 sa0, sa1, sw0, sw1, sw2, sw3, sw4, sw5, ta0, ta1, tw0, tw1, tw2, tw3, tw4, tw5;
  sw2 = sw3 = sw4 = sw5 = tw2 = tw3 = tw4 = tw5 = make_uint4(0, 0, 0, 0);
#define RP_LOAD(p_, c_)                                                                                 \
  {                                                                                                     \
    const int k0_ = min((c_), nk - 1) * RP_BK;      /* past the end: the last chunk again, never used */ \
    p_##a0 = *reinterpret_cast<const uint4*>(ap0 + k0_); p_##a1 = *reinterpret_cast<const uint4*>(ap1 + k0_); \
    p_##w0 = *reinterpret_cast<const uint4*>(wp + k0_); p_##w1 = *reinterpret_cast<const uint4*>(wp + (int64_t)64 * K + k0_); \
    if constexpr (NB >= 2) { p_##w2 = *reinterpret_cast<const uint4*>(wp + (int64_t)128 * K + k0_); p_##w3 = *reinterpret_cast<const uint4*>(wp + (int64_t)192 * K + k0_); } \
    if constexpr (NB >= 3) { p_##w4 = *reinterpret_cast<const uint4*>(wp + (int64_t)256 * K + k0_); p_##w5 = *reinterpret_cast<const uint4*>(wp + (int64_t)320 * K + k0_); } \
  }
#define RP_STORE(p_, stage_)                                                                            \
  {                                                                                                     \
    T* const sA_ = lds + (stage_) * STAGE; T* const sW_ = sA_ + RP_BM * RP_P;                           \
    *reinterpret_cast<uint4*>(sA_ + pr * RP_P + pc) = p_##a0; *reinterpret_cast<uint4*>(sA_ + (pr + 64) * RP_P + pc) = p_##a1; \
    *reinterpret_cast<uint4*>(sW_ + pr * RP_P + pc) = p_##w0; *reinterpret_cast<uint4*>(sW_ + (pr + 64) * RP_P + pc) = p_##w1; \
    if constexpr (NB >= 2) { *reinterpret_cast<uint4*>(sW_ + (pr + 128) * RP_P + pc) = p_##w2; *reinterpret_cast<uint4*>(sW_ + (pr + 192) * RP_P + pc) = p_##w3; } \
    if constexpr (NB >= 3) { *reinterpret_cast<uint4*>(sW_ + (pr + 256) * RP_P + pc) = p_##w4; *reinterpret_cast<uint4*>(sW_ + (pr + 320) * RP_P + pc) = p_##w5; } \
  }
  RP_STAMP(0);
  RP_LOAD(s, 0)
  RP_LOAD(t, 1)
  f32x16 acc[2][NB];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[i][j] = zero_acc();
  RP_STORE(s, 0)
  RP_LOAD(s, 2)
  __syncthreads();
  RP_STAMP(1);
  // body of chunk c (stage c & 1): multiply, then the OTHER register set (chunk c + 1) goes to the other stage and takes chunk c + 3
#define RP_BODY(c_, st_, nxt_)                                                                          \
  {                                                                                                     \
    const T* const fa_ = lds + (st_) * STAGE + (wm * 64 + r) * RP_P + 8 * h;                             \
    const T* const fb_ = lds + (st_) * STAGE + RP_BM * RP_P + (wn * 32 * NB + r) * RP_P + 8 * h;         \
    _Pragma("unroll") for (int s4 = 0; s4 < RP_BK / 16; ++s4) {                                          \
      Frag<T> a0_ = load_frag(fa_ + s4 * 16), a1_ = load_frag(fa_ + 32 * RP_P + s4 * 16);               \
      _Pragma("unroll") for (int j = 0; j < NB; ++j) {                                                   \
        const Frag<T> b_ = load_frag(fb_ + j * 32 * RP_P + s4 * 16);                                     \
        mma16(acc[0][j], a0_, b_);                                                                       \
        mma16(acc[1][j], a1_, b_);                                                                       \
      }                                                                                                 \
    }                                                                                                   \
    RP_STORE(nxt_, (st_) ^ 1)                                                                            \
    RP_LOAD(nxt_, (c_) + 3)                                                                              \
    __syncthreads();                                                                                    \
    RP_STAMP(2 + (c_));                                                                                 \
  }
  int c = 0;
  for (; c + 1 < nk; c += 2) {
    RP_BODY(c, 0, t)
    RP_BODY(c + 1, 1, s)
  }
  if (c < nk) RP_BODY(c, 0, t)
#undef RP_BODY
#undef RP_STORE
#undef RP_LOAD
  // ---- x += acc: element e of lane (r, h), blocks (i, j): row wm * 64 + i * 32 + (e & 3) + 8 (e >> 2) + 4 h, column wn * 32 NB + j * 32 + r ----
  // The reads go out a row block at a time (NB x 16 loads in flight, clamped rows, no branch between them: one load -> wait ->
  // store per element behind `if (row < M)` serialised 96 memory round trips per lane — 35 of the first version's 45 us).
  float* const xo = reinterpret_cast<float*>(g.out);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    float xv[NB][16];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = min(m0 + wm * 64 + i * 32 + acc_row(e, lane), g.M - 1);
        xv[j][e] = xo[(int64_t)row * g.ldo + wn * 32 * NB + j * 32 + r];
      }
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * 64 + i * 32 + acc_row(e, lane);
        if (row < g.M) xo[(int64_t)row * g.ldo + wn * 32 * NB + j * 32 + r] = xv[j][e] + acc[i][j][e];
      }
    RP_STAMP(40 + i);
  }
}

// bf16, plain in-place residual add (no separate source, no dropout: the inference paths), N = 128 / 256 / 384, K a multiple of 64, and
// about a chip's worth of row blocks (one workgroup per 128 rows and CU).  M2M_RESID_PANEL: "0" never, "force" whatever the size.
static bool resid_panel_takes(int precision, int epi, const GemmArgs& a) {
  if (precision != M2M_PREC_BF16 || epi != EPI_RESID || a.resid || a.drop_thresh) return false;
  if (!(a.N == 128 || a.N == 256 || a.N == 384) || a.K % 64 != 0 || a.K < 128 || a.ldo != a.N) return false;
  const EncSwitches& sw = enc_switches_now();
  if (sw.resid_panel == 1) return false;
  if (sw.resid_panel == 2) return true;
  return ceil_div(a.M, RP_BM) >= sw.min_blocks;
}

static int launch_resid_panel(const GemmArgs& a, hipStream_t st) {
  const int NB = a.N / 128;
  const size_t smem = (size_t)2 * (RP_BM + a.N) * RP_P * 2;
  dim3 grid((unsigned)ceil_div(a.M, RP_BM));
#define RP_GO(NB_)                                                                              \
  do {                                                                                          \
    M2M_OPT_IN_LDS((resid_panel_kernel<NB_>), 160 * 1024);                                      \
    hipLaunchKernelGGL((resid_panel_kernel<NB_>), grid, dim3(RP_THREADS), smem, st, a);         \
  } while (0)
  if (NB == 3) RP_GO(3); else if (NB == 2) RP_GO(2); else RP_GO(1);
#undef RP_GO
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

int launch_gemm(int precision, int epi, const GemmArgs& a, hipStream_t st) {
  if (epi == EPI_GATED_BWD) M2M_REQUIRE(gemm_takes_gated_bwd(precision, a.M, a.N, a.K) && a.ab_out && a.ldo == 2 * a.N, "gemm: shape / arguments outside the gate-gradient epilogue");
  if (epi == EPI_GATED_TRAIN) M2M_REQUIRE(gemm_takes_gated_train(precision, a.M, a.N, a.K) && a.ab_out && a.ldo == a.N / 2, "gemm: shape / arguments outside the training gate epilogue");
  M2M_REQUIRE(a.K % 64 == 0, "gemm: K=%d must be a multiple of 64", a.K);
  M2M_REQUIRE(a.M >= 1 && a.N >= 1, "gemm: empty problem");
  if (epi == EPI_GATED) M2M_REQUIRE(a.N % 64 == 0, "gemm: gated epilogue needs N %% 64 == 0 (d_ff %% 32 == 0)");
  if (epi == EPI_GATED16) M2M_REQUIRE(a.N % 16 == 0, "gemm: 16-row gated epilogue needs N %% 16 == 0");
  if (resid_panel_takes(precision, epi, a)) return launch_resid_panel(a, st);
  return precision == M2M_PREC_BF16 ? launch_gemm_t<bf16_t>(epi, a, st) : launch_gemm_t<float>(epi, a, st);
}

// ================================================= fused RMSNorm + GEMM ====
// out = epilogue(RMSNorm(x) . W^T) for the products whose A operand is the normalised d_model-wide residual row (QKV, gated
// up-projection, cross-q, cross-K/V, lm_head of the batched pass): SURVEY K4, hf: modeling_t5.py:59-72 in front of :281-369 / :95-141.
//
// The two-kernel path (rmsnorm_kernel -> h in memory -> gemm_kernel) tiles the product 128 x 128: with K = 384 a tile lives for six
// k-steps, so its load -> LDS prologue and its staged epilogue are a large part of it, every one of the 12-48 column tiles of a row
// block stages the SAME activation tile again, and h makes a round trip through memory.  K = d_model is small enough for a whole
// normalised row panel to stay ON CHIP for every column tile: here a workgroup of 8 waves
//   1. reads its 128 rows of x ONCE (fp32), normalises them with exactly rmsnorm_kernel's arithmetic (a wave per row, the same
//      lane -> column map, the same reduction order, the same rounding point) into a bf16 panel in LDS (100 KB at K = 384);
//   2. every wave takes ITS 32 rows of the panel into registers as MFMA fragments (24 fragments = 96 VGPRs at K = 384) — the
//      activations are never read from LDS again — and the panel's bytes become a three-stage ring for the weight chunks;
//   3. sweeps ALL column tiles: [128 x 64] weight chunks stream L2 -> registers (three chunks in flight per thread, ACROSS tile
//      boundaries: one prologue per workgroup, not per tile) -> ring; a step multiplies chunk t while the fragments of chunk t + 1 are
//      being read and chunk t + 2 is being stored: one barrier per step, LDS reads overlap the matrix core;
//   4. stages each 128 x 128 result through its own LDS buffer with 8-byte writes — the MFMA operand roles are chosen per tile so
//      that the four values a lane holds of one accumulator column run along the staged row (weights as the A operand for row-major
//      outputs, activations as the A operand for the transposed V tile) — and stores whole 128-byte lines while the next tile runs.
// Per output element the k order is gemm_kernel's and the fragments hold the same bf16 values: results are BIT-IDENTICAL to the
// two-kernel path (tests/test_t5_gpu.py::test_norm_gemm_*, M2M_NORM_GEMM=0 is the other leg).  L2 -> LDS traffic per 128 rows: one
// pass over W (the 128 x 128 tiling: one pass over W plus one over the A panel per column tile); the 13 norm launches of an encoder
// pass are gone.
#ifndef M2M_NG_SKIP          // diagnostic builds only (timing with a part removed; results are wrong): 1 output stores, 2 weight loads from
#define M2M_NG_SKIP 0       // memory (one chunk re-used), 4 the MFMAs, 8 the x loads of the prologue (one row re-used)
#endif
constexpr int NG_BM = 128, NG_BN = 128, NG_BK = 64, NG_THREADS = 512;
constexpr int NG_BP = NG_BK + 8;                   // pitch of a weight chunk in the ring (elements)
constexpr int NG_CP = NG_BN + 8;                   // pitch of the staged result tile
constexpr int NG_STAGES = 3, NG_STAGE = NG_BN * NG_BP;

// LDS: the normalised panel [128][K + 8] — after every wave has taken its A fragments the same bytes hold the ring [3][128][72] —
// and the staged result tile [128][136]
__host__ __device__ inline size_t ng_lds_bytes(int K) {
  const size_t panel = (size_t)NG_BM * (K + 8), ring = (size_t)NG_STAGES * NG_STAGE;
  return ((panel > ring ? panel : ring) + (size_t)NG_BM * NG_CP) * 2;
}

__device__ inline uint2 ng_pack4(float a, float b, float c, float d) { return make_uint2(pack2_bf16(a, b), pack2_bf16(c, d)); }

template <int EPI, int NK>        // NK = K / 64 k chunks per column tile (d_model 128 / 256 / 384: 2 / 4 / 6)
__global__ __launch_bounds__(NG_THREADS) void norm_gemm_kernel(GemmArgs g) {
  using T = bf16_t;
  static_assert(EPI == EPI_HEADS || EPI == EPI_GATED || EPI == EPI_GATED16 || EPI == EPI_STORE_F32, "epilogues of the fused-norm products");
  static_assert(NK == 2 || NK == 4 || NK == 6, "chunk -> register set / ring stage / fragment buffer mapping below");
  extern __shared__ __align__(16) unsigned char ng_smem[];
  constexpr int K = NK * NG_BK, PP = K + 8;
  constexpr int RING = NG_STAGES * NG_STAGE, FRONT = NG_BM * PP > RING ? NG_BM * PP : RING;
  T* const panel = reinterpret_cast<T*>(ng_smem);               // [128][K + 8], then:
  T* const Bs = panel;                                           // [3][128][72] weight-chunk ring
  T* const Cs = panel + FRONT;                                   // [128][136] (transposed V tile: [128 cols][136])
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;                       // 4 x 2 waves: 32 rows x 64 columns each.  (Measured alternative: 4 waves
                                                                 // of 64 x 64 — ONE wave per SIMD, 192 VGPRs of A fragments, every weight
                                                                 // fragment feeding two MFMAs, half the LDS reads — QKV 54.8 -> 70.1 us:
                                                                 // a lone wave per SIMD does not hide its own LDS / barrier latencies.)
  const int r = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * NG_BM;
  // Column groups (round 6, small problems): gridDim.y workgroups share a row block, each normalises the panel for itself (the rows
  // come from L2 again, the arithmetic is the same) and sweeps ITS share of the column tiles - so a problem of a few row blocks still
  // spreads over the chip without a separate norm launch.  nt_lo = first tile of this group; everything below counts tiles locally.
  const int ntn_all = (g.N + NG_BN - 1) / NG_BN;
  const int tpg = (ntn_all + (int)gridDim.y - 1) / (int)gridDim.y;
  const int nt_lo = (int)blockIdx.y * tpg;
  const int ntn = min(tpg, ntn_all - nt_lo);
  if (ntn <= 0) return;                                          // (uniform: a trailing group without tiles)
  const T* W = reinterpret_cast<const T*>(g.W);
  // (Measured and dropped: every workgroup starting its sweep at a different column tile, so that the 216 of them do not ask the L2
  // for the same 16 KB of weights at the same moment — encoder + cross-K/V 1.912 / 1.937 against 1.917 / 1.932 ms on the same box:
  // the stream is not held up by hot L2 channels.)

  // weight chunk staging: 128 rows x 8 chunks of 16 bytes = 2 per thread, named scalars (arrays across the loop go to scratch).
  // THREE chunks stay in flight per thread (register sets a, b, c in rotation; the k loop is unrolled, so the set of a chunk is a
  // compile-time choice): with one workgroup per CU nothing else hides a chunk's L2 round trip — one chunk ahead measured ~1 us per
  // k step (QKV 78 us), the whole round trip exposed at every one of the 72 steps.
  const int c0 = tid, c1 = tid + NG_THREADS;
  const int br0 = c0 >> 3, bc0 = (c0 & 7) * 8, br1 = c1 >> 3, bc1 = (c1 & 7) * 8;
  uint4 ra0, ra1, rb0, rb1, rc0, rc1;
  // flat chunk index t = nt * NK + kt over the whole sweep; chunk t lives in register set t % 3 and goes to ring stage t % 3
#define NG_LOADB(set_, t_)                                                                                         \
  {                                                                                                                \
    const int tt_ = (M2M_NG_SKIP & 2) ? min((t_), 2) : (t_);                                                       \
    const int n0_ = (nt_lo + tt_ / NK) * NG_BN, k0_ = (tt_ % NK) * NG_BK;                                          \
    r##set_##0 = *reinterpret_cast<const uint4*>(W + (int64_t)min(n0_ + br0, g.N - 1) * K + k0_ + bc0);           \
    r##set_##1 = *reinterpret_cast<const uint4*>(W + (int64_t)min(n0_ + br1, g.N - 1) * K + k0_ + bc1);           \
  }
#define NG_STOREB(set_, stage_)                                                                                    \
  {                                                                                                                \
    *reinterpret_cast<uint4*>(Bs + (stage_) * NG_STAGE + br0 * NG_BP + bc0) = r##set_##0;                          \
    *reinterpret_cast<uint4*>(Bs + (stage_) * NG_STAGE + br1 * NG_BP + bc1) = r##set_##1;                          \
  }
  // loads are UNCONDITIONAL (past the end the last chunk is fetched again and never used): behind a runtime test the compiler cannot
  // count the loads in flight and waits vmcnt(0) at every step
#define NG_LOADB_SET(set_i_, t_) { if ((set_i_) == 0) NG_LOADB(a, t_) else if ((set_i_) == 1) NG_LOADB(b, t_) else NG_LOADB(c, t_) }
#define NG_STOREB_SET(set_i_) { if ((set_i_) == 0) NG_STOREB(a, 0) else if ((set_i_) == 1) NG_STOREB(b, 1) else NG_STOREB(c, 2) }
  const int nchunks = ntn * NK;
  NG_LOADB(a, 0)                                                 // in flight under the panel's prologue
  NG_LOADB(b, min(1, nchunks - 1))
  NG_LOADB(c, min(2, nchunks - 1))

  // ---- 1. the row panel: rmsnorm_kernel's arithmetic, a wave per row, 8 rows of loads in flight per wave ----
  {
    constexpr int RB = 8;
    const bool one = lane * 4 < K, two = lane * 4 + 256 < K;     // this lane's column chunks (K = 384: every lane has the first, lanes 0..31 the second)
    const float4 gw0 = one ? *reinterpret_cast<const float4*>(g.nw + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 gw1 = two ? *reinterpret_cast<const float4*>(g.nw + lane * 4 + 256) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int rb = 0; rb < NG_BM / 8; rb += RB) {
      float4 v0[RB], v1[RB];
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const float* xr = g.nx + (int64_t)((M2M_NG_SKIP & 8) ? 0 : min(m0 + wave * (NG_BM / 8) + rb + i, g.M - 1)) * K;
        v0[i] = one ? *reinterpret_cast<const float4*>(xr + lane * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        v1[i] = two ? *reinterpret_cast<const float4*>(xr + lane * 4 + 256) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int i = 0; i < RB; ++i) {
        const int rl = wave * (NG_BM / 8) + rb + i;
        float ss = 0.f;
        if (one) ss = ss + rms_sumsq4(v0[i]);
        if (two) ss = ss + rms_sumsq4(v1[i]);
        ss = wave_sum(ss);
        const float rstd = rsqrtf(ss / (float)K + g.neps);
        if (one) {
          const float4 v = v0[i];
          const float y0 = gw0.x * (v.x * rstd), y1 = gw0.y * (v.y * rstd), y2 = gw0.z * (v.z * rstd), y3 = gw0.w * (v.w * rstd);
          const uint2 pk = make_uint2(pack2_bf16(y0, y1), pack2_bf16(y2, y3));
          *reinterpret_cast<uint2*>(panel + rl * PP + lane * 4) = pk;
          if (g.h_out && blockIdx.y == 0 && m0 + rl < g.M) *reinterpret_cast<uint2*>(reinterpret_cast<T*>(g.h_out) + (int64_t)(m0 + rl) * K + lane * 4) = pk;
        }
        if (two) {
          const float4 v = v1[i];
          const float y0 = gw1.x * (v.x * rstd), y1 = gw1.y * (v.y * rstd), y2 = gw1.z * (v.z * rstd), y3 = gw1.w * (v.w * rstd);
          const uint2 pk = make_uint2(pack2_bf16(y0, y1), pack2_bf16(y2, y3));
          *reinterpret_cast<uint2*>(panel + rl * PP + lane * 4 + 256) = pk;
          if (g.h_out && blockIdx.y == 0 && m0 + rl < g.M) *reinterpret_cast<uint2*>(reinterpret_cast<T*>(g.h_out) + (int64_t)(m0 + rl) * K + lane * 4 + 256) = pk;
        }
      }
    }
  }

  // ---- 2. this wave's A fragments -> registers (32 rows x K: NK * 4 fragments, 4 VGPRs each), then the panel's LDS becomes the ring ----
  __syncthreads();                                               // the panel is complete
  Frag<T> af[NK][NG_BK / 16];
  {
    const T* const pa = panel + (wm * 32 + r) * PP + 8 * h;
#pragma unroll
    for (int kt = 0; kt < NK; ++kt)
#pragma unroll
      for (int s = 0; s < NG_BK / 16; ++s) af[kt][s] = load_frag(pa + kt * NG_BK + s * 16);
  }
  __syncthreads();                                               // every wave has its fragments: the panel bytes are free
  NG_STOREB(a, 0)                                                // chunks 0, 1 -> stages 0, 1; their sets take chunks 3, 4
  NG_STOREB(b, 1)
  NG_LOADB(a, min(3, nchunks - 1))
  NG_LOADB(b, min(4, nchunks - 1))
  __syncthreads();
  // Weight fragments: this wave's 64 columns (two 32-column MFMA blocks) of one 16-wide k step, read TWO k steps ahead of their
  // MFMAs into three rotating slots (24 VGPRs; a whole chunk ahead would be 64 and spills) — continuously, across chunk and tile
  // boundaries: the matrix core never waits for an LDS round trip.
  Frag<T> fws[3][2];                                             // [slot][block]; flat k-step index U: slot U % 3
  const T* const pb = Bs + (wn * 64 + r) * NG_BP + 8 * h;
#define NG_READ1(slot_, stage_, s_)                                                                                \
  {                                                                                                                \
    fws[slot_][0] = load_frag(pb + (stage_) * NG_STAGE + (s_) * 16);                                               \
    fws[slot_][1] = load_frag(pb + (stage_) * NG_STAGE + 32 * NG_BP + (s_) * 16);                                  \
  }
  NG_READ1(0, 0, 0)
  NG_READ1(1, 0, 1)

  // ---- 3. all column tiles.  Body t (chunk t, four k steps): each k step first requests the fragments of the step two ahead (the
  //         last two steps of a body read chunk t + 1: stage (t + 1) % 3, complete since the previous barrier), then multiplies; then
  //         chunk t + 2 goes from its register set into stage (t + 2) % 3 (last read in body t - 1) and the set is refilled with
  //         chunk t + 5; ONE barrier.  Chunk -> set / stage (t % 3) and k step -> slot depend on kt alone when NK % 3 == 0
  //         (K = 384); the small geometries (NK = 2, 4) walk three tiles per trip of the outer loop so that the pattern repeats. ----
  constexpr int TPT = (NK % 3 == 0) ? 1 : 3;
  // SW_: weights as the MFMA A operand (a lane then holds 4 consecutive OUTPUT COLUMNS of one row: row-major staging with 8-byte
  // writes); !SW_: activations as the A operand (4 consecutive ROWS of one column: the transposed V tile)
#define NG_KLOOP(SW_)                                                                                              \
  _Pragma("unroll") for (int kt = 0; kt < NK; ++kt) {                                                              \
    const int t = nt * NK + kt;                                                                                    \
    const int q = ti * NK + kt;                         /* == t modulo 3: compile-time after unrolling */           \
    _Pragma("unroll") for (int s = 0; s < NG_BK / 16; ++s) {                                                       \
      const int U = q * (NG_BK / 16) + s;                                                                          \
      NG_READ1((U + 2) % 3, (q + ((s + 2) >> 2)) % 3, (s + 2) & 3)                                                 \
      if (M2M_NG_SKIP & 4) { acc0[s] += __uint_as_float(fws[U % 3][0].v.x ^ af[kt][s].v.x); acc1[s] += __uint_as_float(fws[U % 3][1].v.y ^ af[kt][s].v.w); } \
      else if (SW_) { mma16(acc0, fws[U % 3][0], af[kt][s]); mma16(acc1, fws[U % 3][1], af[kt][s]); }              \
      else { mma16(acc0, af[kt][s], fws[U % 3][0]); mma16(acc1, af[kt][s], fws[U % 3][1]); }                       \
    }                                                                                                              \
    NG_STOREB_SET((q + 2) % 3)                                                                                     \
    NG_LOADB_SET((q + 2) % 3, min(t + 5, nchunks - 1))                                                             \
    __syncthreads();                                                                                               \
  }
  for (int nt0 = 0; nt0 < ntn; nt0 += TPT) {
#pragma unroll
  for (int ti = 0; ti < TPT; ++ti) {
    const int nt = nt0 + ti;
    if (nt >= ntn) break;                                         // uniform
    const int n0 = (nt_lo + nt) * NG_BN;
    f32x16 acc0 = zero_acc(), acc1 = zero_acc();
    // ---- epilogue of this tile follows its k loop (Cs is its own buffer: the stores overlap the next tile's first k steps; the
    //      next write of Cs is a whole k loop of barriers away).  Measured alternative: the staged tile leaving in pieces, one per
    //      k chunk of the NEXT tile (no burst, every store three chunks ahead of the first vmcnt wait that covers it): QKV 54.8 ->
    //      60.0 us, cross-K/V 219 -> 236 — the stores' cost (30 % of the kernel by ablation) is memory write time, not their burst ----
    if constexpr (EPI == EPI_STORE_F32) {
      NG_KLOOP(true)
      const int row = m0 + wm * 32 + r;
      if (row < g.M) {
        float* o = reinterpret_cast<float*>(g.out) + (int64_t)row * g.ldo;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {
            const f32x16& ac = j ? acc1 : acc0;
            const int col = n0 + wn * 64 + j * 32 + 8 * q4 + 4 * h;
            if (col + 4 <= g.N && (g.ldo & 3) == 0) *reinterpret_cast<float4*>(o + col) = make_float4(ac[4 * q4], ac[4 * q4 + 1], ac[4 * q4 + 2], ac[4 * q4 + 3]);
            else
              for (int k2 = 0; k2 < 4; ++k2) if (col + k2 < g.N) o[col + k2] = ac[4 * q4 + k2];
          }
      }
    } else if constexpr (EPI == EPI_HEADS) {
      const int which = n0 / g.inner;
      const bool transposed = (which == g.vt_which);
      if (transposed) {
        NG_KLOOP(false)
        // accumulator element e of lane (r, h): row wm * 32 + (e & 3) + 8 (e >> 2) + 4 h, column wn * 64 + j * 32 + r
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          *reinterpret_cast<uint2*>(Cs + (wn * 64 + r) * NG_CP + wm * 32 + 8 * q4 + 4 * h) = ng_pack4(acc0[4 * q4], acc0[4 * q4 + 1], acc0[4 * q4 + 2], acc0[4 * q4 + 3]);
          *reinterpret_cast<uint2*>(Cs + (wn * 64 + 32 + r) * NG_CP + wm * 32 + 8 * q4 + 4 * h) = ng_pack4(acc1[4 * q4], acc1[4 * q4 + 1], acc1[4 * q4 + 2], acc1[4 * q4 + 3]);
        }
      } else {
        NG_KLOOP(true)
        // swapped roles: element e of lane (r, h): row wm * 32 + r, column wn * 64 + j * 32 + (e & 3) + 8 (e >> 2) + 4 h
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          *reinterpret_cast<uint2*>(Cs + (wm * 32 + r) * NG_CP + wn * 64 + 8 * q4 + 4 * h) = ng_pack4(acc0[4 * q4], acc0[4 * q4 + 1], acc0[4 * q4 + 2], acc0[4 * q4 + 3]);
          *reinterpret_cast<uint2*>(Cs + (wm * 32 + r) * NG_CP + wn * 64 + 32 + 8 * q4 + 4 * h) = ng_pack4(acc1[4 * q4], acc1[4 * q4 + 1], acc1[4 * q4 + 2], acc1[4 * q4 + 3]);
        }
      }
      __syncthreads();
      for (int idx = tid; idx < ((M2M_NG_SKIP & 1) ? 0 : NG_BM * (NG_BN / 8)); idx += NG_THREADS) {
        if (!transposed) {
          const int rl = idx >> 4, ch = idx & 15;
          const int row = m0 + rl, col = n0 + ch * 8;
          if (row < g.M && col < g.N) {
            const int rem = col - which * g.inner, hh = rem / DK, dd = rem - hh * DK;
            const int b = row / g.S, sq = row - b * g.S;
            *reinterpret_cast<uint4*>(reinterpret_cast<T*>(g.out) + ((((int64_t)which * g.Bsz + b) * g.H + hh) * g.S + sq) * DK + dd) =
                *reinterpret_cast<const uint4*>(Cs + rl * NG_CP + ch * 8);
          }
        } else {
          const int cl = idx >> 4, rc = idx & 15;
          const int col = n0 + cl, row0 = m0 + rc * 8;
          if (col < g.N && row0 < g.M) {
            const int rem = col - which * g.inner, hh = rem / DK, dd = rem - hh * DK;
            const int b = row0 / g.S, s0 = row0 - b * g.S;
            T* dst = reinterpret_cast<T*>(g.vt_out) + (((int64_t)b * g.H + hh) * DK + dd) * g.Sp;
            const T* src = Cs + cl * NG_CP + rc * 8;
            if (s0 + 8 <= g.S && row0 + 8 <= g.M && (s0 & 7) == 0) {
              *reinterpret_cast<uint4*>(dst + s0) = *reinterpret_cast<const uint4*>(src);
            } else {                                              // chunk straddles a clip boundary / is misaligned
              for (int j = 0; j < 8; ++j) {
                const int row = row0 + j;
                if (row < g.M) {
                  const int bj = row / g.S, sj = row - bj * g.S;
                  reinterpret_cast<T*>(g.vt_out)[(((int64_t)bj * g.H + hh) * DK + dd) * g.Sp + sj] = src[j];
                }
              }
            }
          }
        }
      }
    } else {   // EPI_GATED (64-row chunks: 32 rows of wi_0 then the matching 32 of wi_1) / EPI_GATED16 (16-row groups: 8 + 8)
      constexpr int GP = NG_BN / 2 + 8;
      NG_KLOOP(true)
      T* const crow = Cs + (wm * 32 + r) * GP;
      if constexpr (EPI == EPI_GATED) {     // the wave's 64 weight rows are [32 of wi_0 | the matching 32 of wi_1]: acc0 = a, acc1 = b
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4)
          *reinterpret_cast<uint2*>(crow + wn * 32 + 8 * q4 + 4 * h) =
              ng_pack4(gelu_new_t<T>(acc0[4 * q4]) * acc1[4 * q4], gelu_new_t<T>(acc0[4 * q4 + 1]) * acc1[4 * q4 + 1],
                       gelu_new_t<T>(acc0[4 * q4 + 2]) * acc1[4 * q4 + 2], gelu_new_t<T>(acc0[4 * q4 + 3]) * acc1[4 * q4 + 3]);
      } else {                               // tile column c: a gate value if (c & 8) == 0, its partner at c + 8 = element e + 4 of the same lane
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int g2 = 0; g2 < 2; ++g2) {
            const f32x16& ac = j ? acc1 : acc0;
            *reinterpret_cast<uint2*>(crow + (wn * 4 + j * 2 + g2) * 8 + 4 * h) =
                ng_pack4(gelu_new_t<T>(ac[8 * g2]) * ac[8 * g2 + 4], gelu_new_t<T>(ac[8 * g2 + 1]) * ac[8 * g2 + 5],
                         gelu_new_t<T>(ac[8 * g2 + 2]) * ac[8 * g2 + 6], gelu_new_t<T>(ac[8 * g2 + 3]) * ac[8 * g2 + 7]);
          }
      }
      __syncthreads();
      for (int idx = tid; idx < ((M2M_NG_SKIP & 1) ? 0 : NG_BM * (NG_BN / 16)); idx += NG_THREADS) {
        const int rl = idx >> 3, ch = idx & 7;
        const int row = m0 + rl, oc = n0 / 2 + ch * 8;
        if (row < g.M && 2 * oc < g.N)
          *reinterpret_cast<uint4*>(reinterpret_cast<T*>(g.out) + (int64_t)row * g.ldo + oc) = *reinterpret_cast<const uint4*>(Cs + rl * GP + ch * 8);
      }
    }
  }   // tiles of a trip
  }
#undef NG_KLOOP
#undef NG_READ1
#undef NG_LOADB_SET
#undef NG_STOREB_SET
#undef NG_LOADB
#undef NG_STOREB
}

// One workgroup per 128 rows and no second workgroup per CU: the fused kernel needs about a chip's worth of row blocks to beat the
// 128 x 128 tiling (which spreads a small problem over rows AND columns).  B = 32 x S = 864 gives 216, the reference-native 128 x 190
// gives 190; below M2M_NORM_GEMM_MIN_BLOCKS (default 160) the two-kernel path runs.  M2M_NORM_GEMM: "0" never, "force" whatever the
// size (the parity tests), "e<digits>" not for the listed epilogue ids (diagnostic).  Latched per session (t5.h EncSwitches).
static bool norm_gemm_on(int epi, int M) {
  const EncSwitches& sw = enc_switches_now();
  if (sw.norm_gemm == 1) return false;
  if (sw.norm_gemm_skip) return !((sw.norm_gemm_skip >> epi) & 1u);
  if (sw.norm_gemm == 2) return true;
  return ceil_div(M, 128) >= sw.min_blocks || sw.norm_gemm_split;
}
// column groups per row block: one from a chip's worth of row blocks on (the round-5 form), else as many as keep the launch at about
// one workgroup per CU - down to one column tile per workgroup (M2M_NORM_GEMM_SPLIT=0: never split, the two-kernel path below the gate)
static int norm_gemm_groups(int M, int N) {
  const EncSwitches& sw = enc_switches_now();
  const int rb = ceil_div(M, NG_BM), ntn = ceil_div(N, NG_BN);
  if (rb >= sw.min_blocks || !sw.norm_gemm_split) return 1;
  int gq = 256 / rb;
  if (gq < 1) gq = 1;
  return gq > ntn ? ntn : gq;
}

// the switches as the environment has them now (a session or a trainer latches the result when it is created: t5.h EncSwitches)
thread_local const EncSwitches* tl_enc_switches = nullptr;
EncSwitches read_enc_switches() {
  EncSwitches sw;
  const auto tri = [](const char* v) { return !v ? 0 : v[0] == '0' ? 1 : v[0] == 'f' ? 2 : 0; };
  const char* ng = env_str("M2M_NORM_GEMM");
  sw.norm_gemm = tri(ng);
  if (ng && ng[0] == 'e') for (const char* c = ng + 1; *c; ++c) if (*c >= '0' && *c <= '9') sw.norm_gemm_skip |= 1u << (*c - '0');
  sw.resid_panel = tri(env_str("M2M_RESID_PANEL"));
  sw.attn_wide = env_on("M2M_ATTN_WIDE");
  sw.min_blocks = env_int("M2M_NORM_GEMM_MIN_BLOCKS", sw.min_blocks);
  sw.norm_gemm_hout = env_set("M2M_NORM_GEMM_HOUT");
  sw.norm_gemm_split = env_on("M2M_NORM_GEMM_SPLIT");
  sw.gemm_small_below = env_int("M2M_GEMM_SMALL_BELOW", sw.gemm_small_below);
  const char* dma = env_str("M2M_GEMM_DMA");
  sw.gemm_dma = !dma ? 1 : dma[0] == '0' ? 0 : dma[0] == 'a' ? 2 : 1;
  sw.gemm_dma_ns1 = env_int("M2M_GEMM_DMA_NS1", sw.gemm_dma_ns1);
  sw.gemm_dma_ns2 = env_int("M2M_GEMM_DMA_NS2", sw.gemm_dma_ns2);
  sw.gemm_dma_mink = env_int("M2M_GEMM_DMA_MINK", sw.gemm_dma_mink);
  sw.gemm_dma_maxt = env_int("M2M_GEMM_DMA_MAXT", sw.gemm_dma_maxt);
  return sw;
}
const EncSwitches& process_enc_switches() { static const EncSwitches sw = read_enc_switches(); return sw; }

int launch_norm_gemm(int precision, int epi, const GemmArgs& a_in, hipStream_t st) {
  {
  const GemmArgs& a = a_in;
  M2M_REQUIRE(a.nx && a.nw && a.A, "norm_gemm: null input (nx, nw, and A as the fallback's scratch for the normalised rows)");
  M2M_REQUIRE(epi == EPI_HEADS || epi == EPI_GATED || epi == EPI_GATED16 || epi == EPI_STORE_F32, "norm_gemm: epilogue %d not supported", epi);
  const bool fused = precision == M2M_PREC_BF16 && norm_gemm_on(epi, a.M) && (a.K == 128 || a.K == 256 || a.K == 384) &&
                     ng_lds_bytes(a.K) <= 160 * 1024 && (epi != EPI_HEADS || a.inner % NG_BN == 0) &&
                     (epi != EPI_GATED || a.N % 64 == 0) && (epi != EPI_GATED16 || a.N % 16 == 0);
  if (!fused) {
    int rc = launch_rmsnorm(precision, a.nx, a.nw, const_cast<void*>(a.A), a.M, a.K, a.neps, st);
    if (rc != M2M_OK) return rc;
    if (a.h_out && a.h_out != a.A)
      M2M_CHECK_HIP(hipMemcpyAsync(a.h_out, a.A, (size_t)a.M * a.K * (precision == M2M_PREC_BF16 ? 2 : 4), hipMemcpyDeviceToDevice, st));
    return launch_gemm(precision, epi, a, st);
  }
  M2M_REQUIRE(a.M >= 1 && a.N >= 1, "norm_gemm: empty problem");
  }
  GemmArgs a2 = a_in;
  if (!a2.h_out && enc_switches_now().norm_gemm_hout) a2.h_out = const_cast<void*>(a2.A);      // diagnostic: the panel also goes to the fallback's h buffer
  const GemmArgs& a = a2;
  const size_t smem = ng_lds_bytes(a.K);
  dim3 grid((unsigned)ceil_div(a.M, NG_BM), (unsigned)norm_gemm_groups(a.M, a.N));
#define NG_GO_K(E_, NK_)                                                                     \
  do {                                                                                       \
    M2M_OPT_IN_LDS((norm_gemm_kernel<E_, NK_>), 160 * 1024);                                 \
    hipLaunchKernelGGL((norm_gemm_kernel<E_, NK_>), grid, dim3(NG_THREADS), smem, st, a);    \
  } while (0)
#define NG_GO(E_) do { if (a.K == 384) NG_GO_K(E_, 6); else if (a.K == 256) NG_GO_K(E_, 4); else NG_GO_K(E_, 2); } while (0)
  switch (epi) {
    case EPI_HEADS: NG_GO(EPI_HEADS); break;
    case EPI_GATED: NG_GO(EPI_GATED); break;
    case EPI_GATED16: NG_GO(EPI_GATED16); break;
    default: NG_GO(EPI_STORE_F32); break;
  }
#undef NG_GO
#undef NG_GO_K
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

}  // namespace m2m

#ifdef M2M_RP_STAMP
extern "C" int m2m_debug_rp_stamps(unsigned long long* out_host) {      // diagnostic builds only (not declared in the public header)
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(m2m::g_rp_stamp), sizeof(unsigned long long) * 64) == hipSuccess ? 0 : -1;
}
#endif
#ifdef M2M_GEMM_STAMP
// diagnostic builds only (not declared in the public header)
extern "C" int m2m_debug_gemm_stamps(unsigned long long* out_host) {
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(m2m::g_gemm_stamp), sizeof(unsigned long long) * 8 * 3 * 8) == hipSuccess ? 0 : -1;
}
#endif
