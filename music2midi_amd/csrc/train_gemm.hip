// The products of the training step that are the trainer's own (train.hip drives them through the launchers of train.h): the
// strided / batched GEMM of the attention products and the split-K fallbacks, the weight-gradient GEMM alone and as the grouped
// launch of a whole step, the transposes, and the per-step copies of the weights (transposed, interleaved, MXFP8).
#include "mma.h"
#include "t5.h"
#include "train.h"

#include <vector>

namespace m2m {

// ============================================================ strided batched GEMM ====
// C[z][M,N] (op)= alpha * A[z][M,K] . B[z][N,K]^T,  z = (b1, b2) with independent strides per operand.
// 64x64 output tile per 256-thread workgroup (2x2 waves, one 32x32 MFMA tile each), BK = 32.
// Operand storage: a_kmajor == 0: element (m, k) at A[m*lda + k]; a_kmajor == 1: at A[k*lda + m]
// (the transposed product reads the buffer as it is: the tile is transposed on its way into LDS).
// k extent staged per step: 96 (bf16) / 64 (fp32).  The attention products reduce over <= ~360 keys / queries, so the dependent
// load -> LDS -> MFMA chain of a workgroup is 3 steps instead of the 9 of BK = 32 (16 -> us per launch).  96 rather than 128 for
// bf16 (round 3): 26.6 KB of LDS instead of 34.8 — five workgroups per CU (97 registers allow them) instead of four, so the
// 1 280 workgroups of the paired dV | dK launch of a 16-clip step are ONE round of the chip, and 261 keys are three steps either way
// (18 launches per step, 17.8 -> 16.3 us each; M2M_TG_BK at build time for measurements).

template <typename T> struct TgCfg;
#ifndef M2M_TG_BK
#define M2M_TG_BK 96
#endif
template <> struct TgCfg<bf16_t> { static constexpr int E = 8, BK = M2M_TG_BK, PITCH = BK + 8; };
template <> struct TgCfg<float> { static constexpr int E = 4, BK = 64, PITCH = BK + 4; };

// one operand tile [64 rows][32 k] -> LDS (row-major, k contiguous), zero-filled outside (rows_valid, k_valid).
// k-major operands: E x E blocks transposed in registers (16-byte LDS rows instead of 2-byte scatters), threads
// [tshift, tshift + blocks) do the work so that the A and the B tile of a step are staged by different waves; the row
// (non-reduction) index may run past `rows` inside the 16-byte chunk: those tile rows only feed outputs that are never stored
// (launch_bgemm checks that the padded row still lies inside the operand's row stride).
template <typename T>
__device__ inline void tg_stage(T* __restrict__ S, const T* __restrict__ G, int64_t ld, int kmajor, int row0, int k0,
                                int rows, int K, int tid, int tshift) {
  using Cfg = TgCfg<T>;
  constexpr int E = Cfg::E;
  if (!kmajor) {
    constexpr int TG_BK = Cfg::BK;
    constexpr int CPR = TG_BK / E;                      // chunks per row
    for (int c = tid; c < TG_BM * CPR; c += 256) {
      const int rl = c / CPR, kc = (c % CPR) * E;
      const int row = row0 + rl, k = k0 + kc;
      T* dst = S + rl * Cfg::PITCH + kc;
      if (row < rows && k + E <= K) {
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(G + (int64_t)row * ld + k);
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) dst[e] = (row < rows && k + e < K) ? G[(int64_t)row * ld + k + e] : from_f32<T>(0.f);
      }
    }
  } else {
    constexpr int KBn = Cfg::BK / E, RBn = TG_BM / E;   // blocks along k / along the tile rows
    const int c0 = tid - tshift;                                             // 128 threads per operand
    for (int c = c0; c0 >= 0 && c0 < 128 && c < KBn * RBn; c += 128) {
      const int kb = c % KBn, rb = c / KBn;
      const int row = row0 + rb * E;
      uint4 rg[E];
#pragma unroll
      for (int kk = 0; kk < E; ++kk) {
        const int k = k0 + kb * E + kk;
        rg[kk] = (k < K && row < rows) ? *reinterpret_cast<const uint4*>(G + (int64_t)k * ld + row) : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < E; ++j) *reinterpret_cast<uint4*>(S + (rb * E + j) * Cfg::PITCH + kb * E) = tr_col<T, E>(rg, j);
    }
  }
}

template <typename T, int EPI>
__global__ __launch_bounds__(256) void bgemm_kernel(BGemmArgs g) {
  using Cfg = TgCfg<T>;
  __shared__ __align__(16) T As[TG_BM * Cfg::PITCH];
  __shared__ __align__(16) T Bs[TG_BN * Cfg::PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;
  const bool split = g.ksplit > 1;
  const int nz = g.nb1 * g.nb2;
  // XCD-contiguous workgroup order (g.xcd_total > 0: 1-D launch; workgroup id % 8 picks the XCD): an XCD walks one eighth of the
  // (x, y, z) list front to back, so the row tiles of one (clip, head) product — which all read the same k-major operand — run
  // side by side on ONE XCD and meet in its L2 (dV / dK: 124 MB fetched per launch for 33 MB of operands with the launch order)
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (g.xcd_total > 0) {
    const int per = (g.xcd_total + 7) >> 3, l = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (l >= g.xcd_total || (int)(blockIdx.x >> 3) >= per) return;        // padding workgroups (uniform)
    bx = l % g.xcd_nx; by = (l / g.xcd_nx) % g.xcd_ny; bz = l / (g.xcd_nx * g.xcd_ny);
  }
  const bool second = !split && g.A2 && bz >= nz;            // pair mode: the second product of the launch
  const int zz = second ? bz - nz : bz;
  const int z1 = split ? 0 : zz / g.nb2, z2 = split ? 0 : zz - z1 * g.nb2;
  const T* A = reinterpret_cast<const T*>(second ? g.A2 : g.A) + z1 * g.sA1 + z2 * g.sA2;
  const T* B = second ? reinterpret_cast<const T*>(g.B2) + z1 * g.sB1_2 + z2 * g.sB2_2 : reinterpret_cast<const T*>(g.B) + z1 * g.sB1 + z2 * g.sB2;
  const int64_t ldb = second ? g.ldb2 : g.ldb;
  void* const Cout = second ? g.C2 : g.C;
  const int64_t coff = z1 * g.sC1 + z2 * g.sC2;
  const int m0 = by * TG_BM, n0 = bx * TG_BN;
  const int kbeg = split ? bz * g.kchunk : 0, kend = split ? min(g.K, kbeg + g.kchunk) : g.K;

  f32x16 acc = zero_acc();
  constexpr int TG_BK = Cfg::BK;
  for (int k0 = kbeg; k0 < kend; k0 += TG_BK) {
    __syncthreads();
    tg_stage<T>(As, A, g.lda, g.a_kmajor, m0, k0, g.M, kend, tid, 0);
    tg_stage<T>(Bs, B, ldb, g.b_kmajor, n0, k0, g.N, kend, tid, 128);
    __syncthreads();
#pragma unroll
    for (int s = 0; s < TG_BK / 16; ++s) {
      const Frag<T> fa = load_frag(As + (wm * 32 + r) * Cfg::PITCH + s * 16 + 8 * h);
      const Frag<T> fb = load_frag(Bs + (wn * 32 + r) * Cfg::PITCH + s * 16 + 8 * h);
      mma16(acc, fa, fb);
    }
  }
  const int col = n0 + wn * 32 + r;
  if (col >= g.N) return;
  const uint64_t dkey = (EPI == TG_RESID_F32 && g.drop_thresh) ? splitmix64(*g.drop_step + g.drop_key) : 0ull;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = m0 + wm * 32 + acc_row(i, lane);
    if (row >= g.M) continue;
    if (split) {                                   // partial tile of this k-slice
      g.Cpart[((int64_t)bz * g.M + row) * g.N + col] = acc[i];
      continue;
    }
    const int64_t at = coff + (int64_t)row * g.ldc + col;
    const float v = g.alpha * acc[i];
    if constexpr (EPI == TG_STORE_T) reinterpret_cast<T*>(Cout)[at] = from_f32<T>(v);
    else if constexpr (EPI == TG_STORE_F32) reinterpret_cast<float*>(Cout)[at] = v;
    else if constexpr (EPI == TG_ACC_F32) reinterpret_cast<float*>(Cout)[at] += v;
    else {                                                                       // TG_RESID_F32: C = R + dropout(acc)
      float u = v;
      if (g.drop_thresh) u = drop_keep(dkey, at, g.drop_thresh) ? v * g.drop_scale : 0.f;
      reinterpret_cast<float*>(Cout)[at] = g.R[at] + u;
    }
  }
}

template <typename T>
static int launch_bgemm_t(int epi, const BGemmArgs& g_in, hipStream_t st, bool xcd) {
  BGemmArgs g = g_in;
  dim3 grid((unsigned)ceil_div(g.N, TG_BN), (unsigned)ceil_div(g.M, TG_BM), (unsigned)(g.ksplit > 1 ? g.ksplit : g.nb1 * g.nb2 * (g.A2 ? 2 : 1)));
  if (xcd && (int64_t)grid.x * grid.y * grid.z >= 64 && (int64_t)grid.x * grid.y * grid.z < (1 << 30)) {
    g.xcd_nx = (int)grid.x; g.xcd_ny = (int)grid.y; g.xcd_total = (int)(grid.x * grid.y * grid.z);
    grid = dim3((unsigned)(8 * ceil_div(g.xcd_total, 8)));
  }
  switch (epi) {
    case TG_STORE_T: hipLaunchKernelGGL((bgemm_kernel<T, TG_STORE_T>), grid, dim3(256), 0, st, g); break;
    case TG_STORE_F32: hipLaunchKernelGGL((bgemm_kernel<T, TG_STORE_F32>), grid, dim3(256), 0, st, g); break;
    case TG_ACC_F32: hipLaunchKernelGGL((bgemm_kernel<T, TG_ACC_F32>), grid, dim3(256), 0, st, g); break;
    case TG_RESID_F32: hipLaunchKernelGGL((bgemm_kernel<T, TG_RESID_F32>), grid, dim3(256), 0, st, g); break;
    default: set_error("bgemm: bad epilogue %d", epi); return M2M_ERR_INVALID;
  }
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

// C[row][col] = alpha * sum_z part[z][row][col]   (z ascending: fixed order)
// (accumulate != 0: C[row][col] += alpha * sum — the accumulate mode of a weight gradient, m2m_train_forward_backward_acc)
__global__ void splitk_reduce_kernel(const float* __restrict__ part, float* __restrict__ C, int M, int N, int64_t ldc, int ksplit, float alpha,
                                     int accumulate) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = (int64_t)M * N, stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    float acc = 0.f;
    for (int z = 0; z < ksplit; ++z) acc += part[(int64_t)z * n + i];
    const int64_t row = i / N;
    float* c = C + row * ldc + (i - row * N);
    *c = accumulate ? *c + alpha * acc : alpha * acc;
  }
}

// ============================================================ weight-gradient GEMM ====
// C[N1, N2] (fp32) = A[K, N1]^T . B[K, N2]: both operands row-major with the REDUCTION index as the row (a weight
// gradient dW = dY^T . X reads dY [rows, N1] and X [rows, N2] exactly as the forward / backward passes left them).
// The MFMA wants 8 consecutive k per lane, memory has 8 consecutive n: every thread loads an E x E block (E rows of k,
// 16 bytes = E elements of n each; a wave's request is eight full 128-byte lines), transposes it IN REGISTERS (bf16:
// 32 v_perm_b32 per 8x8 block; fp32: pure renaming) and writes E 16-byte rows of the usual [n][k] LDS tile — the same
// number of LDS writes as a k-contiguous operand, where the generic kernel above scatters 2-byte elements.
// Tiles 128x128 (TF = 2) or 64x64 (TF = 1), BK = 64 / 32, next k-step prefetched into registers, split over k on
// blockIdx.z with fp32 partial tiles summed in z order by splitk_reduce_kernel (deterministic).
template <typename T> struct DwCfg;
template <> struct DwCfg<bf16_t> { static constexpr int BK = 64, E = 8; };
template <> struct DwCfg<float> { static constexpr int BK = 32, E = 4; };

// the epilogue's store: overwrite, or (accum, workgroup-uniform) add to what the buffer holds — one extra read per element
__device__ inline void dw_put(float* p, float v, int accum) { *p = accum ? *p + v : v; }

// one output tile [n1_0, +BT) x [n2_0, +BT) over k in [kbeg, kend), written to (accum: added to) out (row stride ldo)
template <typename T, int TF>
__device__ inline void dw_tile(const DwGemmArgs& g, T* __restrict__ AB, int n1_0, int n2_0, int kbeg, int kend, float* __restrict__ out, int64_t ldo,
                               int accum) {
  using Cfg = DwCfg<T>;
  constexpr int BK = Cfg::BK, E = Cfg::E, PITCH = BK + E;
  constexpr int BT = 64 * TF, WT = 32 * TF;
  constexpr int KB = BK / E, NB = BT / E, BPO = KB * NB, TB = 2 * BPO, NBT = (TB + 255) / 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int r = lane & 31, h = lane >> 5;

  // this thread's blocks: (operand, n block, k block); kb runs fastest over the lanes, so one store instruction of a wave
  // covers whole 128-byte LDS rows and one load instruction whole 128-byte lines of 8 k-rows
  const T* src[NBT];
  int64_t ld[NBT];
  int kofs[NBT], lds_off[NBT];
  bool ok[NBT];
#pragma unroll
  for (int u = 0; u < NBT; ++u) {
    const int bi = tid + 256 * u;
    const int op = bi / BPO, id = bi - op * BPO;
    const int kb = id % KB, nb = id / KB;
    const int n0 = op ? n2_0 : n1_0, nlim = op ? g.N2 : g.N1;
    ok[u] = bi < TB && n0 + nb * E + E <= nlim;
    src[u] = reinterpret_cast<const T*>(op ? g.B : g.A) + (ok[u] ? n0 + nb * E : 0);
    ld[u] = op ? g.ldb : g.lda;
    kofs[u] = kb * E;
    lds_off[u] = (min(op, 1) * BT + nb * E) * PITCH + kb * E;
  }
  uint4 rg[NBT][E];
  auto gload = [&](int k0) {
#pragma unroll
    for (int u = 0; u < NBT; ++u)
#pragma unroll
      for (int kk = 0; kk < E; ++kk) {
        const int k = k0 + kofs[u] + kk;
        const uint4 v = *reinterpret_cast<const uint4*>(src[u] + (int64_t)min(k, kend - 1) * ld[u]);   // clamped, never predicated
        rg[u][kk] = (ok[u] && k < kend) ? v : make_uint4(0, 0, 0, 0);
      }
  };
  auto sstore = [&]() {
#pragma unroll
    for (int u = 0; u < NBT; ++u) {
      if (TB < 256 && tid >= TB) continue;
#pragma unroll
      for (int j = 0; j < E; ++j) *reinterpret_cast<uint4*>(AB + lds_off[u] + j * PITCH) = tr_col<T, E>(rg[u], j);
    }
  };

  f32x16 acc[TF][TF];
#pragma unroll
  for (int i = 0; i < TF; ++i)
#pragma unroll
    for (int j = 0; j < TF; ++j) acc[i][j] = zero_acc();
  const T* As = AB;
  const T* Bs = AB + BT * PITCH;
  gload(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    __syncthreads();
    sstore();
    __syncthreads();
    if (k0 + BK < kend) gload(k0 + BK);
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      Frag<T> fa[TF], fb[TF];
#pragma unroll
      for (int i = 0; i < TF; ++i) {
        fa[i] = load_frag(As + (wm * WT + i * 32 + r) * PITCH + s * 16 + 8 * h);
        fb[i] = load_frag(Bs + (wn * WT + i * 32 + r) * PITCH + s * 16 + 8 * h);
      }
#pragma unroll
      for (int i = 0; i < TF; ++i)
#pragma unroll
        for (int j = 0; j < TF; ++j) mma16(acc[i][j], fa[i], fb[j]);
    }
  }
#pragma unroll
  for (int mi = 0; mi < TF; ++mi)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = n1_0 + wm * WT + mi * 32 + acc_row(e, lane);
      if (row >= g.N1) continue;
#pragma unroll
      for (int ni = 0; ni < TF; ++ni) {
        const int col = n2_0 + wn * WT + ni * 32 + r;
        if (col < g.N2) dw_put(out + (int64_t)row * ldo + col, acc[mi][ni][e], accum);
      }
    }
}

// The same 128 x 128 tile for bf16 WITHOUT the register transposes: the operands' k-major rows are copied to LDS as they lie in
// memory ([k][n], 320-byte rows: four consecutive k-rows fall into four different 16-bank groups), and an MFMA fragment — 8
// consecutive k of one column — is two `ds_read_b64_tr_b16` (gfx950's transposing LDS read: per 16 lanes a 4 x 16 block comes back
// column-major; lane map checked by tools/trprobe.hip).  What this buys is on the LOAD side: with an 8 x 8 register block per
// thread, neighbouring lanes had to sit in different k-rows (so that the transposed block lands in one LDS row), and every
// 16-byte request was a cache access of its own — PMC: 2.5e8 L1 accesses per launch for 3.9 GB, 77 % of the kernel's cycles per
// CU; here 16 neighbouring lanes read one 256-byte row segment.  ~140 VALU instructions per k-step and wave disappear with it.
constexpr int DWT_PITCH = 160;                       // bf16 elements per staged k-row: 128 + 32 of padding
typedef short dw_v4s __attribute__((ext_vector_type(4)));
__device__ inline Frag<bf16_t> dw_tr_frag(const bf16_t* p) {            // p: this lane's address of the first 4 k-rows (see dw_tile_tr)
  typedef dw_v4s __attribute__((address_space(3))) * lds_v4s;
  const dw_v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(p));
  const dw_v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(p + 4 * DWT_PITCH));
  Frag<bf16_t> f;
  f.v = make_uint4(__builtin_bit_cast(uint2, lo).x, __builtin_bit_cast(uint2, lo).y, __builtin_bit_cast(uint2, hi).x, __builtin_bit_cast(uint2, hi).y);
  return f;
}
// FULL: the tile lies inside the matrix on both sides (every tile of the projection weights; not the last tiles of lm_head):
// no column predicate anywhere.  The k loop runs whole 64-row steps from pointers that advance by a constant — no clamp, no
// select, no 64-bit multiply per load — and one guarded step takes the ragged end (M = 4 176 rows = 65 steps + 16 rows).
template <bool FULL>
__device__ inline void dw_tile_tr(const DwGemmArgs& g, bf16_t* __restrict__ AB, int n1_0, int n2_0, int kbeg, int kend, float* __restrict__ out,
                                  int64_t ldo, int accum) {
  constexpr int BK = 64, P = DWT_PITCH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // staging: threads 0..127 copy operand A (dY), 128..255 operand B (X); a thread owns 16-byte chunk `ch` of the k-rows
  // rw, rw + 8, ... rw + 56: 16 neighbouring lanes cover one 256-byte row segment
  const int op = tid >> 7, c = tid & 127, ch = c & 15, rw = c >> 4;
  const int n0 = op ? n2_0 : n1_0, nlim = op ? g.N2 : g.N1;
  const bool ok = FULL || n0 + ch * 8 + 8 <= nlim;
  const int64_t ld = op ? g.ldb : g.lda;
  const bf16_t* pk = reinterpret_cast<const bf16_t*>(op ? g.B : g.A) + (ok ? n0 + ch * 8 : 0) + (int64_t)(kbeg + rw) * ld;   // row rw of the current step
  const int64_t step = (int64_t)BK * ld, ld8 = 8 * ld;
  bf16_t* dst = AB + op * (BK * P) + rw * P + ch * 8;
  uint4 r0, r1, r2, r3, r4, r5, r6, r7;               // named: arrays across the k loop end up in scratch (hipcc 7.2)
#define M2M_DW_LD(u) { const uint4 v = *reinterpret_cast<const uint4*>(pk + (u) * ld8); r##u = ok ? v : make_uint4(0, 0, 0, 0); }
#define M2M_DW_LD_TAIL(u, k0) { const int k = (k0) + rw + 8 * (u); const uint4 v = *reinterpret_cast<const uint4*>(pk + (int64_t)(min(k, kend - 1) - ((k0) + rw)) * ld); \
                                r##u = (ok && k < kend) ? v : make_uint4(0, 0, 0, 0); }
#define M2M_DW_GLOAD() { M2M_DW_LD(0) M2M_DW_LD(1) M2M_DW_LD(2) M2M_DW_LD(3) M2M_DW_LD(4) M2M_DW_LD(5) M2M_DW_LD(6) M2M_DW_LD(7) }
#define M2M_DW_GLOAD_TAIL(k0) { M2M_DW_LD_TAIL(0, k0) M2M_DW_LD_TAIL(1, k0) M2M_DW_LD_TAIL(2, k0) M2M_DW_LD_TAIL(3, k0) M2M_DW_LD_TAIL(4, k0) \
                                M2M_DW_LD_TAIL(5, k0) M2M_DW_LD_TAIL(6, k0) M2M_DW_LD_TAIL(7, k0) }
#define M2M_DW_ST(u) *reinterpret_cast<uint4*>(dst + 8 * (u) * P) = r##u;
#define M2M_DW_SSTORE() { M2M_DW_ST(0) M2M_DW_ST(1) M2M_DW_ST(2) M2M_DW_ST(3) M2M_DW_ST(4) M2M_DW_ST(5) M2M_DW_ST(6) M2M_DW_ST(7) }
  // fragment addresses: lane = 16 g + 4 q + p supplies row q of its group's 4 x 16 block, columns 4p .. 4p+3; groups 0 / 1 are the
  // column halves of k 0..7, groups 2 / 3 those of k 8..15 (h = g >> 1) of a 16-deep substep
  const int li = lane & 15, q = li >> 2, pp = li & 3, gq = lane >> 4, h = lane >> 5;
  const bf16_t* fa = AB + (8 * h + q) * P + wm * 64 + 16 * (gq & 1) + 4 * pp;
  const bf16_t* fb = AB + BK * P + (8 * h + q) * P + wn * 64 + 16 * (gq & 1) + 4 * pp;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = zero_acc();
  const int nfull = (kend - kbeg) / BK;               // whole steps; a ragged one may follow
  const bool ragged = kbeg + nfull * BK < kend;
  const int nsteps = nfull + (ragged ? 1 : 0);
  if (nfull > 0) M2M_DW_GLOAD() else M2M_DW_GLOAD_TAIL(kbeg)
  for (int it = 0; it < nsteps; ++it) {
    __syncthreads();
    M2M_DW_SSTORE()
    __syncthreads();
    pk += step;
    if (it + 1 < nfull) M2M_DW_GLOAD()
    else if (it + 1 < nsteps) M2M_DW_GLOAD_TAIL(kbeg + (it + 1) * BK)
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      Frag<bf16_t> a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = dw_tr_frag(fa + 16 * s * P + 32 * i);
        b[i] = dw_tr_frag(fb + 16 * s * P + 32 * i);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) mma16(acc[i][j], a[i], b[j]);
    }
  }
#undef M2M_DW_LD
#undef M2M_DW_LD_TAIL
#undef M2M_DW_GLOAD
#undef M2M_DW_GLOAD_TAIL
#undef M2M_DW_ST
#undef M2M_DW_SSTORE
  const int r = lane & 31;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = n1_0 + wm * 64 + mi * 32 + acc_row(e, lane);
      if (!FULL && row >= g.N1) continue;
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) {
        const int col = n2_0 + wn * 64 + ni * 32 + r;
        if (FULL || col < g.N2) dw_put(out + (int64_t)row * ldo + col, acc[mi][ni][e], accum);
      }
    }
}

template <typename T, int TF>
__global__ __launch_bounds__(256) void dw_gemm_kernel(DwGemmArgs g) {
  constexpr int BT = 64 * TF, PITCH = DwCfg<T>::BK + DwCfg<T>::E;
  __shared__ __align__(16) T AB[2 * BT * PITCH];
  const bool split = g.ksplit > 1;
  const int kbeg = split ? blockIdx.z * g.kchunk : 0, kend = split ? min(g.K, kbeg + g.kchunk) : g.K;
  dw_tile<T, TF>(g, AB, blockIdx.y * BT, blockIdx.x * BT, kbeg, kend, split ? g.Cpart + (int64_t)blockIdx.z * g.N1 * g.N2 : g.C,
                 split ? (int64_t)g.N2 : g.ldc, split ? 0 : g.accum);
}

// Every weight gradient of a step in ONE launch: the backward pass only records (dY, X, dW) triples — each sub-layer
// keeps its dY operands in buffers of its own, 0.55 GB at 16 clips, nothing for a 288 GB part — and this kernel walks
// the table: workgroup -> (problem, 128x128 tile), full reduction length per tile.  ~1 850 tiles fill the 256 CUs
// seven times over, so no product is split over k: the split-K partial images (3.8 GB written and re-read per step
// for the 67 products, 134 launches) are gone.
template <typename T, bool TR>
__global__ __launch_bounds__(256) void dw_group_kernel(const DwProb* __restrict__ probs, int n_probs, int n_tiles, int xcd_order) {
  constexpr int PITCH = DwCfg<T>::BK + DwCfg<T>::E;
  constexpr int LDS_ELEMS = TR ? 2 * 64 * DWT_PITCH : 2 * 128 * PITCH;
  __shared__ __align__(16) T AB[LDS_ELEMS];
  // XCD-contiguous tile order (workgroup id % 8 picks the XCD): each XCD walks one eighth of the tile list front to back, so the
  // tiles that run side by side on an XCD are neighbours in the list — the same product, the same dY column block (tiles of a
  // product are numbered along X fastest), a handful of X column blocks — and their operand slices meet in that XCD's L2
  const int per = (n_tiles + 7) >> 3;
  const int tile = xcd_order ? (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  if (tile >= n_tiles || (xcd_order && (int)(blockIdx.x >> 3) >= per)) return;       // padding workgroups (uniform)
  int p = 0;
  while (p + 1 < n_probs && tile >= probs[p + 1].tile0) ++p;                          // uniform scan of <= ~70 entries
  const DwProb pr = probs[p];
  const int tl = tile - pr.tile0;
  if constexpr (TR) {
    const int n1_0 = (tl / pr.tn2) * 128, n2_0 = (tl % pr.tn2) * 128;
    if (n1_0 + 128 <= pr.g.N1 && n2_0 + 128 <= pr.g.N2) dw_tile_tr<true>(pr.g, AB, n1_0, n2_0, 0, pr.g.K, pr.g.C, pr.g.ldc, pr.g.accum);      // (workgroup-uniform)
    else dw_tile_tr<false>(pr.g, AB, n1_0, n2_0, 0, pr.g.K, pr.g.C, pr.g.ldc, pr.g.accum);
  } else dw_tile<T, 2>(pr.g, AB, (tl / pr.tn2) * 128, (tl % pr.tn2) * 128, 0, pr.g.K, pr.g.C, pr.g.ldc, pr.g.accum);
}

// C = A^T . B with the split chosen here: enough workgroups to fill the chip, as few k-slices as that allows (every slice
// writes and re-reads an fp32 image of C).
int launch_dw_gemm(int precision, const void* A, int64_t lda, int N1, const void* B, int64_t ldb, int N2, int K, float* C, int64_t ldc,
                   float* kpart, int64_t kpart_floats, hipStream_t st, int accumulate, const TrainSwitches& sw) {
  const int E = precision == M2M_PREC_BF16 ? 8 : 4, BK = precision == M2M_PREC_BF16 ? 64 : 32;
  M2M_REQUIRE(N1 % E == 0 && N2 % E == 0 && lda % E == 0 && ldb % E == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(B) & 15) == 0,
              "dw_gemm: operands must be 16-byte aligned with row lengths that are multiples of %d", E);
  const int t128 = ceil_div(N1, 128) * ceil_div(N2, 128);
  const int tf = sw.dw_tile == 64 ? 1 : 2;   // 128x128 measured faster for every weight shape of the model (16 clips: 8.80 vs 9.90 ms per step)
  (void)t128;
  const int bt = 64 * tf;
  const int tiles = ceil_div(N1, bt) * ceil_div(N2, bt);
  int ks = ceil_div(sw.dw_wgs, tiles);
  if (ks > 32) ks = 32;
  while (ks > 1 && ((int64_t)ks * N1 * N2 > kpart_floats || K / ks < 2 * BK)) --ks;
  DwGemmArgs g{};
  g.A = A; g.B = B; g.C = C; g.Cpart = kpart; g.N1 = N1; g.N2 = N2; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.ksplit = 1; g.kchunk = K;
  if (ks > 1) { g.kchunk = (int)align_up(ceil_div(K, ks), BK); g.ksplit = ceil_div(K, g.kchunk); }
  g.accum = accumulate;                   // (a split product adds in splitk_reduce_kernel; its partial tiles are stored)
  dim3 grid((unsigned)ceil_div(N2, bt), (unsigned)ceil_div(N1, bt), (unsigned)g.ksplit);
  if (precision == M2M_PREC_BF16) {
    if (tf == 2) hipLaunchKernelGGL((dw_gemm_kernel<bf16_t, 2>), grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL((dw_gemm_kernel<bf16_t, 1>), grid, dim3(256), 0, st, g);
  } else {
    if (tf == 2) hipLaunchKernelGGL((dw_gemm_kernel<float, 2>), grid, dim3(256), 0, st, g);
    else hipLaunchKernelGGL((dw_gemm_kernel<float, 1>), grid, dim3(256), 0, st, g);
  }
  M2M_CHECK_HIP(hipGetLastError());
  if (g.ksplit > 1) {
    const int64_t n = (int64_t)N1 * N2;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256)), dim3(256), 0, st, kpart, C, N1, N2,
                       ldc, g.ksplit, 1.0f, accumulate);
    M2M_CHECK_HIP(hipGetLastError());
  }
  return M2M_OK;
}

// dst[c][r] = src[r][c]: src [R][C] (row stride ld_s) -> dst [C][ld_d]; the columns [R, Rpad) of dst are zeroed
template <typename TS, typename TD>
__global__ __launch_bounds__(256) void transpose_kernel(const TS* __restrict__ src, int64_t ld_s, TD* __restrict__ dst, int64_t ld_d, int R, int C,
                                                        int Rpad) {
  __shared__ float tile[64][65];
  const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int rl = i >> 6, cl = i & 63;
    tile[rl][cl] = (r0 + rl < R && c0 + cl < C) ? to_f32(src[(int64_t)(r0 + rl) * ld_s + c0 + cl]) : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int cl = i >> 6, rl = i & 63;
    if (c0 + cl < C && r0 + rl < Rpad) dst[(int64_t)(c0 + cl) * ld_d + r0 + rl] = from_f32<TD>(tile[rl][cl]);
  }
}

// all weight matrices of the model in one launch: WT[off .. ] = W[off ..]^T in the storage type (block -> (matrix, tile) table)
// ... and, in the same pass over the fp32 master (Wc != null: bf16 mode), the plain copy in the storage type the forward products
// read: every matrix a product reads is in the table, so the separate conversion of the whole parameter buffer (30 us, 121 MB read
// a second time) is gone.  WT == null (a forward-only pass): the copy only.
// Wil (bf16 mode): the gate-pair matrices once more with their rows interleaved in 32-row chunks (wi_0 rows [32c, 32c + 32), then the
// matching wi_1 rows), the B operand of the fused gated-GELU product (EPI_GATED_TRAIN): a wave's 64 output columns are then a | b of
// the same 32 hidden units.
template <typename TD>
__global__ __launch_bounds__(256) void weights_transpose_kernel(const WtBlock* __restrict__ blocks, const float* __restrict__ P, TD* __restrict__ WT,
                                                                TD* __restrict__ Wc, TD* __restrict__ Wil) {
  __shared__ float tile[64][65];
  const WtBlock b = blocks[blockIdx.x];
  const int n0 = b.tn * 64, k0 = b.tk * 64;
  const float* src = P + b.off;
  TD* dst = WT + b.off;
  // four elements per thread and access (16-byte loads, 8-byte bf16 stores; the element-wise form moved 2 bytes per store: 62 us for the
  // step's 265 MB); tiles at a ragged edge (K or N not a multiple of 4 there) take the element-wise loop
  const bool vec = sizeof(TD) == 2 && (b.K & 3) == 0 && (b.N & 3) == 0 && ((b.off & 3) == 0);
  if (vec) {
    for (int i = threadIdx.x; i < 64 * 16; i += 256) {
      const int nl = i >> 4, kl = (i & 15) * 4;
      const bool in = n0 + nl < b.N && k0 + kl < b.K;          // (K % 4 == 0: the whole piece is inside or outside)
      const int64_t at = (int64_t)(n0 + nl) * b.K + k0 + kl;
      const float4 v = in ? *reinterpret_cast<const float4*>(src + at) : make_float4(0.f, 0.f, 0.f, 0.f);
      tile[nl][kl] = v.x; tile[nl][kl + 1] = v.y; tile[nl][kl + 2] = v.z; tile[nl][kl + 3] = v.w;
      if (in && (Wc || (Wil && b.il_half))) {
        const uint2 pk = make_uint2(pack2_bf16(v.x, v.y), pack2_bf16(v.z, v.w));
        if (Wc) *reinterpret_cast<uint2*>(Wc + b.off + at) = pk;
        if (Wil && b.il_half) {
          const int n = n0 + nl, m = n < b.il_half ? n : n - b.il_half;
          *reinterpret_cast<uint2*>(Wil + b.off + (int64_t)((m >> 5) * 64 + (n < b.il_half ? 0 : 32) + (m & 31)) * b.K + k0 + kl) = pk;
        }
      }
    }
    if (!WT) return;
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 16; i += 256) {
      const int kl = i >> 4, nl = (i & 15) * 4;
      if (k0 + kl < b.K && n0 + nl < b.N)
        *reinterpret_cast<uint2*>(dst + (int64_t)(k0 + kl) * b.N + n0 + nl) =
            make_uint2(pack2_bf16(tile[nl][kl], tile[nl + 1][kl]), pack2_bf16(tile[nl + 2][kl], tile[nl + 3][kl]));
    }
    return;
  }
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int nl = i >> 6, kl = i & 63;
    const bool in = n0 + nl < b.N && k0 + kl < b.K;
    const float v = in ? src[(int64_t)(n0 + nl) * b.K + k0 + kl] : 0.f;
    tile[nl][kl] = v;
    if (Wc && in) Wc[b.off + (int64_t)(n0 + nl) * b.K + k0 + kl] = from_f32<TD>(v);
    if (Wil && in && b.il_half) {
      const int n = n0 + nl, m = n < b.il_half ? n : n - b.il_half;
      Wil[b.off + (int64_t)((m >> 5) * 64 + (n < b.il_half ? 0 : 32) + (m & 31)) * b.K + k0 + kl] = from_f32<TD>(v);
    }
  }
  if (!WT) return;
  __syncthreads();
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int kl = i >> 6, nl = i & 63;
    if (k0 + kl < b.K && n0 + nl < b.N) dst[(int64_t)(k0 + kl) * b.N + n0 + nl] = from_f32<TD>(tile[nl][kl]);
  }
}

// fp8 mode: every projection matrix W [N][K] (fp32 master) -> MXFP8 in BOTH layouts in one launch: row-major with blocks
// along K (the forward's B operand) and transposed [K][Np] with blocks along N (the B operand of dX = dY . W).
// One 64-thread workgroup per 32 x 64 tile (table entry, W8Tile of train.h); e4m3.
__device__ inline float w8_scale_exp(float amax) {
  if (!(amax > 0.f)) return -127.f;
  int e;
  (void)frexpf(amax, &e);
  int se = e - 1 - 8;
  return (float)(se < -127 ? -127 : (se > 127 ? 127 : se));
}
__device__ inline uint32_t w8_pack4(float a, float b, float c, float d) {
  a = fminf(fmaxf(a, -448.f), 448.f); b = fminf(fmaxf(b, -448.f), 448.f); c = fminf(fmaxf(c, -448.f), 448.f); d = fminf(fmaxf(d, -448.f), 448.f);
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (uint32_t)w;
}
__global__ __launch_bounds__(64) void mxq_weights_kernel(const W8Tile* __restrict__ tiles, const float* __restrict__ P, uint8_t* __restrict__ w8) {
  __shared__ float tile[32][65];
  const W8Tile tl = tiles[blockIdx.x];
  const int n0 = tl.tn * 32, k0 = tl.tk * 64;
  const float* src = P + tl.off;
  for (int i = threadIdx.x; i < 32 * 64; i += 64) {
    const int nl = i >> 6, kl = i & 63;
    tile[nl][kl] = (n0 + nl < tl.N && k0 + kl < tl.K) ? src[(int64_t)(n0 + nl) * tl.K + k0 + kl] : 0.f;
  }
  __syncthreads();
  {  // rows: thread -> (row, k-block)
    const int nl = threadIdx.x >> 1, kb = threadIdx.x & 1;
    if (n0 + nl < tl.N && k0 + 32 * kb < tl.K) {
      float v[32], amax = 0.f;
#pragma unroll
      for (int j = 0; j < 32; ++j) { v[j] = tile[nl][32 * kb + j]; amax = fmaxf(amax, fabsf(v[j])); }
      const float se = w8_scale_exp(amax), inv = exp2f(-se);
      uint32_t* dst = reinterpret_cast<uint32_t*>(w8 + tl.q + (int64_t)(n0 + nl) * tl.K + k0 + 32 * kb);
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = w8_pack4(v[4 * j] * inv, v[4 * j + 1] * inv, v[4 * j + 2] * inv, v[4 * j + 3] * inv);
      w8[tl.qs + (int64_t)(n0 + nl) * (tl.K / 32) + (k0 + 32 * kb) / 32] = (uint8_t)((int)se + 127);
    }
  }
  {  // columns: thread -> column k, block of 32 rows n0 .. n0 + 31
    const int kl = threadIdx.x;
    if (k0 + kl < tl.K) {
      float v[32], amax = 0.f;
#pragma unroll
      for (int j = 0; j < 32; ++j) { v[j] = tile[j][kl]; amax = fmaxf(amax, fabsf(v[j])); }
      const float se = w8_scale_exp(amax), inv = exp2f(-se);
      uint32_t* dst = reinterpret_cast<uint32_t*>(w8 + tl.qt + (int64_t)(k0 + kl) * tl.Np + n0);
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[j] = w8_pack4(v[4 * j] * inv, v[4 * j + 1] * inv, v[4 * j + 2] * inv, v[4 * j + 3] * inv);
      w8[tl.qts + (int64_t)(k0 + kl) * (tl.Np / 32) + n0 / 32] = (uint8_t)((int)se + 127);
    }
  }
}
W8Lin w8_add_matrix(int64_t off, int N, int K, int64_t& w8_bytes, std::vector<W8Tile>& tiles) {
  W8Lin w{off, N, K, (int)align_up(N, 128), 0, 0, 0, 0};
  w.q = w8_bytes; w8_bytes = align_up(w8_bytes + (int64_t)N * K, 256);
  w.qs = w8_bytes; w8_bytes = align_up(w8_bytes + (int64_t)N * (K / 32), 256);
  w.qt = w8_bytes; w8_bytes = align_up(w8_bytes + (int64_t)K * w.Np, 256);
  w.qts = w8_bytes; w8_bytes = align_up(w8_bytes + (int64_t)K * (w.Np / 32), 256);
  for (int tn = 0; tn < ceil_div(N, 32); ++tn)
    for (int tk = 0; tk < ceil_div(K, 64); ++tk) tiles.push_back({off, N, K, w.Np, w.q, w.qs, w.qt, w.qts, tn, tk});
  return w;
}
int launch_mxq_weights(const W8Tile* tiles_dev, int n_tiles, const float* P, uint8_t* w8, hipStream_t st) {
  hipLaunchKernelGGL(mxq_weights_kernel, dim3(n_tiles), dim3(64), 0, st, tiles_dev, P, w8);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

int launch_bgemm(int precision, int epi, const BGemmArgs& g, hipStream_t st, const TrainSwitches& sw) {
  const int E = precision == M2M_PREC_BF16 ? 8 : 4;
  M2M_REQUIRE(g.M >= 1 && g.N >= 1 && g.K >= 1 && g.nb1 >= 1 && g.nb2 >= 1, "bgemm: empty problem");
  M2M_REQUIRE(g.lda % E == 0 && g.ldb % E == 0, "bgemm: operand row strides (%lld, %lld) must be multiples of %d elements (16-byte rows)",
              (long long)g.lda, (long long)g.ldb, E);
  M2M_REQUIRE(g.sA1 % E == 0 && g.sA2 % E == 0 && g.sB1 % E == 0 && g.sB2 % E == 0, "bgemm: batch strides must keep 16-byte alignment");
  M2M_REQUIRE((int64_t)g.nb1 * g.nb2 * (g.A2 ? 2 : 1) <= 65535, "bgemm: too many batch entries");
  M2M_REQUIRE(!g.A2 || (g.B2 && g.C2 && g.ksplit <= 1 && g.ldb2 % E == 0 && g.sB1_2 % E == 0 && g.sB2_2 % E == 0 && (!g.b_kmajor || g.ldb2 >= align_up(g.N, E))),
              "bgemm: bad second product");
  M2M_REQUIRE((!g.a_kmajor || g.lda >= align_up(g.M, E)) && (!g.b_kmajor || g.ldb >= align_up(g.N, E)),
              "bgemm: a k-major operand's row stride must cover its rows padded to %d", E);
  if (g.ksplit > 1) {
    M2M_REQUIRE(g.nb1 == 1 && g.nb2 == 1 && (epi == TG_STORE_F32 || epi == TG_ACC_F32) && g.Cpart && g.kchunk % TG_BK_MAX == 0,
                "bgemm: split-K is for plain fp32-store / fp32-accumulate products");
    int rc = precision == M2M_PREC_BF16 ? launch_bgemm_t<bf16_t>(epi, g, st, sw.xcd_order) : launch_bgemm_t<float>(epi, g, st, sw.xcd_order);
    if (rc != M2M_OK) return rc;
    const int64_t n = (int64_t)g.M * g.N;
    hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256)), dim3(256), 0, st, g.Cpart,
                       reinterpret_cast<float*>(g.C), g.M, g.N, g.ldc, g.ksplit, g.alpha, epi == TG_ACC_F32 ? 1 : 0);
    M2M_CHECK_HIP(hipGetLastError());
    return M2M_OK;
  }
  return precision == M2M_PREC_BF16 ? launch_bgemm_t<bf16_t>(epi, g, st, sw.xcd_order) : launch_bgemm_t<float>(epi, g, st, sw.xcd_order);
}

// ------------------------------------------------------------ the launches the trainer makes by name
// the grouped weight-gradient launch: the `tiles` 128 x 128 tiles of the n_probs products in the device table
int launch_dw_group(int precision, const DwProb* probs_dev, int n_probs, int tiles, hipStream_t st, const TrainSwitches& sw) {
  const bool tr_reads = sw.dw_tr;
  const int xcd_order = sw.dw_xcd;
  const int grid = xcd_order ? 8 * ceil_div(tiles, 8) : tiles;
  if (precision == M2M_PREC_BF16 && tr_reads)
    hipLaunchKernelGGL((dw_group_kernel<bf16_t, true>), dim3(grid), dim3(256), 0, st, probs_dev, n_probs, tiles, xcd_order);
  else if (precision == M2M_PREC_BF16)
    hipLaunchKernelGGL((dw_group_kernel<bf16_t, false>), dim3(grid), dim3(256), 0, st, probs_dev, n_probs, tiles, xcd_order);
  else
    hipLaunchKernelGGL((dw_group_kernel<float, false>), dim3(grid), dim3(256), 0, st, probs_dev, n_probs, tiles, xcd_order);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

// the operands of a weight gradient on the split-K bgemm route: dY [M][Ny] -> tA [Ny][Mp], X [M][Kx] -> tB [Kx][Mp]
template <typename T>
static void transpose_pair_t(const void* dY, int64_t ldy, int Ny, const void* X, int64_t ldx, int Kx, void* tA, void* tB, int M, int Mp, hipStream_t st) {
  hipLaunchKernelGGL((transpose_kernel<T, T>), dim3(ceil_div(Ny, 64), ceil_div(Mp, 64)), dim3(256), 0, st, (const T*)dY, ldy, (T*)tA, (int64_t)Mp, M, Ny, Mp);
  hipLaunchKernelGGL((transpose_kernel<T, T>), dim3(ceil_div(Kx, 64), ceil_div(Mp, 64)), dim3(256), 0, st, (const T*)X, ldx, (T*)tB, (int64_t)Mp, M, Kx, Mp);
}
int launch_transpose_pair(int precision, const void* dY, int64_t ldy, int Ny, const void* X, int64_t ldx, int Kx, void* tA, void* tB, int M, int Mp,
                          hipStream_t st) {
  if (precision == M2M_PREC_BF16) transpose_pair_t<bf16_t>(dY, ldy, Ny, X, ldx, Kx, tA, tB, M, Mp, st);
  else transpose_pair_t<float>(dY, ldy, Ny, X, ldx, Kx, tA, tB, M, Mp, st);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

// WT (null: a forward-only pass), Wc and Wil (null outside the bf16 mode) from the fp32 master P, in the mode's storage type
int launch_weights_transpose(int precision, const WtBlock* blocks_dev, int n_blocks, const float* P, void* WT, void* Wc, void* Wil, hipStream_t st) {
  if (precision == M2M_PREC_BF16)
    hipLaunchKernelGGL(weights_transpose_kernel<bf16_t>, dim3(n_blocks), dim3(256), 0, st, blocks_dev, P, (bf16_t*)WT, (bf16_t*)Wc, (bf16_t*)Wil);
  else
    hipLaunchKernelGGL(weights_transpose_kernel<float>, dim3(n_blocks), dim3(256), 0, st, blocks_dev, P, (float*)WT, (float*)Wc, (float*)Wil);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

}  // namespace m2m
