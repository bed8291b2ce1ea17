// Internal structures of the training path (train.hip and the files of kernels it drives); not part of the C ABI.
#pragma once

#include "common.h"
#include "env.h"

#include <string.h>

#include <vector>

namespace m2m {

enum { TG_STORE_T = 0, TG_STORE_F32 = 1, TG_ACC_F32 = 2, TG_RESID_F32 = 3 };

// Environment switches of the training path.  CONSTRUCTING one reads the environment — every member's initialiser is the one
// read of its switch — and that happens at two places: m2m_trainer holds one (sw), so a trainer latches them when it is created,
// keeps the kernel forms it started with (its graphs bake them in) and no pass or launch reads the environment; and the entry
// points without a trainer (the single-product test hooks) share process_train_switches().  The launchers below take the struct
// from their caller.
struct TrainSwitches {
  struct Fp8Parts { bool fwd = true, dx = true, dw = false; };
  static Fp8Parts fp8_parts(const char* p) { return p ? Fp8Parts{strstr(p, "fwd") != nullptr, strstr(p, "dx") != nullptr, strstr(p, "dw") != nullptr} : Fp8Parts{}; }
  static bool is(const char* v, const char* word) { return v && strcmp(v, word) == 0; }
  static bool starts(const char* v, char c) { return v && v[0] == c; }
  bool side = env_on("M2M_TRAIN_SIDE");                  // 0: everything on the caller's stream
  bool graph = env_on("M2M_TRAIN_GRAPH");                // 0: no graph replay, every pass issued directly
  bool graph_caller = env_on("M2M_TRAIN_GRAPH_CALLER");  // 0: an unsplit graph replays on the trainer's own stream
  bool dw_group = env_on("M2M_TRAIN_DW_GROUP");          // 0: a launch per weight gradient instead of the grouped one (bf16 / fp32 modes)
  bool tail_side = env_on("M2M_TRAIN_TAIL_SIDE");        // 0: the small reductions of the tail stay on the main stream
  Fp8Parts fp8 = fp8_parts(env_str("M2M_FP8_PARTS"));    // subset of fwd,dx,dw: which projection products run on MXFP8 (see m2m_trainer)
  int grad_fmt = is(env_str("M2M_FP8_GRAD"), "e5m2");    // element format of the gradient operands: 0 = e4m3 (default), 1 = e5m2
  bool fp8_fused_q = env_on("M2M_FP8_FUSED_Q");          // 0: activations through the separate row quantiser
  bool tuned_gemm = !env_set("M2M_TRAIN_PLAIN_GEMM");    // set (diagnostic): everything through bgemm
  int dw_kmajor = env_int("M2M_TRAIN_DW_KMAJOR", -1);    // -1 = by size, 0 / 1 = forced
  bool dw_old = env_set("M2M_TRAIN_DW_OLD");             // set: the split-K bgemm weight gradient
  bool dw_tr = env_on("M2M_DW_TR");                      // 0: the register-transposing tile of the grouped launch
  int dw_xcd = env_int("M2M_DW_XCD", 1);                 // 0: the grouped launch in plain workgroup order
  int dw_tile = env_int("M2M_DW_TILE", 0);               // 64 / 128 (diagnostic): tile of launch_dw_gemm
  int dw_wgs = env_int("M2M_DW_WGS", 512);               // workgroups launch_dw_gemm aims for
  bool gate_epi = env_on("M2M_TRAIN_GATE_EPI");          // 0: gated_fwd / gated_bwd kernel launches
  bool stripes = env_on("M2M_TRAIN_STRIPES");            // 0: no fused scores + softmax
  bool attn_head = !starts(env_str("M2M_TRAIN_ATTN"), 's');   // stripes: bf16 / fp8 attention on the stripe kernels, not the whole-head ones
  bool st_slim = env_on("M2M_ST_SLIM");                  // 0: never five stripe workgroups per CU
  bool xcd_order = env_on("M2M_XCD_ORDER");              // 0: plain grids for bgemm, the stripe kernels and the MXFP8 products
  int ah_waves = env_int("M2M_AH_WAVES", 0);             // 1..4: waves per whole-head attention workgroup (0: by size)
  int ah_split = env_int("M2M_AH_SPLIT", 0);             // 1..3: waves per query block of the forward kernel (0: two)
};
inline const TrainSwitches& process_train_switches() { static const TrainSwitches sw; return sw; }      // read at its first use, once per process

// C[z][M,N] (op)= alpha * A[z][M,K] . B[z][N,K]^T ; z = (b1, b2)
struct BGemmArgs {
  const void* A;
  const void* B;
  void* C;
  const float* R;          // TG_RESID_F32: C = R + acc (same indexing as C)
  int M, N, K;
  int64_t lda, ldb, ldc;   // elements between consecutive rows AS STORED
  int a_kmajor, b_kmajor;  // 0: element (m, k) at [m*ld + k]; 1: at [k*ld + m]
  int nb1, nb2;
  int64_t sA1, sA2, sB1, sB2, sC1, sC2;
  float alpha;
  // split-K (nb1 == nb2 == 1 only): blockIdx.z takes k in [z*kchunk, (z+1)*kchunk); partial tiles go to Cpart[z][M][N]
  // (fp32) and splitk_reduce sums them into C in a fixed order.  ksplit <= 1: off.
  int ksplit, kchunk;
  float* Cpart;
  // TG_RESID_F32 only: dropout on the product before the residual add, C = R + keep(i) * drop_scale * acc  (drop_thresh == 0: off)
  uint32_t drop_thresh;
  float drop_scale;
  uint64_t drop_key;           // the site's salt: key = splitmix64(*drop_step + drop_key) (common.h DropKey)
  const uint64_t* drop_step;
  // pair mode (A2 != null): a SECOND product of the same shape in the same launch (blockIdx.z >= nb1*nb2): same strides for A and
  // C, its own B layout — dV = P~^T dO and dK = dS^T Q of an attention layer are one launch
  const void *A2, *B2;
  // XCD-contiguous workgroup order (set by launch_bgemm): 1-D launch of xcd_total = nx * ny * nz logical workgroups; 0: plain 3-D grid
  int xcd_total, xcd_nx, xcd_ny;
  void* C2;
  int64_t ldb2, sB1_2, sB2_2;
};


int launch_bgemm(int precision, int epi, const BGemmArgs& g, hipStream_t st, const TrainSwitches& sw);
constexpr int TG_BM = 64, TG_BN = 64;      // launch_bgemm's output tile
constexpr int TG_BK_MAX = 128;             // ... and a bound of the k it stages per step: a split-K kchunk is a multiple of it

// Weight gradient (train_gemm.hip): C[N1, N2] (fp32) = A[K, N1]^T . B[K, N2], the reduction index as the row of both operands
struct DwGemmArgs {
  const void *A, *B;
  float* C;
  float* Cpart;
  int N1, N2, K;
  int64_t lda, ldb, ldc;
  int ksplit, kchunk;
  int accum;             // 1: C += A^T . B (gradient accumulation; never set on a k-slice's partial tile)
};
int launch_dw_gemm(int precision, const void* A, int64_t lda, int N1, const void* B, int64_t ldb, int N2, int K, float* C, int64_t ldc,
                   float* kpart, int64_t kpart_floats, hipStream_t st, int accumulate, const TrainSwitches& sw);
// ... and every weight gradient of a step as ONE launch over a device table of them, 128 x 128 tiles numbered through the table
struct DwProb {
  DwGemmArgs g;
  int tile0, tn2;          // first tile of this problem in the launch; tiles along N2
};
int launch_dw_group(int precision, const DwProb* probs_dev, int n_probs, int tiles, hipStream_t st, const TrainSwitches& sw);
// dY [M][Ny] -> tA [Ny][Mp], X [M][Kx] -> tB [Kx][Mp] (columns [M, Mp) zeroed): the operands of a weight gradient on the split-K bgemm route
int launch_transpose_pair(int precision, const void* dY, int64_t ldy, int Ny, const void* X, int64_t ldx, int Kx, void* tA, void* tB, int M, int Mp,
                          hipStream_t st);
// all weight matrices of the model in one launch (weights_transpose_kernel, train_gemm.hip), from a table of 64 x 64 tiles
struct WtBlock { int64_t off; int N, K, tn, tk; int il_half; };     // il_half > 0: a gate pair [wi_0 | wi_1], il_half = d_ff rows each
int launch_weights_transpose(int precision, const WtBlock* blocks_dev, int n_blocks, const float* P, void* WT, void* Wc, void* Wil, hipStream_t st);

__device__ inline uint32_t u4_get(const uint4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
// Column j of an E x E block held as E 16-byte rows (E = 8 bf16 / 4 fp32), as one 16-byte row of the transposed block.
// bf16: halves (2d, 2d+1) of dword j/2 through v_perm_b32; fp32: register renaming.  (The k-major staging of train_gemm.hip and
// kv_transpose_kernel of train.hip.)
template <typename T, int E>
__device__ inline uint4 tr_col(const uint4 (&rg)[E], int j) {
  if constexpr (sizeof(T) == 2) {
    const uint32_t sel = (j & 1) ? 0x07060302u : 0x05040100u;
    return make_uint4(__builtin_amdgcn_perm(u4_get(rg[1], j >> 1), u4_get(rg[0], j >> 1), sel),
                      __builtin_amdgcn_perm(u4_get(rg[3], j >> 1), u4_get(rg[2], j >> 1), sel),
                      __builtin_amdgcn_perm(u4_get(rg[5], j >> 1), u4_get(rg[4], j >> 1), sel),
                      __builtin_amdgcn_perm(u4_get(rg[7], j >> 1), u4_get(rg[6], j >> 1), sel));
  } else {
    return make_uint4(u4_get(rg[0], j), u4_get(rg[1], j), u4_get(rg[2], j), u4_get(rg[3], j));
  }
}

// MXFP8 product (mx8.hip): C[M,N] (epi)= A[M,K] . B[N,K]^T, block-scaled fp8 operands (32 elements along K per E8M0 scale)
struct MxGemmArgs {
  const uint8_t *A, *B;      // fp8 bytes, [M][lda] / [N][ldb]; lda, ldb multiples of 128, zero-padded past K
  const uint8_t *sA, *sB;    // E8M0 scales, [M][lda/32] / [N][ldb/32]
  void* C;
  const float* R;            // TG_RESID_F32
  int M, N, K;
  int64_t lda, ldb, ldc;
  int ksplit, kchunk;
  float* Cpart;
  uint32_t drop_thresh;
  float drop_scale;
  uint64_t drop_key;           // salt, as in BGemmArgs
  const uint64_t* drop_step;
  // launch_mxgemm_q: A is given as bf16 [M][ld_src] (columns >= Kvalid count as zero) and quantised while it is staged
  const void* Asrc;
  int64_t ld_src;
  int Kvalid;
  // XCD-contiguous workgroup order (set by the launchers of the _q / _p kernels): 1-D launch of xcd_total = nx * ny logical
  // workgroups, column tile fastest, so the column tiles of a row block share its rows in ONE XCD's L2; 0: plain 2-D grid
  int xcd_total, xcd_nx;
};
int launch_mxgemm(int fmt_a, int fmt_b, int epi, const MxGemmArgs& g, hipStream_t st, const TrainSwitches& sw);      // fmt: 0 = e4m3, 1 = e5m2
int launch_mxgemm_q(int fmt_a, int epi, const MxGemmArgs& g, hipStream_t st, const TrainSwitches& sw);               // A quantised in the product's own staging
int launch_mxq_rows(int src_kind, const void* src, int64_t ld_s, uint8_t* q, uint8_t* sc, int R, int C, int Cp, int fmt, hipStream_t st);
int launch_mxq_cols(int src_kind, const void* src, int64_t ld_s, uint8_t* qt, uint8_t* sc, int R, int C, int Rp, int fmt, hipStream_t st);

// fp8 mode: the MXFP8 images of one projection matrix W [N][K] (fp32 master at parameter offset `off`), as byte offsets into the
// trainer's w8 buffer: q [N][K] + qs [N][K/32] with blocks along K (the forward's B operand), qt [K][Np] + qts [K][Np/32] with
// blocks along N (the B operand of dX = dY . W); Np = align_up(N, 128).  mxq_weights_kernel (train_gemm.hip) writes all four from a
// table of 32 x 64 tiles.  w8_add_matrix is the per-matrix part of the table builder: it places the four images behind
// `w8_bytes` (advancing it, 256-byte aligned) and appends the matrix's tiles.
struct W8Lin { int64_t off; int N, K, Np; int64_t q, qs, qt, qts; };
struct W8Tile { int64_t off; int N, K, Np; int64_t q, qs, qt, qts; int tn, tk; };
W8Lin w8_add_matrix(int64_t off, int N, int K, int64_t& w8_bytes, std::vector<W8Tile>& tiles);
int launch_mxq_weights(const W8Tile* tiles_dev, int n_tiles, const float* P, uint8_t* w8, hipStream_t st);

// The three MXFP8 routes of the fp8 step (mx8.hip), called by Ops::mm / dX / dW_on (train.hip) and by the single-product test
// hook m2m_mx8_step_product: the step and the hook run the same lines.  bf16 operands; fused quantisation and the gradient
// element format come from sw (fp8_fused_q, grad_fmt).
struct MxDrop { uint32_t thresh; float scale; uint64_t key; const uint64_t* step; };      // the dropout fields of MxGemmArgs (thresh == 0: off)
// Y[M,N] (epi)= X[M,K] . W^T: X bf16 [M][ldx], the weight's row image wq / wqs ([N][K]); q8a / s8a: scratch for X's fp8 image
// ([M][K] + [M][K/32]; untouched when X is quantised in the product's staging)
int mx8_fwd(int epi, const void* X, int64_t ldx, const uint8_t* wq, const uint8_t* wqs, uint8_t* q8a, uint8_t* s8a, void* C, int64_t ldc, const float* R,
            int M, int N, int K, const MxDrop& drop, const TrainSwitches& sw, hipStream_t st);
// dX[M,Kw] (epi)= dY[M,Nw] . W: dY bf16 [M][ldy], the weight's transposed image wqt / wqts ([Kw][Np]); scratch [M][Np] + [M][Np/32]
int mx8_dx(int epi, const void* dY, int64_t ldy, int Nw, int Kw, const uint8_t* wqt, const uint8_t* wqts, int Np, uint8_t* q8a, uint8_t* s8a, void* C,
           int64_t ldc, const float* R, int M, const MxDrop& drop, const TrainSwitches& sw, hipStream_t st);
// G[Ny,Kx] (+)= dY[M,Ny]^T . X[M,Kx]: both operands through the transposing quantiser (scratch q8ta [Ny][Mp] / q8tb [Kx][Mp],
// Mp = align_up(M, 128), + scales), then a product over the M rows split over k while that fills the chip and kpart
// (kpart_floats floats) holds the slices.  used_ksplit / used_kchunk (optional): what the policy chose.
int mx8_dw(const void* dY, int64_t ldy, int Ny, const void* X, int64_t ldx, int Kx, uint8_t* q8ta, uint8_t* s8ta, uint8_t* q8tb, uint8_t* s8tb, float* kpart,
           int64_t kpart_floats, float* G, int accumulate, int M, const TrainSwitches& sw, hipStream_t st, int* used_ksplit = nullptr,
           int* used_kchunk = nullptr);

// one 64-bit word on the device holding the dropout step key of a test call (the single-kernel test hooks of the C ABI)
struct StepWord {
  uint64_t* dev = nullptr;
  uint64_t last = 0;
  int set(uint64_t v, hipStream_t st) {
    if (dev && v == last) return M2M_OK;                    // (repeated calls with one key — tools/attn_head_bench.py — stay asynchronous)
    if (!dev) M2M_CHECK_HIP(hipMalloc((void**)&dev, 8));
    M2M_CHECK_HIP(hipStreamSynchronize(st));
    M2M_CHECK_HIP(hipMemcpyAsync(dev, &v, 8, hipMemcpyHostToDevice, st));
    M2M_CHECK_HIP(hipStreamSynchronize(st));
    last = v;
    return M2M_OK;
  }
};

// Whole-head attention of the training step (attn_train.hip): forward with the row log-sum-exp, two-pass backward
struct HeadAttnArgs {
  // (position, d) of clip b, head h at ptr + b * sXb + h * 64 + position * ldx   (bf16 storage)
  const bf16_t *Q, *K, *V;
  int64_t ldq, ldk, ldv, sQb, sKb, sVb;
  bf16_t* O;                   // forward out, backward in
  int64_t ldo, sOb;
  float* lse;                  // [B*H][Sq]: forward out, backward in
  const bf16_t* dO;            // backward in (layout of O)
  bf16_t *dQ, *dK, *dV;        // backward out
  int64_t lddq, lddk, lddv, sdQb, sdKb, sdVb;
  const float* bias_tab;       // [H][tab_stride] by (key - query + tab_center), or null
  int tab_stride, tab_center;
  float* diag_part;            // backward, self-attention with bias: [B*H][ceil(Sq/32)][Sk + 31] diagonal sums of dS, or null
  int H, Sq, Sk, causal, ldp;  // ldp: row pitch of the dropout element index (round-up-8 of Sk, as the stored P had)
  DropKey dk;
  uint32_t thresh;
  float scale;
  int key_split;               // forward: waves per query block (set by the launcher)
  uint32_t* keep_bits;         // with dropout: [B*H][ceil(Sk/32)][round_up_32(Sq)] words, bit k of word (key block j, query q) = probability (q, 32 j + k)
                               // is kept.  The forward pass hashes once and writes them; both backward orientations read them instead of hashing again.
};
constexpr int AH_MAX_S = 288;  // rows an LDS image holds (9 blocks of 32): 36 KB per [S, 64] bf16 operand, two images + tables per workgroup, two workgroups per CU
int launch_attn_head_fwd(const HeadAttnArgs& a, int nB, hipStream_t st, const TrainSwitches& sw);
int launch_attn_head_bwd(const HeadAttnArgs& a, int nB, hipStream_t st, const TrainSwitches& sw);

// Adafactor plan (device tables built once per trainer; kernels and launcher: adafactor.hip)
constexpr int AF_ROWS = 16;      // rows of a matrix per block (32 until round 3: 235 registers in pass A, two blocks per CU; 16 rows run pass A / B / C in
                                 // 51 / 23 / 61 us instead of 64 / 31 / 69; 8 rows gain nothing more and cost pass A2 its partial sums)
struct AfTensor {
  int64_t offset;          // into the flat parameter / gradient buffers
  int rows, cols;          // vectors: rows = 1
  int row_off;             // into rowsum / rfac
  int cfac_off;            // into cfac
  int64_t col_off;         // into colpart (nblocks * cols floats)
  int64_t state_off;       // into the optimizer state (matrix: R[rows] | C[cols]; vector: V[cols])
  int block0, nblocks;
};
struct AfBlock {
  int tensor, row0;
  int64_t col_off;
};
struct AfPlan {
  int n_tensors = 0, n_blocks = 0;
  AfTensor* tensors = nullptr;
  AfBlock* blocks = nullptr;
  float *rowsum = nullptr, *colpart = nullptr, *blk_a = nullptr, *blk_b = nullptr, *state = nullptr, *rfac = nullptr,
        *cfac = nullptr, *tstat = nullptr;
  int64_t state_floats = 0;
  // gradient clipping (grad_clip.hip): per-block sums of g^2, and the norm words — [0] total norm, [1] coef of the last step in
  // norm mode; [2], [3] the same two of the last m2m_trainer_grad_norm call
  float *blk_g = nullptr, *gn_words = nullptr;
};
// Gradient clipping folded into the step (Lightning's Trainer(gradient_clip_val, gradient_clip_algorithm); music2midi_amd/clipping.py)
enum { AF_CLIP_OFF = 0, AF_CLIP_NORM = 1, AF_CLIP_VALUE = 2 };
// clip AF_CLIP_NORM: passes A, B and C read g * *coef_dev (the word launch_grad_norm wrote);  AF_CLIP_VALUE: g clamped to +-clip_value
int launch_adafactor(const AfPlan& pl, float* P, const float* G, int step, hipStream_t st, int clip = AF_CLIP_OFF,
                     const float* coef_dev = nullptr, float clip_value = 0.f);
// global 2-norm of G as torch.nn.utils.clip_grad_norm_ takes it (the norm of the per-tensor norms) -> words[0], and
// coef = min(1, max_norm / (norm + 1e-6)) -> words[1].  Two launches, no atomics, every sum in a fixed order.
int launch_grad_norm(const AfPlan& pl, const float* G, float max_norm, float* words, hipStream_t st);

}  // namespace m2m
