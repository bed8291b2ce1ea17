// Internal structures of the T5 encoder/decoder path (not part of the C ABI).
#pragma once

#include "common.h"
#include "env.h"

#include <vector>

namespace m2m {

constexpr int DK = 64;  // d_kv: the attention kernels are specialised for 64 (HF default the reference uses)

// ------------------------------------------------------------------ model ---
struct EncLayerPacked {
  const float* ln0;   // [d]
  const void* wqkv;   // [3*inner, d]      rows: q | k | v
  const void* wo;     // [d, inner]
  const float* ln1;   // [d]
  const void* wi;     // [2*dff, d]        64-row chunks: 32 rows of wi_0 then the matching 32 rows of wi_1
  const void* wo_ff;  // [d, dff]
};

struct DecLayerPacked {
  const float* ln0;
  const void* wqkv;   // [3*inner, d]
  const void* wo;     // [d, inner]
  const float* ln1;
  const void* wcq;    // [inner, d]
  const void* wco;    // [d, inner]
  const float* ln2;
  const void* wi;     // [2*dff, d]        16-row chunks: 8 rows of wi_0 then the matching 8 rows of wi_1
  const void* wo_ff;  // [d, dff]
  // Step-weight image of the feed-forward (repack.hip ff_image_kernel): the same elements as wi and wo_ff, in the order the loads of
  // dec_ff_body read them - hidden slice c (32 columns), wave ks (k-slice of 64), then the wave's 12 fragment loads: wf[j][s]
  // (j = 0..3, s = 0..1: elements [64 ks + 32 s + 8 g, +8) of row 64 c + 16 j + r of wi), then wo[j] (elements [32 c + 8 g, +8) of
  // row 16 (4 ks + j) + r of wo_ff).  A fragment load is 512 consecutive elements, lane 16 g + r in lane order (fp32: the lanes'
  // low halves, then their high halves); a wave's block is 6144 elements, a slice's d / 64 of them.  wi and wo_ff stay for the batched pass.
  const void* ff_img; // [dff / 32][d / 64][12][512]
  // Step images of the attention output projections (repack.hip attn_out_image_kernel), self (wo) and cross (wco): head h, then
  // load instruction u (0 .. 32 / E - 1, E = elements in 16 bytes), then thread tid < 2 d: the 16 bytes the decode attention
  // kernels' thread tid reads with its load u - row tid / 2, columns 64 h + 32 (tid & 1) + E u.  The same elements as wo / wco.
  const void* wo_img;   // [H][32 / E][2 d][E]
  const void* wco_img;  // [H][32 / E][2 d][E]
};

constexpr int FF_IMG_FRAG = 512;                 // elements of one fragment load of a wave in the feed-forward image
constexpr int FF_IMG_WAVE = 12 * FF_IMG_FRAG;    // elements of a wave's block: 8 fragments of wi, 4 of wo_ff
constexpr int64_t TOKEN_TABLES_MAX_BYTES = 16ll << 20;   // m2m_model::q0_tab / k0_tab / v0_tab: no tables beyond this (T5's own 32 128-token vocabulary: 131 MB)

}  // namespace m2m

struct m2m_model {
  m2m_t5_geometry g;
  int precision;
  int inner;            // num_heads * d_kv
  int vocab_pad;        // vocab rounded up to 16 (lm_head rows beyond vocab are zero)
  size_t esize;         // sizeof storage element (4 or 2)
  void* blob = nullptr; // one device allocation holding every packed tensor
  int64_t blob_bytes = 0;
  std::vector<m2m::EncLayerPacked> enc;
  std::vector<m2m::DecLayerPacked> dec;
  const float* enc_final_ln = nullptr;
  const float* dec_final_ln = nullptr;
  const float* shared = nullptr;     // [V, d] fp32 (feeds the fp32 residual stream)
  const void* lm_head = nullptr;     // [vocab_pad, d]
  const void* wckv = nullptr;        // [L_dec * 2 * inner, d]  per layer: ck rows then cv rows
  // Layer-0 token tables (decode.hip dec_token_tables_kernel, written once in m2m_model_create): the decoder's layer-0 input row is
  // emb[tok] and nothing else, so the head's q (fp32) and k, v (rounded to T) of that row are functions of the token id alone -
  // entry (h, tok) holds the bits the step kernel's own norm + da_project would produce.  Null when the three tables together
  // would exceed TOKEN_TABLES_MAX_BYTES or the vocabulary does not fit a 16-bit id: every step then projects as before.
  const float* q0_tab = nullptr;     // [H][V][64] fp32
  const void* k0_tab = nullptr;      // [H][V][64] T
  const void* v0_tab = nullptr;      // [H][V][64] T
  std::vector<float> enc_rel_bias_host;  // [num_buckets, H]
  std::vector<float> dec_rel_bias_host;  // [num_buckets, H]
};

namespace m2m {

// device-resident decode loop state
struct DecState {
  int t;             // position of the token being fed this step (0-based)
  int done;          // every row has emitted EOS
  int out_len;       // valid columns of the token matrix once done
  int n_unfinished;
  int max_steps;     // steps after which the loop must stop (max_length - 1)
  int overflow;      // sticky: a value outside the fixed-point residual range (|v| >= 2^21, Inf, NaN) was produced
  int t_copy;        // headless greedy loop: t of the current step, rewritten every step by the layer-0 cross kernel (the lm_head
                     // kernel, which ADVANCES t at its end, reads this stable copy instead of t itself)
  int zero;          // always 0 (cleared with the rest of the state, never written): what a "never skip" row flag points at
  int smp_unfinished;  // select and beam heads (several workgroups per step; decode.hip close_step): unfinished rows or clips summed ...
  int smp_ticket;      // ... over the step's workgroups, and workgroups done; the last one closes the step and clears both
};

// Parameters of the sampling select (decode.hip select_head: dec_sample_kernel and the sampled forms of dec_process_kernel and
// dec_scored_kernel), a device block of the session workspace: written with an async copy before every sampled call, so one
// captured graph serves every call and every seed.
struct SampleParams {
  float temperature;        // > 0; 1 = no scaling
  int top_k;                // 0 = no top-k filter
  float top_p;              // [0, 1]; 1 = no nucleus filter
  int pad_;
  unsigned long long seed;  // the call's seed: the draw of clip row r at position t hashes (seed, r, t)
};

// Logits processors (m2m_generate_processed, decode.hip dec_process_kernel): the call's parameters, a device block of the workspace
// written before the chains start (as SampleParams).  Vocabulary bitmaps hold the id lists that do not depend on the history.
constexpr int PROC_MAX_VOCAB = 4096;      // = SAMPLE_MAX_VOCAB: the row lives in one wavefront's registers
constexpr int PROC_BITS = PROC_MAX_VOCAB / 32;   // words of a vocabulary bitmap
constexpr int PROC_MAX_LEN = 2048;        // max_length: a row's history is staged in LDS as 16-bit ids
constexpr int PROC_MAX_BAD = 64;          // bad-word sequences of two or more ids (one lane each)
constexpr int PROC_MAX_BAD_IDS = 512;     // ids in those sequences together
struct ProcessParams {
  float penalty;            // repetition_penalty; 1 = off
  int ngram;                // no_repeat_ngram_size; 0 = off
  int min_length;           // EOS is banned while cur_len < min_length (0 = off)
  int min_new;              // ... and while cur_len - 1 < min_new_tokens (0 = off)
  int forced_bos;           // -1 = off
  int forced_eos;           // -1 = off
  int begin_index;          // cur_len at which begin_suppress applies (1, or 2 with forced_bos)
  int max_length;           // the call's max_length (forced EOS at cur_len == max_length - 1)
  int has_bad1, has_supp, has_begin;   // the bitmaps below are not empty
  int n_bad;                // bad-word sequences of two or more ids
  int bad_off[PROC_MAX_BAD + 1];       // sequence q is bad_ids[bad_off[q] .. bad_off[q + 1])
  int bad_ids[PROC_MAX_BAD_IDS];
  unsigned bad1[PROC_BITS];            // one-id bad words (the [eos] entry filtered out)
  unsigned supp[PROC_BITS];            // suppress_tokens
  unsigned begin[PROC_BITS];           // begin_suppress_tokens
};

// Per-token outputs of m2m_generate_scored (decode.hip dec_scored_kernel): where the call's outputs go, a device block of the workspace
// written before the chains start (as SampleParams): the captured step reads the pointers from it.
struct ScoreParams {
  float* scores;            // [steps][rows][V] the row each token was selected from, or nullptr
  float* logprobs;          // [rows][steps] log_softmax(that row)[token], or nullptr
  int rows, steps;          // the call's clips (the encoded batch) and max_length - 1
  int vec4;                 // the rows of `scores` are 16-byte aligned (V % 4 == 0, aligned base): float4 stores
  int pad_;
};

// The MIDI token grammar (m2m_generate_grammar, decode.hip grammar_*; music2midi_amd/grammar.py is the definition): the call's
// parameters, a device block of the workspace written before the chains start by EVERY call of the processed or scored head (enable
// = 0 without the grammar: one captured graph serves both), and the state of one clip, indexed by the clip (tok_row[b]), not the
// slot - live-row re-packing does not move it.  The states are zeroed on the caller's stream before the chains start: zero is the
// start state (no phase entered, every time index allowed, nothing sounding).  The processed beam head (m2m_generate_beam_processed)
// keeps one state per ROW instead (row c * nb + i: beam i of clip c) in the same region, which holds max_batch states: a clip's
// beams diverge, and dec_beam_kernel gives new beam i its parent's state advanced by its token.
constexpr int GRAM_MAX_PITCH = 128;
constexpr int GRAM_EOS = 2, GRAM_ONSET = 3, GRAM_OFFSET = 4;     // music2midi_amd/tokenizer.py
enum { GRAM_START = 0, GRAM_TIME = 1, GRAM_ONSET_OPEN = 2, GRAM_ONSET_LIST = 3, GRAM_OFFSET_OPEN = 4, GRAM_OFFSET_LIST = 5 };
struct GrammarParams {
  int enable;               // 0: the head neither reads nor writes a state
  int pitch0, time0, end;   // pitch ids [pitch0, time0), time ids [time0, end); ids from `end` upwards are never allowed
};
struct GrammarState {
  int phase;                // GRAM_*
  int next_time;            // last_time + 1: the smallest time index still allowed (0 at the start)
  int pad_[2];
  unsigned open_old[GRAM_MAX_PITCH / 32];   // sounding pitches whose onset lies before the current group
  unsigned open_new[GRAM_MAX_PITCH / 32];   // onsets of the current group
};
static_assert(sizeof(GrammarState) == 48, "one clip's grammar state: three 16-byte loads");

// Beam search (m2m_generate_beam): the call's parameters, a device block of the workspace written before the chains start (as
// SampleParams), and the per-clip / per-row state of the beam head (decode.hip dec_beam_kernel).
struct BeamParams {
  int nb;                   // beams per clip, 2..BEAM_MAX
  float lp;                 // length_penalty
  int early;                // early_stopping: 0 False, 1 True, 2 "never"
  int n;                    // num_return_sequences, 1..nb
  int max_length;
  int max_hyp_len;          // written by the finalize kernel: the longest returned hypothesis (0 before)
  int pad_[2];
};
struct BeamClip {           // BeamHypotheses of one clip
  double worst;             // worst kept score (1e9 while empty)
  int n_hyp;                // hypotheses kept (<= nb)
  int done;
  int stamp;                // hypotheses added so far (the order of BeamHypotheses.beams)
  int pad_;
};
struct BeamRow {            // row c * nb + h: running beam h of clip c, and hypothesis slot h of that clip
  double hyp_score;         // sum_logprobs / len ** length_penalty (double: HF computes it in Python floats)
  float score;              // running beam score (fp32, as HF's beam_scores)
  int hyp_len;              // tokens of the hypothesis (start token included, EOS not)
  int hyp_stamp;            // when it was added
  int pad_;
};

// The host side of the five parameter blocks: one pinned allocation of the session.  An export fills the blocks its head reads,
// decode_call copies each of those to its device block in the workspace (sample_dev, proc_dev, ...).
struct CallParams {
  SampleParams sample;
  ProcessParams proc;
  ScoreParams score;
  GrammarParams gram;       // written by decode_call from the call's block
  BeamParams beam;
};

}  // namespace m2m

namespace m2m {
// Environment switches of the encoder-side kernel families (enc_gemm.hip, enc_attn.hip), read ONCE when a session is created: they choose
// between kernels that are not all bit-identical (the two attention forms differ in the last bits), so a session keeps the forms
// it started with whatever the environment does later, and no launch reads the environment (not safe against a concurrent setenv;
// ADVICE r5).  A trainer latches its own the same way.  The public entry points of a session and of a trainer put theirs in scope
// (EncSwitchScope); launches outside any scope (tools, the single-product hooks) take the process-wide value, read once.
struct EncSwitches {
  int norm_gemm = 0;            // M2M_NORM_GEMM: 0 by size, 1 never ("0"), 2 always ("force")
  unsigned norm_gemm_skip = 0;  // "e<digits>": not for the listed epilogue ids (diagnostic)
  int resid_panel = 0;          // M2M_RESID_PANEL: as norm_gemm
  int attn_wide = 1;            // M2M_ATTN_WIDE=0: the first attention kernel in the bf16 mode as well
  int min_blocks = 160;         // M2M_NORM_GEMM_MIN_BLOCKS: row blocks from which the row-panel kernels run
  int norm_gemm_hout = 0;       // M2M_NORM_GEMM_HOUT (diagnostic)
  int norm_gemm_split = 1;      // M2M_NORM_GEMM_SPLIT=0: below min_blocks the two-kernel path instead of the column-group form (round 6)
  // the form of gemm_kernel a product takes (enc_gemm.hip gemm_small_below, gemm_dma_ns)
  int gemm_small_below = 512;   // M2M_GEMM_SMALL_BELOW: 64x64 tiles for plain products of fewer 128x128 tiles than this
  int gemm_dma = 1;             // M2M_GEMM_DMA: 1 the LDS-DMA ring by shape, 0 never ("0"), 2 always ("all")
  int gemm_dma_ns1 = 4;         // M2M_GEMM_DMA_NS1 / _NS2: ring depth of the small / the large tile
  int gemm_dma_ns2 = 3;
  int gemm_dma_mink = 512;      // M2M_GEMM_DMA_MINK: by shape, the ring from this K on ...
  int gemm_dma_maxt = 1024;     // M2M_GEMM_DMA_MAXT: ... and up to this many small tiles (64 clips: 1 566 tiles per N = 384 product, the ring costs 1 %)
};
EncSwitches read_enc_switches();
const EncSwitches& process_enc_switches();      // read at its first use, once per process
extern thread_local const EncSwitches* tl_enc_switches;
struct EncSwitchScope {
  const EncSwitches* prev;
  explicit EncSwitchScope(const EncSwitches* s) : prev(tl_enc_switches) { tl_enc_switches = s; }
  ~EncSwitchScope() { tl_enc_switches = prev; }
};
inline const EncSwitches& enc_switches_now() { return tl_enc_switches ? *tl_enc_switches : process_enc_switches(); }

// Environment switches of a session.  CONSTRUCTING one reads the environment - every member's initialiser is the one read of its
// switch - and m2m_session holds one (sw): a session latches them when it is created and keeps the kernel forms it started with
// (its graphs bake them in); m2m_session_create refuses the values outside a switch's range.
struct SessionSwitches {
  static int one_of_124(int c) { return (c == 1 || c == 2 || c == 4) ? c : 0; }
  static int zero_is_1(int c) { return c == 0 ? 1 : c; }
  EncSwitches enc = read_enc_switches();                            // the encoder-side kernel families (above)
  int attn_clips = env_int("M2M_DA_CLIPS", 0);                      // decode attention: clips per workgroup (0: by chain size)
  int attn_clips_self = one_of_124(env_int("M2M_DA_CLIPS_SELF", 0));    // (diagnostic) clips per self-attention workgroup when it should differ from the cross kernels
  int ff_rows = env_int("M2M_DEC_FF_ROWS", 0);                      // decode feed-forward: residual rows per workgroup (0: by chain size)
  int ff_slices = env_int("M2M_DEC_FF_SLICES", 0);                  // decode feed-forward: hidden slices per workgroup (0: by chain size)
  int mc_cif = zero_is_1(env_int("M2M_MC_CIF", 0));                 // multi-clip cross-attention: clips in flight (diagnostic: 2; 0 or unset: 1, the product)
  bool headless = env_on("M2M_HEADLESS");                           // 0 keeps dec_head_kernel in the greedy loop (the round-1 step: 20 kernels); default: folded away (19 kernels)
  bool finished_skip = env_on("M2M_FINISHED_SKIP");                 // 0: finished rows keep streaming their K/V (the behaviour before round 4; bench.py's ragged_eos "before" leg)
  int kv_resident_layers = env_int("M2M_KV_RESIDENT_LAYERS", -1);   // layers of cross K/V kept cache-resident when the rest streams non-temporally (-1: by a 180 MB budget)
  bool kv_resident_stagger = env_on("M2M_KV_RESIDENT_STAGGER");     // two chains: each keeps a window of its own resident (kv_layer_resident); 0: both the first layers
  int token_tables = env_int("M2M_DEC_TOKEN_TABLES", 2);            // layer-0 self-attention of the headless one-clip greedy step: 0 projects q, k, v and streams the cache; 1 takes this step's q, k, v from the model's token tables; 2 reads the cached K/V from them as well
};

constexpr int MAX_GROUPS = 8;

// A contiguous range of clips decoded as one independent chain (own step counter/stream/graph).
struct DecView {
  int b0, nb;
  DecState* state;          // device
  int ord = 0, count = 1;   // the chain's ordinal among the `count` chains of its plan (plan_groups)
};

// Does cross-K/V layer `layer` of `L` keep the default cache policy (cache-resident from step to step) when `resident` layers may
// and the rest streams non-temporally?  The first `resident` layers - except with exactly two chains (and `stagger`), where chain
// i keeps the window [i * resident, i * resident + resident) mod L: the resident bytes are the same, and no layer is streamed
// from HBM by both chains when the windows hold every layer between them.  Alone this measured equal to one window; it is what
// lets the decode loop stop draining the chains at its polls (decode.hip decode_chains_may_drift).
inline bool kv_layer_resident(int layer, int L, int resident, int ord, int count, bool stagger) {
  if (resident >= L) return true;
  if (resident <= 0) return false;
  const int first = (stagger && count == 2) ? (ord * resident) % L : 0;
  return (layer - first + L) % L < resident;
}

struct DecGroup {
  DecView view{0, 0, nullptr};
  DecState* state_host = nullptr;   // pinned
  hipStream_t stream = nullptr;
  hipEvent_t ev_done = nullptr;
  hipGraphExec_t graph_exec = nullptr;           // the graph of the current view (an entry of `graphs`)
  // captured graphs by (B, S, b0, nb, steps per graph, finished-row skip on / off, head form, beams, chain ordinal and count, token-table form) — all baked into the launches.  Re-packing the live
  // rows changes (b0, nb) several times per batch, and the next batch starts from the full views again: a small cache instead of
  // a re-capture (~1 ms per 8-step graph) at every change
  struct GraphEntry { int key[11]; hipGraph_t graph; hipGraphExec_t exec; unsigned long long used; };
  std::vector<GraphEntry> graphs;
  unsigned long long graph_clock = 0;
};
}  // namespace m2m

struct m2m_session {
  const m2m_model* m;
  int max_batch, max_enc, max_dec;
  unsigned char* ws;       // caller-owned workspace
  int64_t ws_bytes;
  // carved buffers
  float* x_enc;            // [B*S, d] fp32 residual stream
  void* h_enc;             // [B*S, d] T normalised activations
  void* qkv_enc;           // [3][B][H][S][64] T  (the V third is unused: V is written transposed)
  void* vt_enc;            // [B][H][64][Sp] T, Sp = S rounded up to 64
  void* attn_enc;          // [B*S, inner] T
  void* mid_enc;           // [B*S, dff] T
  float* enc_bias_tab;     // [H][2*max_enc-1]
  int enc_bias_far, dec_bias_far;   // AttnArgs::bias_far of the two tables (0 when the table never becomes constant inside its range)
  float* dec_bias_tab;     // [H][max_dec]
  float* dec_bias_full_tab;// [H][2*max_dec-1] the same bias by (key - query) + max_dec - 1 (batched causal pass)
  void* cross_vt;          // [B][H][64][Sp] T scratch: one layer's cross V transposed (batched pass)
  void* cross_kv;          // [L][2][B][H][S][64] T
  void* self_k;            // [L][B][H][max_dec][64] T
  void* self_v;
  void* x_dec;             // [32-row padded B, d] int64 fixed-point residual stream of the decoder (decode.hip xq_t)
  float* logits;           // [B, vocab_pad]
  int64_t* tokens;         // [B, max_dec]
  int* finished;           // [B]
  int* tok_row;            // [B] slot -> clip (row of `tokens`) of the greedy loop: identity until live rows are re-packed (decode.hip)
  unsigned long long* keys;// [B] headless greedy loop: packed (logit, vocabulary index) arg-max keys of the previous step
  m2m::DecState* states;   // device [MAX_GROUPS]
  int64_t* forced_ids;     // [B, max_dec]
  // current problem
  int B = 0, S = 0;
  m2m::SessionSwitches sw;  // every switch of the session, latched at creation
  int repacks = 0, rows_moved = 0;   // live-row re-packings / rows moved by them in the last m2m_generate_greedy / _sample
  int head_mode = 0;       // head form of the free-running decode step: 0 greedy (arg-max), 1 sampling, 2 beam, | 4 processed, | 8 scored
                           // (set for the length of a call)
  int* fin_host = nullptr;                    // pinned [max_batch]: the finished flags as of the decode loop's last poll
  m2m::CallParams* call_host = nullptr;       // pinned staging copy of the five parameter blocks; their device blocks, [1] each in the workspace:
  m2m::SampleParams* sample_dev = nullptr;
  m2m::ProcessParams* proc_dev = nullptr;
  m2m::ScoreParams* score_dev = nullptr;
  m2m::GrammarParams* gram_dev = nullptr;
  m2m::GrammarState* gram_state = nullptr;    // [max_batch] in the workspace, by clip (by row in a processed beam call)
  // beam search (m2m_generate_beam): rows = encoded clips x beam_nb; every buffer below is in the workspace
  int beam_nb = 0;                            // beams per clip during a beam call, 0 otherwise
  m2m::BeamParams* beam_dev = nullptr;        // [1]
  m2m::BeamClip* beam_clip = nullptr;         // [max_batch]
  m2m::BeamRow* beam_row = nullptr;           // [max_batch]
  unsigned char* anc = nullptr;               // [2][max_batch][max_dec] ancestries (slot within the clip of every cached position)
  int64_t* hyp_tok = nullptr;                 // [max_batch][max_dec] hypothesis snapshots
  bool encoded = false;
  // decode chains
  hipEvent_t ev_in = nullptr;
  m2m::DecGroup groups[m2m::MAX_GROUPS];
};

namespace m2m {

// -------------------------------------------------------- launch helpers ---
// encoder-side (enc_gemm.hip, enc_attn.hip, enc_kernels.hip)
enum { EPI_STORE = 0, EPI_RESID = 1, EPI_GATED = 2, EPI_HEADS = 3, EPI_STORE_F32 = 4, EPI_GATED16 = 5, EPI_GATED_TRAIN = 6, EPI_GATED_BWD = 7 };

struct GemmArgs {
  const void* A;     // [M, K] T row-major
  const void* W;     // [N, K] T row-major (HF [out, in])
  int M, N, K;
  void* out;         // EPI_STORE / EPI_GATED / EPI_HEADS: T ; EPI_RESID: float (in-place +=)
  int ldo;           // leading dimension of out (STORE/RESID/GATED)
  // EPI_HEADS: out[(which*B + b)*H + h][s][64], which = n / inner
  int Bsz, S, H, inner;
  // EPI_HEADS, optional: the projection `vt_which` (V of the encoder) is written TRANSPOSED instead,
  // vt_out[(b*H + h)*64 + d][s] with row pitch Sp, so the attention kernel stages V^T with 16-byte copies
  int vt_which;      // -1: none
  void* vt_out;
  int Sp;
  int ng;            // column tiles per group of the XCD-aware tile order (set by launch_gemm)
  // EPI_RESID extras (training path; zero = the inference behaviour out += acc):
  const float* resid;      // out = resid + acc instead of out += acc (same indexing as out)
  uint32_t drop_thresh;    // dropout on acc before the add: keep(i) * drop_scale * acc, i = row * ldo + col (common.h drop_keep)
  float drop_scale;
  uint64_t drop_key;       // the site's salt: key = splitmix64(*drop_step + drop_key) (common.h DropKey)
  const uint64_t* drop_step;
  // EPI_GATED_TRAIN (training forward of the gated feed-forward, bf16, weights row-interleaved in 32-row chunks like EPI_GATED): out
  // = mid [M][N/2] = dropout(gelu_new(a) * b) as EPI_GATED writes it, AND the gate pair itself for the backward pass,
  // ab_out [M][N] = [a | b] in the MASTER column order (column c of wi_0 at c, of wi_1 at N/2 + c); dropout via the drop_* fields
  // with element index row * (N/2) + c.  gemm_takes_gated_train() says whether a shape takes this path.
  void* ab_out;
  // EPI_GATED_BWD (training backward of the gated feed-forward, bf16, small tiles): the product is dmid = dy . Wo [M][N = d_ff]; the
  // epilogue turns each tile straight into the gate pair's gradient, out = dab [M][2N] = [dmid~ * b * gelu'(a) | dmid~ * gelu(a)]
  // (ldo = 2N) with dmid~ = dropout mask of the forward applied to bf16(dmid) and a | b read from ab_out [M][2N]; dmid itself is
  // never stored.
  // launch_norm_gemm (the product's A operand is RMSNorm(nx) over the K = d_model wide fp32 residual rows; `A` is then only the scratch the
  // two-kernel fallback normalises into): nx [M][K] fp32, nw [K] the norm weight, neps; h_out (optional) [M][K] T receives the
  // normalised rows as well (the training pass keeps them for the weight gradients).
  const float* nx;
  const float* nw;
  float neps;
  void* h_out;
};

int launch_gemm(int precision, int epi, const GemmArgs& a, hipStream_t st);
// out = epilogue(RMSNorm(a.nx; a.nw, a.neps) . W^T): one kernel in the bf16 mode (row panel normalised once into LDS and kept there for
// every column tile), rmsnorm_kernel into a.A + launch_gemm otherwise (fp32 parity mode, K beyond the LDS panel, M2M_NORM_GEMM=0).
// Epilogues: EPI_HEADS, EPI_GATED, EPI_GATED16, EPI_STORE_F32.  Bit-identical to the two-kernel path (tests/test_t5_gpu.py).
int launch_norm_gemm(int precision, int epi, const GemmArgs& a, hipStream_t st);
bool gemm_takes_gated_train(int precision, int M, int N, int K);
bool gemm_takes_gated_bwd(int precision, int M, int N, int K);
int launch_rmsnorm(int precision, const float* x, const float* w, void* out, int M, int d, float eps, hipStream_t st);
// flash attention of the encoder and of the batched (teacher-forced) decoder pass
struct AttnArgs {
  const void* Q;          // [B*H][Sq][64] T
  const void* K;          // [B*H][Sk][64] T
  const void* Vt;         // [B*H][64][Sp] T (V transposed, row pitch Sp >= Sk rounded up to the 64-key tile)
  int Sp;
  const float* bias_tab;  // [H][tab_stride] relative-position bias by (key - query) + tab_center, or nullptr (cross-attention)
  int tab_stride, tab_center;
  void* out;              // [B*Sq][H*64] T
  int B, H, Sq, Sk;
  int bias_far;           // the table is constant from (key - query) <= -bias_far down and from >= +bias_far up (T5's last bucket of
                          // either direction); 0 = not known.  attn_wide_kernel reads no table for tiles that far from their queries
};
int launch_attn(int precision, const AttnArgs& a, bool causal, hipStream_t st);
int launch_transpose_v(int precision, const void* v, void* vt, int BH, int S, int Sp, hipStream_t st);
int launch_embed_rows(const int64_t* ids, const float* table, float* x, int M, int d, int V, int pad_id, hipStream_t st);
int launch_final_norm_f32(const float* x, const float* w, float* out_f32, void* out_T, int precision, int M, int d,
                          float eps, hipStream_t st);

// repack (repack.hip)
int launch_convert(int precision, const float* src, void* dst, int64_t n, hipStream_t st);
int launch_interleave(int precision, const float* wi0, const float* wi1, void* dst, int dff, int d, int half,
                      hipStream_t st);
int launch_ff_image(int precision, const void* wi, const void* wo_ff, void* img, int dff, int d, hipStream_t st);
int launch_attn_out_image(int precision, const void* wo, void* img, int H, int d, hipStream_t st);
int launch_copy_f32(const float* src, float* dst, int64_t n, hipStream_t st);
int launch_fill_zero(void* dst, int64_t bytes, hipStream_t st);
int launch_checksum(const void* buf, int64_t bytes, unsigned long long* acc_dev, hipStream_t st);
int launch_token_tables(const m2m_model* m, hipStream_t st);   // decode.hip: fills q0_tab / k0_tab / v0_tab from shared, dec[0].ln0 and dec[0].wqkv (behind their conversions)

// decoder-side (decode.hip)
int decode_init(m2m_session* s, const DecView& v, int max_steps, bool forced, hipStream_t st);
int decode_launch_step(m2m_session* s, const DecView& v, bool forced, float* logits_out, int Ld, hipStream_t st);
int decode_launch_attn(m2m_session* s, const DecView& v, bool self, int layer, int self_len, hipStream_t st, bool headless = false,
                       bool skip_finished = false);
int decode_move_rows(m2m_session* s, const int* src, const int* dst, int n, int t, hipStream_t st);   // live-row re-packing (decode.hip)
struct KvPolicy { bool nt; int resident; };   // K/V loads non-temporal; layers of cross K/V that keep the default policy then
KvPolicy decode_kv_policy(const m2m_session* s);
bool decode_chains_may_drift(const m2m_session* s, int chains);   // the decode loop's poll look-ahead is taken only then
int decode_clear_self(m2m_session* s, const DecView& v, int t0, int t1, hipStream_t st);   // zero the self K/V positions [t0, t1) of the view's rows
int decode_finalize(m2m_session* s, const DecView& v, hipStream_t st);   // headless greedy loop: write the last token, close the chain
constexpr int HEAD_GREEDY = 0, HEAD_SAMPLE = 1, HEAD_BEAM = 2;
constexpr int HEAD_PROCESSED = 4;        // bit: logits processors before the greedy (| 0) or sampling (| HEAD_SAMPLE) select, or on the
                                         // log-probabilities of the beam head (| HEAD_BEAM: m2m_generate_beam_processed)
constexpr int HEAD_SCORED = 8;           // bit: the processed head that also writes scores / log-probabilities (always with HEAD_PROCESSED)
constexpr int BEAM_MAX = 32;             // beams per clip: one LDS list of 2 x 32 candidates per beam, ancestries in bytes
int decode_beam_init(m2m_session* s, const DecView& v, hipStream_t st);
int decode_beam_finalize(m2m_session* s, int rows, int steps, int64_t* out, float* scores, int max_length, hipStream_t st);
constexpr int SAMPLE_MAX_VOCAB = 4096;   // the select and beam heads keep a row in the registers of one wavefront (64 lanes x 64 logits)
int decode_attn_clips(const m2m_session* s, int nb);
int decode_ff_rows(const m2m_session* s, int nb);
int decode_ff_slices(const m2m_session* s, int nb);

}  // namespace m2m
