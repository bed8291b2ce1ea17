// Frame-level piano-roll scoring for gfx950: decoded notes against label notes -> the true-positive / false-negative / false-positive
// cells of the two piano rolls at 100 frames per second, as counts (per confidence threshold) and as notes, on the device.
// The definition is music2midi_amd/frame_metrics.py (error_rolls, frame_counts, roll_to_notes: ref music2midi/plot_midi.py:19-135
// restated); every integer here is EQUAL to its.  The frame arithmetic is score_frames.h, the one score.hip uses.
//
// A roll is bit-packed, pitch-major: one bit per frame, row p word w holds frames [32 w, 32 w + 32) of pitch p.  A note's range is a
// few LDS atomicOr's of word masks, a count is a popcount, a falling edge is x & ~(x >> 1 | next << 31).
//
//   counts  m2m_score_frame_counts, grid (frame tiles, timelines), one launch for every threshold.  A workgroup finds n_frames of
//           the labels and of the whole output, builds the label roll of its tile once (and its 12-row melody roll: the pitch
//           class of the highest sounding pitch, found by walking the pitches from 127 down with a `seen` mask, one lane per word),
//           then for every threshold k: n_frames under k (labels and the output notes kept under k - the cut at n_frames - 1 moves
//           with it), the output roll of the kept notes, the popcounts of ref & est, ref & ~est, ~ref & est of the full and of the
//           melody roll.  One integer atomic per count, workgroup and threshold.
//   notes   m2m_score_error_notes, one threshold, full or melody roll.  fr_rolls_kernel (same grid) builds both rolls of its tile
//           plus one halo word, writes the three error rolls to the workspace and the number of falling edges of the tile;
//           fr_notes_kernel turns the falling edges into notes in the definition's order (ascending end frame, then pitch): lane i
//           owns four frames, counts their edges over the rows, a block scan plus the earlier tiles' totals give every edge its
//           slot, and the edge finds its start by walking back along its row in the workspace (across tiles: a run is one note).
//
// Everything runs on the caller's stream; the workspace and the outputs are the caller's.
#include "common.h"
#include "score_frames.h"

#include <math.h>

namespace m2m {
namespace {

#pragma clang fp contract(off)

constexpr int FR_THREADS = 256;
constexpr int FR_TILE = M2M_SCORE_FRAME_TILE;   // frames of one timeline per workgroup
constexpr int FR_W = FR_TILE / 32;              // words per row of a tile
constexpr int FR_WH = FR_W + 1;                 // ... with the halo word of the notes path
constexpr int FR_ROWS = 128;
static_assert(FR_TILE == 4 * FR_THREADS, "fr_notes_kernel: every lane owns four frames of the tile");

struct FrArgs {
  const int32_t* notes;      // [R][L][3]
  const int32_t* counts;     // [R]
  const float* note_lp;      // [R][L][2] or null
  const double* lab;         // [3][n_labels]: start, end, pitch
  const int32_t* lab_off;    // [T + 1]
  const float* thr;          // [K] (counts path) or null
  float thr0;                // the one threshold of the notes path
  int R, L, sequential, n_labels, frame_cap, K;
  double time_step;
};

// a timeline's share of the inputs
struct FrSpan { int r0, r1, l0, l1; };
__device__ inline FrSpan fr_span(const FrArgs& a, int t) {
  FrSpan s;
  s.r0 = a.sequential ? 0 : t;
  s.r1 = a.sequential ? a.R : t + 1;
  s.l0 = min(max(a.lab_off[t], 0), a.n_labels);
  s.l1 = min(max(a.lab_off[t + 1], s.l0), a.n_labels);
  return s;
}

// kept under the threshold: dropped iff on + off < thr is true in float32 (note_match.hip's add and comparison; a NaN total is kept)
__device__ inline bool fr_kept(const float* note_lp, int64_t n, bool masked, float thr) {
  return !(masked && note_lp[n * 2 + 0] + note_lp[n * 2 + 1] < thr);
}

// bits [b0, b1) of a row, b0 < b1
__device__ inline void fr_set(uint32_t* row, int b0, int b1) {
  const int w0 = b0 >> 5, w1 = (b1 - 1) >> 5;
  for (int w = w0; w <= w1; ++w) {
    uint32_t m = 0xFFFFFFFFu;
    if (w == w0) m &= 0xFFFFFFFFu << (b0 & 31);
    if (w == w1) m &= 0xFFFFFFFFu >> (31 - ((b1 - 1) & 31));
    atomicOr(&row[w], m);
  }
}

// this thread's share of max(n_frames) over the label notes (end > start)
__device__ inline int fr_label_frames(const FrArgs& a, const FrSpan& s, int tid) {
  const double* ls = a.lab;
  const double* le = a.lab + a.n_labels;
  int m = 0;
  for (int i = s.l0 + tid; i < s.l1; i += FR_THREADS)
    if (le[i] > ls[i]) m = max(m, sc_count_capped(le[i], a.frame_cap));
  return m;
}

// this thread's share of the largest offset index over the output notes kept under thr, -1 = none (frames are monotone in it)
__device__ inline int fr_output_end(const FrArgs& a, const FrSpan& s, int tid, bool masked, float thr) {
  int m = -1;
  for (int r = s.r0; r < s.r1; ++r) {
    const int c = min(a.counts[r], a.L);    // a row with an id outside the vocabulary (-1) has no notes; the caller raises for it
    const int32_t* nr = a.notes + (int64_t)r * a.L * 3;
    for (int n = tid; n < c; n += FR_THREADS)
      if (fr_kept(a.note_lp, (int64_t)r * a.L + n, masked, thr)) m = max(m, nr[n * 3 + 1]);
  }
  return m;
}

__device__ inline int fr_frames_of_index(int end_idx, const FrArgs& a) {
  return end_idx < 0 ? 0 : sc_count_capped(sc_seconds(end_idx, a.time_step), a.frame_cap);
}

// the label notes into rows of S words: frames [f0, f1) only, bit 0 = frame f0
template <int S>
__device__ inline void fr_fill_labels(uint32_t* roll, const FrArgs& a, const FrSpan& s, int tid, int f0, int f1) {
  const double* ls = a.lab;
  const double* le = a.lab + a.n_labels;
  const double* lp = a.lab + 2 * (int64_t)a.n_labels;
  for (int i = s.l0 + tid; i < s.l1; i += FR_THREADS) {
    const double b = ls[i], e = le[i];
    if (!(e > b)) continue;
    const int lo = max(sc_pos_capped(b, a.frame_cap), f0), hi = min(sc_pos_capped(e, a.frame_cap), f1);
    const int p = (int)lp[i];
    if (lo < hi && (unsigned)p < (unsigned)FR_ROWS) fr_set(roll + p * S, lo - f0, hi - f0);
  }
}

template <int S>
__device__ inline void fr_fill_output(uint32_t* roll, const FrArgs& a, const FrSpan& s, int tid, int f0, int f1, bool masked, float thr) {
  for (int r = s.r0; r < s.r1; ++r) {
    const int c = min(a.counts[r], a.L);
    const int32_t* nr = a.notes + (int64_t)r * a.L * 3;
    for (int n = tid; n < c; n += FR_THREADS) {
      if (!fr_kept(a.note_lp, (int64_t)r * a.L + n, masked, thr)) continue;
      const int lo = max(sc_pos_capped(sc_seconds(nr[n * 3 + 0], a.time_step), a.frame_cap), f0);
      const int hi = min(sc_pos_capped(sc_seconds(nr[n * 3 + 1], a.time_step), a.frame_cap), f1);
      const int p = nr[n * 3 + 2];
      if (lo < hi && (unsigned)p < (unsigned)FR_ROWS) fr_set(roll + p * S, lo - f0, hi - f0);
    }
  }
}

// word w of the 12 melody rows of a roll: in every frame where anything sounds, the row (highest pitch % 12)
template <int S>
__device__ inline void fr_melody_word(const uint32_t* roll, int w, uint32_t mel[12]) {
#pragma unroll
  for (int j = 0; j < 12; ++j) mel[j] = 0;
  uint32_t seen = 0;
  for (int base = 120; base >= 0; base -= 12) {   // base % 12 == 0: pitch base + j has class j
#pragma unroll
    for (int j = 11; j >= 0; --j) {
      if (base + j < FR_ROWS) {
        const uint32_t x = roll[(base + j) * S + w];
        mel[j] |= x & ~seen;
        seen |= x;
      }
    }
  }
}

// the bits of word w (of a tile that starts at frame f0) that lie below frame `last`
__device__ inline uint32_t fr_valid(int f0, int w, int last) {
  const int n = last - f0 - 32 * w;
  return n >= 32 ? 0xFFFFFFFFu : n <= 0 ? 0u : (1u << n) - 1u;
}

__device__ inline void fr_zero(uint32_t* p, int n, int tid) {
  for (int i = tid; i < n; i += FR_THREADS) p[i] = 0;
}

// ------------------------------------------------------------------------------------------------------------------ counts
__global__ __launch_bounds__(FR_THREADS) void fr_counts_kernel(FrArgs a, int32_t* __restrict__ out, int32_t* __restrict__ frames) {
  __shared__ uint32_t lab[FR_ROWS * FR_W];        // 16 KiB
  __shared__ uint32_t est[FR_ROWS * FR_W];        // 16 KiB
  __shared__ uint32_t mel_lab[12 * FR_W];         // the melody roll of the labels: 1.5 KiB
  __shared__ int s_nf_lab, s_end, s_cnt[6];
  const int t = blockIdx.y, tid = threadIdx.x;
  const int tile0 = blockIdx.x * FR_TILE;
  const FrSpan s = fr_span(a, t);
  const bool masked = a.note_lp != nullptr && a.thr != nullptr;

  if (tid == 0) { s_nf_lab = 0; s_end = -1; }
  if (tid < 6) s_cnt[tid] = 0;
  fr_zero(lab, FR_ROWS * FR_W, tid);
  __syncthreads();
  {
    const int m = fr_label_frames(a, s, tid), e = fr_output_end(a, s, tid, false, 0.0f);
    if (m > 0) atomicMax(&s_nf_lab, m);
    if (e >= 0) atomicMax(&s_end, e);
  }
  __syncthreads();
  const int nf_lab = s_nf_lab;
  const int nf_all = max(nf_lab, fr_frames_of_index(s_end, a));   // n_frames with every output note kept: the largest of all k
  if (nf_all > a.frame_cap) {                 // a timeline longer than the caller sized the grid for: no counts, frames = -1
    if (blockIdx.x == 0 && tid == 0) frames[t] = -1;
    return;
  }
  if (blockIdx.x == 0 && tid == 0) frames[t] = nf_all;
  const int last_all = nf_all - 1;            // frames [0, n_frames - 1) are compared; the roll's last frame stays silent
  if (tile0 >= last_all) return;              // uniform
  fr_fill_labels<FR_W>(lab, a, s, tid, tile0, min(tile0 + FR_TILE, last_all));
  __syncthreads();
  if (tid < FR_W) {
    uint32_t m[12];
    fr_melody_word<FR_W>(lab, tid, m);
#pragma unroll
    for (int j = 0; j < 12; ++j) mel_lab[j * FR_W + tid] = m[j];
  }

  for (int k = 0; k < a.K; ++k) {
    const float thr = masked ? a.thr[k] : 0.0f;
    if (tid == 0) s_end = -1;
    fr_zero(est, FR_ROWS * FR_W, tid);
    __syncthreads();
    if (masked) {
      const int e = fr_output_end(a, s, tid, true, thr);
      if (e >= 0) atomicMax(&s_end, e);
    }
    __syncthreads();
    const int nf_k = masked ? max(nf_lab, fr_frames_of_index(s_end, a)) : nf_all;
    const int last = nf_k - 1;
    if (tile0 < last) fr_fill_output<FR_W>(est, a, s, tid, tile0, min(tile0 + FR_TILE, last), masked, thr);
    __syncthreads();
    int c[6] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < FR_ROWS * FR_W; i += FR_THREADS) {
      const uint32_t l = lab[i] & fr_valid(tile0, i % FR_W, last), e = est[i];
      c[0] += __popc(l & e);
      c[1] += __popc(l & ~e);
      c[2] += __popc(~l & e);
    }
    if (tid < FR_W) {
      uint32_t m[12];
      fr_melody_word<FR_W>(est, tid, m);
      const uint32_t v = fr_valid(tile0, tid, last);
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        const uint32_t l = mel_lab[j * FR_W + tid] & v, e = m[j];
        c[3] += __popc(l & e);
        c[4] += __popc(l & ~e);
        c[5] += __popc(~l & e);
      }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j)
      if (c[j]) atomicAdd(&s_cnt[j], c[j]);
    __syncthreads();
    if (tid < 6) {
      if (s_cnt[tid]) atomicAdd(&out[((int64_t)t * a.K + k) * 6 + tid], s_cnt[tid]);
      s_cnt[tid] = 0;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------ notes
struct FrRolls {
  int melody, rows, tiles, row_words;   // rows: 128 or 12; row_words = tiles * FR_W
  int max_labels;                       // the caller's bound on the label notes of one timeline (it sizes `cap`)
  int32_t* flags;                       // [T]: n_frames, or -1 for a timeline beyond frame_cap or max_labels
  int32_t* tile_edges;                  // [T][3][tiles]: falling edges of every tile
  uint32_t* rolls;                      // [T][3][rows][row_words]: tp, fn, fp
};

__device__ inline uint32_t fr_kind(int q, uint32_t l, uint32_t e) { return q == 0 ? (l & e) : q == 1 ? (l & ~e) : (~l & e); }

__global__ __launch_bounds__(FR_THREADS) void fr_rolls_kernel(FrArgs a, FrRolls g) {
  __shared__ uint32_t lab[FR_ROWS * FR_WH];       // 16.5 KiB
  __shared__ uint32_t est[FR_ROWS * FR_WH];
  __shared__ uint32_t mel[2][12 * FR_WH];
  __shared__ int s_nf, s_end, s_edges[3];
  const int t = blockIdx.y, tid = threadIdx.x;
  const int tile0 = blockIdx.x * FR_TILE;
  const FrSpan s = fr_span(a, t);
  const bool masked = a.note_lp != nullptr;

  if (tid == 0) { s_nf = 0; s_end = -1; }
  if (tid < 3) s_edges[tid] = 0;
  fr_zero(lab, FR_ROWS * FR_WH, tid);
  fr_zero(est, FR_ROWS * FR_WH, tid);
  __syncthreads();
  {
    const int m = fr_label_frames(a, s, tid), e = fr_output_end(a, s, tid, masked, a.thr0);
    if (m > 0) atomicMax(&s_nf, m);
    if (e >= 0) atomicMax(&s_end, e);
  }
  __syncthreads();
  const int nf = max(s_nf, fr_frames_of_index(s_end, a));
  const bool refused = nf > a.frame_cap || s.l1 - s.l0 > g.max_labels;
  if (blockIdx.x == 0 && tid == 0) g.flags[t] = refused ? -1 : nf;
  if (refused) return;                        // uniform, and the same in every workgroup of the timeline
  const int last = nf - 1;
  const int f1 = min(tile0 + FR_WH * 32, last);   // the tile and its halo word
  if (tile0 < f1) {
    fr_fill_labels<FR_WH>(lab, a, s, tid, tile0, f1);
    fr_fill_output<FR_WH>(est, a, s, tid, tile0, f1, masked, a.thr0);
  }
  __syncthreads();
  const uint32_t* src_l = lab;
  const uint32_t* src_e = est;
  if (g.melody) {
    if (tid < 2 * FR_WH) {
      const int side = tid / FR_WH, w = tid % FR_WH;
      uint32_t m[12];
      fr_melody_word<FR_WH>(side ? est : lab, w, m);
#pragma unroll
      for (int j = 0; j < 12; ++j) mel[side][j * FR_WH + w] = m[j];
    }
    __syncthreads();
    src_l = mel[0];
    src_e = mel[1];
  }
  int edges[3] = {0, 0, 0};
  for (int i = tid; i < g.rows * FR_W; i += FR_THREADS) {
    const int p = i / FR_W, w = i % FR_W;
    const uint32_t l = src_l[p * FR_WH + w], e = src_e[p * FR_WH + w], ln = src_l[p * FR_WH + w + 1], en = src_e[p * FR_WH + w + 1];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const uint32_t x = fr_kind(q, l, e), nx = fr_kind(q, ln, en);
      g.rolls[(((int64_t)t * 3 + q) * g.rows + p) * g.row_words + blockIdx.x * FR_W + w] = x;
      edges[q] += __popc(x & ~((x >> 1) | (nx << 31)));
    }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q)
    if (edges[q]) atomicAdd(&s_edges[q], edges[q]);
  __syncthreads();
  if (tid < 3) g.tile_edges[((int64_t)t * 3 + tid) * g.tiles + blockIdx.x] = s_edges[tid];
}

__global__ __launch_bounds__(FR_THREADS) void fr_notes_kernel(FrRolls g, int cap, int32_t* __restrict__ notes, int32_t* __restrict__ counts) {
  __shared__ uint32_t edge[FR_ROWS * FR_W];       // the falling edges of one kind of the tile
  __shared__ int scan[FR_THREADS];
  __shared__ int s_before[3], s_total[3];
  const int t = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  if (g.flags[t] < 0) {                           // uniform
    if (tile == 0 && tid < 3) counts[t * 3 + tid] = -1;
    return;
  }
  const int32_t* te = g.tile_edges + (int64_t)t * 3 * g.tiles;
  if (tile != 0 && te[tile] == 0 && te[g.tiles + tile] == 0 && te[2 * g.tiles + tile] == 0) return;   // uniform: nothing ends here
  if (tid < 3) { s_before[tid] = 0; s_total[tid] = 0; }
  __syncthreads();
  for (int q = 0; q < 3; ++q) {
    int before = 0, total = 0;
    for (int i = tid; i < g.tiles; i += FR_THREADS) {
      const int v = te[q * g.tiles + i];
      total += v;
      if (i < tile) before += v;
    }
    if (before) atomicAdd(&s_before[q], before);
    if (total) atomicAdd(&s_total[q], total);
  }
  __syncthreads();
  // cap bounds the runs by construction; a total beyond it would be a broken bound: -1 and nothing written
  if (tile == 0 && tid < 3) counts[t * 3 + tid] = s_total[tid] <= cap ? s_total[tid] : -1;

  const int w = tid >> 3, b0 = (tid & 7) * 4;     // this lane's four frames: bits [b0, b0 + 4) of word w
  for (int q = 0; q < 3; ++q) {
    if (te[q * g.tiles + tile] == 0 || s_total[q] > cap) continue;   // uniform
    const uint32_t* roll = g.rolls + ((int64_t)t * 3 + q) * g.rows * g.row_words;
    __syncthreads();                              // the previous kind's edges and scan are read no more
    for (int i = tid; i < g.rows * FR_W; i += FR_THREADS) {
      const int p = i / FR_W, gw = tile * FR_W + i % FR_W;
      const uint32_t x = roll[(int64_t)p * g.row_words + gw];
      const uint32_t nx = gw + 1 < g.row_words ? roll[(int64_t)p * g.row_words + gw + 1] : 0u;
      edge[i] = x & ~((x >> 1) | (nx << 31));
    }
    __syncthreads();
    int c[4] = {0, 0, 0, 0};
    for (int p = 0; p < g.rows; ++p) {
      const uint32_t x = edge[p * FR_W + w] >> b0;
      c[0] += x & 1; c[1] += (x >> 1) & 1; c[2] += (x >> 2) & 1; c[3] += (x >> 3) & 1;
    }
    const int mine = c[0] + c[1] + c[2] + c[3];
    scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < FR_THREADS; d <<= 1) {
      const int v = tid >= d ? scan[tid - d] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    int slot = s_before[q] + scan[tid] - mine;
    int32_t* out = notes + ((int64_t)t * 3 + q) * cap * 3;
    for (int j = 0; j < 4; ++j) {
      if (c[j] == 0) continue;
      const int f = tile * FR_TILE + w * 32 + b0 + j;             // the run's last frame
      for (int p = 0; p < g.rows; ++p) {
        if (!((edge[p * FR_W + w] >> (b0 + j)) & 1u)) continue;
        // walk back along row p to the first frame of the run
        const uint32_t* row = roll + (int64_t)p * g.row_words;
        int gw = f >> 5;
        uint32_t zeros = ~row[gw] & (0xFFFFFFFFu >> (31 - (f & 31)));
        while (zeros == 0 && gw > 0) zeros = ~row[--gw];
        const int first = zeros ? gw * 32 + 32 - __clz((int)zeros) : 0;
        if (slot < cap) {
          out[(int64_t)slot * 3 + 0] = first;
          out[(int64_t)slot * 3 + 1] = f + 1;
          out[(int64_t)slot * 3 + 2] = p;
        }
        ++slot;
      }
    }
  }
}

}  // namespace
}  // namespace m2m

// ------------------------------------------------------------------ C ABI ---
using namespace m2m;

// the checks both exports share: 0, or M2M_ERR_INVALID with the message set under the export's name
static int fr_common_args(const char* who, int R, int L, int sequential, double time_step, int n_labels, int n_timelines, int frame_cap) {
  M2M_REQUIRE(R >= 1 && R <= M2M_SCORE_MAX_ROWS, "%s: %d rows out of range (1..%d)", who, R, M2M_SCORE_MAX_ROWS);
  M2M_REQUIRE(L >= 1 && L <= M2M_SCORE_MAX_TOKENS, "%s: L=%d out of range (1..%d)", who, L, M2M_SCORE_MAX_TOKENS);
  M2M_REQUIRE(sequential == 0 || sequential == 1, "%s: sequential must be 0 or 1", who);
  M2M_REQUIRE(n_timelines == (sequential ? 1 : R), "%s: %d timelines for %d rows (%s)", who, n_timelines, R,
              sequential ? "sequential: one" : "batched: one per row");
  M2M_REQUIRE(time_step > 0.0 && time_step <= 3600.0, "%s: time_step %g out of range (0..3600 s]", who, time_step);
  M2M_REQUIRE(n_labels >= 0 && n_labels <= M2M_SCORE_MAX_LABELS, "%s: %d label notes out of range (0..%d)", who, n_labels,
              M2M_SCORE_MAX_LABELS);
  M2M_REQUIRE(frame_cap >= 1 && frame_cap <= M2M_SCORE_MAX_FRAMES, "%s: frame_cap %d out of range (1..%d)", who, frame_cap,
              M2M_SCORE_MAX_FRAMES);
  return M2M_OK;
}

extern "C" int m2m_score_frame_counts(const int32_t* notes_dev, const int32_t* counts_dev, const float* note_lp_dev, int R, int L,
                                      int sequential, double time_step, const double* labels_dev, const int32_t* label_offsets_dev,
                                      int n_labels, int n_timelines, int frame_cap, const float* min_logprobs_dev, int n_thresholds,
                                      int32_t* out_dev, int32_t* frames_dev, void* stream) {
  const char* who = "m2m_score_frame_counts";
  // every refusal is made on the arguments alone, before the first HIP call
  if (const int st = fr_common_args(who, R, L, sequential, time_step, n_labels, n_timelines, frame_cap)) return st;
  M2M_REQUIRE(n_thresholds >= 1 && n_thresholds <= M2M_SCORE_MAX_THRESHOLDS, "%s: %d thresholds out of range (1..%d)", who, n_thresholds,
              M2M_SCORE_MAX_THRESHOLDS);
  M2M_REQUIRE(notes_dev && counts_dev && label_offsets_dev && out_dev && frames_dev, "%s: null notes / counts / offsets / output / frames",
              who);
  M2M_REQUIRE(labels_dev || n_labels == 0, "%s: null labels", who);
  M2M_REQUIRE(note_lp_dev || n_thresholds == 1, "%s: %d thresholds need the notes' log-probabilities (null note_lp)", who, n_thresholds);
  M2M_REQUIRE(min_logprobs_dev || !note_lp_dev, "%s: null min_logprobs with log-probabilities", who);
  const hipStream_t s = (hipStream_t)stream;
  M2M_CHECK_HIP(hipMemsetAsync(out_dev, 0, (size_t)n_timelines * n_thresholds * 6 * sizeof(int32_t), s));
  FrArgs a;
  a.notes = notes_dev; a.counts = counts_dev; a.note_lp = note_lp_dev; a.lab = labels_dev; a.lab_off = label_offsets_dev;
  a.thr = note_lp_dev ? min_logprobs_dev : nullptr; a.thr0 = 0.0f;
  a.R = R; a.L = L; a.sequential = sequential; a.n_labels = n_labels; a.frame_cap = frame_cap; a.K = n_thresholds; a.time_step = time_step;
  hipLaunchKernelGGL(fr_counts_kernel, dim3((unsigned)ceil_div(frame_cap, FR_TILE), (unsigned)n_timelines), dim3(FR_THREADS), 0, s, a,
                     out_dev, frames_dev);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

extern "C" int m2m_score_error_notes_capacity(int R, int L, int sequential, int max_timeline_labels, int melody_only) {
  if (R < 1 || R > M2M_SCORE_MAX_ROWS || L < 1 || L > M2M_SCORE_MAX_TOKENS || (sequential != 0 && sequential != 1) ||
      max_timeline_labels < 0 || max_timeline_labels > M2M_SCORE_MAX_LABELS || (melody_only != 0 && melody_only != 1))
    return -1;
  // a run of an error roll starts where a run of either side starts or ends: N_ref + N_est runs per kind; the melody's top pitch
  // changes only where a note starts or ends: twice that.  A row decodes to at most L notes.
  const int64_t n = (int64_t)max_timeline_labels + (int64_t)(sequential ? R : 1) * L;
  return (int)((melody_only ? 2 : 1) * n);
}

// the byte offsets of the workspace arrays; the total
static int64_t fr_layout(int64_t T, int64_t tiles, int64_t rows, int64_t at[3]) {
  const int64_t sizes[3] = {4 * T, 4 * T * 3 * tiles, 4 * T * 3 * rows * tiles * FR_W};
  int64_t total = 0;
  for (int i = 0; i < 3; ++i) { at[i] = total; total += align_up(sizes[i], 8); }
  return total;
}

extern "C" int64_t m2m_score_error_notes_workspace_bytes(int n_timelines, int frame_cap, int melody_only) {
  if (n_timelines < 1 || n_timelines > M2M_SCORE_MAX_ROWS || frame_cap < 1 || frame_cap > M2M_SCORE_MAX_FRAMES ||
      (melody_only != 0 && melody_only != 1))
    return -1;
  int64_t at[3];
  return fr_layout(n_timelines, ceil_div(frame_cap, FR_TILE), melody_only ? 12 : FR_ROWS, at);
}

extern "C" int m2m_score_error_notes(const int32_t* notes_dev, const int32_t* counts_dev, const float* note_lp_dev, int R, int L,
                                     int sequential, double time_step, const double* labels_dev, const int32_t* label_offsets_dev,
                                     int n_labels, int n_timelines, int frame_cap, float min_logprob, int melody_only,
                                     int max_timeline_labels, void* workspace_dev, int64_t workspace_bytes, int32_t* notes_out_dev,
                                     int32_t* counts_out_dev, void* stream) {
  const char* who = "m2m_score_error_notes";
  if (const int st = fr_common_args(who, R, L, sequential, time_step, n_labels, n_timelines, frame_cap)) return st;
  M2M_REQUIRE(melody_only == 0 || melody_only == 1, "%s: melody_only must be 0 or 1", who);
  M2M_REQUIRE(max_timeline_labels >= 0 && max_timeline_labels <= M2M_SCORE_MAX_LABELS, "%s: max_timeline_labels %d out of range (0..%d)",
              who, max_timeline_labels, M2M_SCORE_MAX_LABELS);
  M2M_REQUIRE(notes_dev && counts_dev && label_offsets_dev && notes_out_dev && counts_out_dev,
              "%s: null notes / counts / offsets / output notes / output counts", who);
  M2M_REQUIRE(labels_dev || n_labels == 0, "%s: null labels", who);
  M2M_REQUIRE(!(min_logprob != min_logprob), "%s: min_logprob is NaN", who);
  M2M_REQUIRE(note_lp_dev || min_logprob == -INFINITY, "%s: a threshold needs the notes' log-probabilities (null note_lp)", who);
  const int tiles = ceil_div(frame_cap, FR_TILE), rows = melody_only ? 12 : FR_ROWS;
  int64_t at[3];
  const int64_t need = fr_layout(n_timelines, tiles, rows, at);
  M2M_REQUIRE(workspace_dev && ((uintptr_t)workspace_dev & 7) == 0, "%s: null or misaligned workspace (8 bytes)", who);
  M2M_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed (m2m_score_error_notes_workspace_bytes)", who,
              (long long)workspace_bytes, (long long)need);
  const hipStream_t s = (hipStream_t)stream;
  char* w = (char*)workspace_dev;
  FrArgs a;
  a.notes = notes_dev; a.counts = counts_dev; a.note_lp = note_lp_dev; a.lab = labels_dev; a.lab_off = label_offsets_dev;
  a.thr = nullptr; a.thr0 = min_logprob;
  a.R = R; a.L = L; a.sequential = sequential; a.n_labels = n_labels; a.frame_cap = frame_cap; a.K = 1; a.time_step = time_step;
  FrRolls g;
  g.melody = melody_only; g.rows = rows; g.tiles = tiles; g.row_words = tiles * FR_W; g.max_labels = max_timeline_labels;
  g.flags = (int32_t*)(w + at[0]); g.tile_edges = (int32_t*)(w + at[1]); g.rolls = (uint32_t*)(w + at[2]);
  const int cap = m2m_score_error_notes_capacity(R, L, sequential, max_timeline_labels, melody_only);
  const dim3 grid((unsigned)tiles, (unsigned)n_timelines);
  hipLaunchKernelGGL(fr_rolls_kernel, grid, dim3(FR_THREADS), 0, s, a, g);
  M2M_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(fr_notes_kernel, grid, dim3(FR_THREADS), 0, s, g, cap, notes_out_dev, counts_out_dev);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}
