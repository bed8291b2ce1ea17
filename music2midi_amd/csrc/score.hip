// Scoring of decoded tokens for gfx950: token ids -> notes -> melody -> the two integers chroma accuracy is a ratio of, on the device.
// Replaces, for labelled decodes, ref: music2midi/tokenizer.py:169-200 (the decode state machine), music2midi/utils.py:5-20 and
// music2midi/evaluation.py:10-75; the definitions are music2midi_amd/tokenizer.py (_decode_tokens, _decode), utils.py (numpy_to_midi)
// and evaluation.py, which stay the oracle.  Everything here is integer work except the frame arithmetic, which repeats the host's
// float64 operations in the host's order (sc_frame_count, sc_frame_pos): the results are equal, not close.
//
// Two launches, both on the caller's stream, nothing returns to the host:
//   detok   one workgroup per token row.  The ids go to LDS (range-checked, 16 bit); ONE lane walks them as the host loop does and
//           files every emission: an ONSET opens note n (time, pitch, the pitch's latest OFFSET event so far), an OFFSET appends an
//           event to its pitch's chain.  All lanes then close the notes: note n takes the first event of its pitch's chain, after
//           the one it was linked to, whose time is later than its onset - the event that closes it on the host, where an OFFSET
//           closes every open earlier note of the pitch.  A block scan compacts the closed notes in emission order.
//           The scored form (m2m_score_detokenize_scored) is the same body with the tokens' log-probabilities staged next to the
//           ids: the walking lane files (lp[time] + lp[mode]) + lp[pitch] with every note and every OFFSET event, the closing pass
//           gives a note its event's sum and drops it when on + off < min_logprob, before the scan.
//   counts  grid (frame tiles, timelines).  A workgroup reads its timeline's notes twice: the largest per-note frame count is
//           n_frames (monotone in the end time), then every note raises the pitch of the frames it covers inside the tile with LDS
//           integer maxima, labels and output side by side; the n_frames - 1 cut and the two counts follow from the tile in LDS, one
//           integer atomic add per count and workgroup.  The melody never goes to memory.
#include "common.h"
#include "score_frames.h"

#include <math.h>

namespace m2m {
namespace {

constexpr int SC_THREADS = 256;
constexpr int SC_MAX_L = M2M_SCORE_MAX_TOKENS;
constexpr int SC_TILE = 2048;          // frames of one timeline per workgroup of the counts kernel (2 x 8 KiB of LDS)
constexpr int SC_EOS = 2, SC_ONSET = 3, SC_OFFSET = 4;

// The frame arithmetic (sc_frame_count, sc_frame_pos, sc_seconds and the saturating conversions) is score_frames.h, shared with
// frame_roll.hip.  No contraction or reassociation may touch the float sums below either.
#pragma clang fp contract(off)

// SCORED: lp is the log-probability of every id, column-aligned.  Every sum below is one rounded float32 add, in the order of
// music2midi_amd/confidence.py (note_logprobs): (time + mode) + pitch per emission, on + off per note; contraction is off above.
template <bool SCORED>
__global__ __launch_bounds__(SC_THREADS) void sc_detok_kernel(const int64_t* __restrict__ ids, int L, int64_t row_stride,
                                                              int64_t steps_per_row, int pitch_offset, int time_offset, int vocab_size,
                                                              const float* __restrict__ lp, int64_t lp_row_stride, float min_logprob,
                                                              int32_t* __restrict__ notes, int32_t* __restrict__ counts,
                                                              float* __restrict__ note_lp) {
  __shared__ __attribute__((aligned(16))) uint16_t tok[SC_MAX_L];
  __shared__ int note_t[SC_MAX_L];          // onset index of note n
  __shared__ int note_e[SC_MAX_L];          // offset index, -1 = never closed
  __shared__ short note_link[SC_MAX_L];     // the latest OFFSET event of the note's pitch when it was opened, -1 = none
  __shared__ unsigned char note_p[SC_MAX_L];
  __shared__ int off_t[SC_MAX_L];           // time index of OFFSET event k
  __shared__ short off_next[SC_MAX_L];      // the next OFFSET event of the same pitch, -1 = last
  __shared__ short first_off[128], last_off[128];
  __shared__ int scan[SC_THREADS];
  __shared__ int s_bad, s_notes;
  // scored only (24 KiB on top of the 39.5 KiB above: 63.5 KiB of the 64 KiB a workgroup may declare)
  constexpr int SC_LP = SCORED ? SC_MAX_L : 4;
  __shared__ __attribute__((aligned(16))) float tok_lp[SC_LP];   // lp of id i; after the walk: the offset part of note n
  __shared__ float note_on[SC_LP];          // onset part of note n
  __shared__ float off_lp[SC_LP];           // sum of OFFSET event k
  float* const note_off = tok_lp;

  const int r = blockIdx.x, tid = threadIdx.x;
  const int64_t* row = ids + (int64_t)r * row_stride;
  if (tid == 0) { s_bad = 0; s_notes = 0; }
  if (tid < 128) { first_off[tid] = -1; last_off[tid] = -1; }
  __syncthreads();
  const int Lp = (L + 7) & ~7;              // the walk reads 8 ids at a time: the tail is EOS
  bool bad = false;
  for (int i = tid; i < Lp; i += SC_THREADS) {
    int64_t v = SC_EOS;
    if (i < L) {
      v = row[i];
      if (v < 0 || v >= (int64_t)vocab_size) { bad = true; v = SC_EOS; }
    }
    tok[i] = (uint16_t)v;
    if constexpr (SCORED) tok_lp[i] = i < L ? lp[(int64_t)r * lp_row_stride + i] : 0.0f;
  }
  if (bad) s_bad = 1;
  __syncthreads();
  if (s_bad) {                              // uniform
    if (tid == 0) counts[r] = -1;
    return;
  }

  if (tid == 0) {
    const int start = (int)((int64_t)r * steps_per_row);
    int time_idx = -1, mode = -1, pitch = -1, nn = 0, no = 0;
    float time_lp = 0.0f, mode_lp = 0.0f, pitch_lp = 0.0f;          // lp of the latest time / mode / pitch token
    bool done = false;
    for (int i = 0; i < Lp && !done; i += 8) {
      const uint4 w = *reinterpret_cast<const uint4*>(&tok[i]);
      const uint32_t words[4] = {w.x, w.y, w.z, w.w};
      float lps[8] = {};
      if constexpr (SCORED) {
        const float4 a = *reinterpret_cast<const float4*>(&tok_lp[i]), b = *reinterpret_cast<const float4*>(&tok_lp[i + 4]);
        lps[0] = a.x; lps[1] = a.y; lps[2] = a.z; lps[3] = a.w; lps[4] = b.x; lps[5] = b.y; lps[6] = b.z; lps[7] = b.w;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int t = (int)((words[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
        if (t == SC_EOS) { done = true; break; }
        if (t < SC_EOS) continue;                                   // PAD, BOS
        if (t == SC_ONSET) mode = 1;
        else if (t == SC_OFFSET) mode = 0;
        if (t >= time_offset) { time_idx = start + (t - time_offset); mode = -1; pitch = -1; }
        else if (t >= pitch_offset) pitch = t - pitch_offset;
        if constexpr (SCORED) {
          if (t >= time_offset) time_lp = lps[k];
          else if (t >= pitch_offset) pitch_lp = lps[k];
          else if (t <= SC_OFFSET) mode_lp = lps[k];                // ONSET, OFFSET
        }
        if (time_idx == -1 || mode == -1 || pitch == -1) continue;
        if (mode == 1) {
          note_t[nn] = time_idx;
          note_p[nn] = (unsigned char)pitch;
          note_link[nn] = last_off[pitch];
          if constexpr (SCORED) note_on[nn] = (time_lp + mode_lp) + pitch_lp;
          ++nn;
        } else {
          off_t[no] = time_idx;
          if constexpr (SCORED) off_lp[no] = (time_lp + mode_lp) + pitch_lp;
          off_next[no] = -1;
          const int l = last_off[pitch];
          if (l < 0) first_off[pitch] = (short)no;
          else off_next[l] = (short)no;
          last_off[pitch] = (short)no;
          ++no;
        }
        pitch = -1;
      }
    }
    s_notes = nn;
  }
  __syncthreads();

  // close: the first later OFFSET event of the pitch with time > onset (time may go backwards: earlier-or-equal ones are skipped)
  const int nn = s_notes;
  for (int n = tid; n < nn; n += SC_THREADS) {
    const int l = note_link[n], on = note_t[n];
    int k = l < 0 ? first_off[note_p[n]] : off_next[l];
    while (k >= 0 && off_t[k] <= on) k = off_next[k];
    int e = k >= 0 ? off_t[k] : -1;
    if constexpr (SCORED) {
      if (k >= 0) {                           // the filter: dropped iff on + off < min_logprob (a NaN total is kept)
        const float off = off_lp[k];
        if (note_on[n] + off < min_logprob) e = -1;
        note_off[n] = off;                    // tok_lp is dead: the walk ended before the barrier above
      }
    }
    note_e[n] = e;
  }
  __syncthreads();

  // compact: thread t owns notes [8 t, 8 t + 8)
  const int base = tid * (SC_MAX_L / SC_THREADS);
  int mine = 0;
#pragma unroll
  for (int j = 0; j < SC_MAX_L / SC_THREADS; ++j) {
    const int n = base + j;
    if (n < nn && note_e[n] >= 0) ++mine;
  }
  scan[tid] = mine;
  __syncthreads();
  for (int s = 1; s < SC_THREADS; s <<= 1) {
    const int v = tid >= s ? scan[tid - s] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  int pos = scan[tid] - mine;
  int32_t* out = notes + (int64_t)r * L * 3;
#pragma unroll
  for (int j = 0; j < SC_MAX_L / SC_THREADS; ++j) {
    const int n = base + j;
    if (n < nn && note_e[n] >= 0 && pos < L) {       // pos < L always holds (every emission consumed a token)
      out[pos * 3 + 0] = note_t[n];
      out[pos * 3 + 1] = note_e[n];
      out[pos * 3 + 2] = note_p[n];
      if constexpr (SCORED) {
        float* out_lp = note_lp + (int64_t)r * L * 2;
        out_lp[pos * 2 + 0] = note_on[n];
        out_lp[pos * 2 + 1] = note_off[n];
      }
      ++pos;
    }
  }
  if (tid == SC_THREADS - 1) counts[r] = scan[tid];
}

struct ScCounts {
  const int32_t* notes;      // [R][L][3]
  const int32_t* counts;     // [R]
  const double* lab;         // [3][n_labels]: start, end, pitch
  const int32_t* lab_off;    // [T + 1]
  int R, L, sequential, n_labels, frame_cap;
  double time_step;
};

__global__ __launch_bounds__(SC_THREADS) void sc_counts_kernel(ScCounts a, int32_t* __restrict__ out) {
  __shared__ int mel[2][SC_TILE];           // [0] labels, [1] output: highest covered pitch of the tile's frames, -1 = silent
  __shared__ int s_nf, s_correct, s_voiced;
  const int t = blockIdx.y, tid = threadIdx.x;
  const int tile0 = blockIdx.x * SC_TILE;
  const int r0 = a.sequential ? 0 : t, r1 = a.sequential ? a.R : t + 1;
  const int l0 = a.lab_off[t], l1 = a.lab_off[t + 1];
  const double* ls = a.lab;
  const double* le = a.lab + a.n_labels;
  const double* lp = a.lab + 2 * (int64_t)a.n_labels;

  if (tid == 0) { s_nf = 0; s_correct = 0; s_voiced = 0; }
  for (int j = tid; j < SC_TILE; j += SC_THREADS) { mel[0][j] = -1; mel[1][j] = -1; }
  __syncthreads();

  // n_frames of the timeline, over the labels and the output together; notes with end <= start do not exist
  int m = 0;
  for (int i = l0 + tid; i < l1; i += SC_THREADS)
    if (le[i] > ls[i]) m = max(m, sc_count_capped(le[i], a.frame_cap));
  for (int r = r0; r < r1; ++r) {
    const int c = a.counts[r];
    const int32_t* nr = a.notes + (int64_t)r * a.L * 3;
    for (int n = tid; n < c; n += SC_THREADS) m = max(m, sc_count_capped(sc_seconds(nr[n * 3 + 1], a.time_step), a.frame_cap));
  }
  if (m > 0) atomicMax(&s_nf, m);
  __syncthreads();
  const int nf = s_nf;
  if (nf > a.frame_cap) {                   // a timeline longer than the caller sized the grid for: no counts, frames = -1
    if (blockIdx.x == 0 && tid == 0) out[t * 3 + 2] = -1;
    return;
  }
  if (blockIdx.x == 0 && tid == 0) out[t * 3 + 2] = nf;
  const int last = nf - 1;                  // frames [0, last) are compared; the roll's last frame stays silent
  if (tile0 >= last) return;                // uniform
  const int tile1 = min(tile0 + SC_TILE, last);

  for (int i = l0 + tid; i < l1; i += SC_THREADS) {
    const double s = ls[i], e = le[i];
    if (!(e > s)) continue;
    const int lo = max(sc_pos_capped(s, a.frame_cap), tile0), hi = min(sc_pos_capped(e, a.frame_cap), tile1);
    const int p = (int)lp[i];
    for (int f = lo; f < hi; ++f) atomicMax(&mel[0][f - tile0], p);
  }
  for (int r = r0; r < r1; ++r) {
    const int c = a.counts[r];
    const int32_t* nr = a.notes + (int64_t)r * a.L * 3;
    for (int n = tid; n < c; n += SC_THREADS) {
      const int lo = max(sc_pos_capped(sc_seconds(nr[n * 3 + 0], a.time_step), a.frame_cap), tile0);
      const int hi = min(sc_pos_capped(sc_seconds(nr[n * 3 + 1], a.time_step), a.frame_cap), tile1);
      const int p = nr[n * 3 + 2];
      for (int f = lo; f < hi; ++f) atomicMax(&mel[1][f - tile0], p);
    }
  }
  __syncthreads();

  int correct = 0, voiced = 0;
  for (int j = tid; j < tile1 - tile0; j += SC_THREADS) {
    const int l = mel[0][j], o = mel[1][j];
    if (l >= 0) {
      ++voiced;
      if (o >= 0 && (l - o) % 12 == 0) ++correct;
    }
  }
  if (voiced) atomicAdd(&s_voiced, voiced);
  if (correct) atomicAdd(&s_correct, correct);
  __syncthreads();
  if (tid == 0) {
    if (s_correct) atomicAdd(&out[t * 3 + 0], s_correct);
    if (s_voiced) atomicAdd(&out[t * 3 + 1], s_voiced);
  }
}

}  // namespace
}  // namespace m2m

// ------------------------------------------------------------------ C ABI ---
using namespace m2m;

extern "C" int64_t m2m_score_frame_count(double end_seconds) {
  if (!(end_seconds > 0.0)) return 0;
  const double f = sc_frame_count(end_seconds);
  return f >= 9.0e18 ? INT64_MAX : (int64_t)f;
}

// the checks the two detokenise exports share: 0, or M2M_ERR_INVALID with the message set under the export's name
static int sc_detok_args(const char* who, int R, int L, int64_t row_stride, int64_t steps_per_row, int pitch_offset, int time_offset,
                         int vocab_size) {
  M2M_REQUIRE(R >= 1 && R <= M2M_SCORE_MAX_ROWS, "%s: %d rows out of range (1..%d)", who, R, M2M_SCORE_MAX_ROWS);
  M2M_REQUIRE(L >= 1 && L <= M2M_SCORE_MAX_TOKENS, "%s: L=%d out of range (1..%d)", who, L, M2M_SCORE_MAX_TOKENS);
  M2M_REQUIRE(row_stride >= L, "%s: row stride %lld below L=%d", who, (long long)row_stride, L);
  M2M_REQUIRE(vocab_size >= 1 && vocab_size <= 4096, "%s: vocab_size %d out of range (1..4096)", who, vocab_size);
  M2M_REQUIRE(pitch_offset >= 5, "%s: pitch_offset %d below the 5 special ids", who, pitch_offset);
  M2M_REQUIRE(time_offset > pitch_offset && time_offset - pitch_offset <= 128, "%s: %d pitch ids out of range (1..128)", who,
              time_offset - pitch_offset);
  M2M_REQUIRE(time_offset <= vocab_size, "%s: time_offset %d beyond vocab_size %d", who, time_offset, vocab_size);
  M2M_REQUIRE(steps_per_row >= 0 && steps_per_row <= INT32_MAX, "%s: steps_per_row %lld out of range", who, (long long)steps_per_row);
  M2M_REQUIRE((int64_t)(R - 1) * steps_per_row + (int64_t)(vocab_size - time_offset) <= (int64_t)INT32_MAX,
              "%s: time index of row %d does not fit in int32 (steps_per_row %lld)", who, R - 1, (long long)steps_per_row);
  M2M_REQUIRE((int64_t)(R - 1) * row_stride + L <= (int64_t)INT32_MAX, "%s: the id tensor does not fit in int32 elements", who);
  return M2M_OK;
}

extern "C" int m2m_score_detokenize(const int64_t* ids_dev, int R, int L, int64_t row_stride, int64_t steps_per_row, int pitch_offset,
                                    int time_offset, int vocab_size, int32_t* notes_out_dev, int32_t* counts_out_dev, void* stream) {
  // every refusal is made on the arguments alone, before the first HIP call
  if (const int st = sc_detok_args("m2m_score_detokenize", R, L, row_stride, steps_per_row, pitch_offset, time_offset, vocab_size)) return st;
  M2M_REQUIRE(ids_dev && notes_out_dev && counts_out_dev, "m2m_score_detokenize: null ids / notes / counts");
  hipLaunchKernelGGL(sc_detok_kernel<false>, dim3((unsigned)R), dim3(SC_THREADS), 0, (hipStream_t)stream, ids_dev, L, row_stride,
                     steps_per_row, pitch_offset, time_offset, vocab_size, (const float*)nullptr, (int64_t)0, 0.0f, notes_out_dev,
                     counts_out_dev, (float*)nullptr);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

extern "C" int m2m_score_detokenize_scored(const int64_t* ids_dev, int R, int L, int64_t row_stride, int64_t steps_per_row,
                                           int pitch_offset, int time_offset, int vocab_size, const float* logprobs_dev,
                                           int64_t lp_row_stride, float min_logprob, int32_t* notes_dev, int32_t* counts_dev,
                                           float* note_lp_dev, void* stream) {
  const char* who = "m2m_score_detokenize_scored";
  if (const int st = sc_detok_args(who, R, L, row_stride, steps_per_row, pitch_offset, time_offset, vocab_size)) return st;
  M2M_REQUIRE(lp_row_stride >= L, "%s: log-probability row stride %lld below L=%d", who, (long long)lp_row_stride, L);
  M2M_REQUIRE((int64_t)(R - 1) * lp_row_stride + L <= (int64_t)INT32_MAX, "%s: the log-probability tensor does not fit in int32 elements",
              who);
  M2M_REQUIRE(ids_dev && notes_dev && counts_dev, "%s: null ids / notes / counts", who);
  M2M_REQUIRE(logprobs_dev && note_lp_dev, "%s: null logprobs / note_lp", who);
  hipLaunchKernelGGL(sc_detok_kernel<true>, dim3((unsigned)R), dim3(SC_THREADS), 0, (hipStream_t)stream, ids_dev, L, row_stride,
                     steps_per_row, pitch_offset, time_offset, vocab_size, logprobs_dev, lp_row_stride, min_logprob, notes_dev, counts_dev,
                     note_lp_dev);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

extern "C" int m2m_score_chroma_counts(const int32_t* notes_dev, const int32_t* counts_dev, int R, int L, int sequential, double time_step,
                                       const double* labels_dev, const int32_t* label_offsets_dev, int n_labels, int n_timelines,
                                       int frame_cap, int32_t* out_dev, void* stream) {
  M2M_REQUIRE(R >= 1 && R <= M2M_SCORE_MAX_ROWS, "m2m_score_chroma_counts: %d rows out of range (1..%d)", R, M2M_SCORE_MAX_ROWS);
  M2M_REQUIRE(L >= 1 && L <= M2M_SCORE_MAX_TOKENS, "m2m_score_chroma_counts: L=%d out of range (1..%d)", L, M2M_SCORE_MAX_TOKENS);
  M2M_REQUIRE(sequential == 0 || sequential == 1, "m2m_score_chroma_counts: sequential must be 0 or 1");
  M2M_REQUIRE(n_timelines == (sequential ? 1 : R), "m2m_score_chroma_counts: %d timelines for %d rows (%s)", n_timelines, R,
              sequential ? "sequential: one" : "batched: one per row");
  M2M_REQUIRE(time_step > 0.0 && time_step <= 3600.0, "m2m_score_chroma_counts: time_step %g out of range (0..3600 s]", time_step);
  M2M_REQUIRE(n_labels >= 0 && n_labels <= M2M_SCORE_MAX_LABELS, "m2m_score_chroma_counts: %d label notes out of range (0..%d)", n_labels,
              M2M_SCORE_MAX_LABELS);
  M2M_REQUIRE(frame_cap >= 1 && frame_cap <= M2M_SCORE_MAX_FRAMES, "m2m_score_chroma_counts: frame_cap %d out of range (1..%d)", frame_cap,
              M2M_SCORE_MAX_FRAMES);
  M2M_REQUIRE(notes_dev && counts_dev && label_offsets_dev && out_dev, "m2m_score_chroma_counts: null notes / counts / offsets / output");
  M2M_REQUIRE(labels_dev || n_labels == 0, "m2m_score_chroma_counts: null labels");
  const hipStream_t s = (hipStream_t)stream;
  M2M_CHECK_HIP(hipMemsetAsync(out_dev, 0, (size_t)n_timelines * 3 * sizeof(int32_t), s));
  ScCounts a;
  a.notes = notes_dev; a.counts = counts_dev; a.lab = labels_dev; a.lab_off = label_offsets_dev;
  a.R = R; a.L = L; a.sequential = sequential; a.n_labels = n_labels; a.frame_cap = frame_cap; a.time_step = time_step;
  hipLaunchKernelGGL(sc_counts_kernel, dim3((unsigned)ceil_div(frame_cap, SC_TILE), (unsigned)n_timelines), dim3(SC_THREADS), 0, s, a, out_dev);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}
