// Note-level matching for gfx950: decoded notes against label notes -> (true positives, decoded notes, label notes) per timeline
// and per confidence threshold, on the device.  The definition is music2midi_amd/note_metrics.py (match_counts: the hit rules of
// mir_eval.transcription.match_notes, the size of a maximum matching from scipy); the three integers are EQUAL to its.
//
// One launch, grid (128 pitches, timelines), on the caller's stream; the workspace is the caller's, nothing is allocated here.
// A hit needs equal pitches, so the hit graph is 128 independent graphs and workgroup (p, t) owns pitch p of timeline t:
//   bucket  every workgroup counts the timeline's kept notes (end > start) per pitch in LDS, labels and output side by side; the
//           exclusive sums give pitch p its own segment of the timeline's part of the workspace, and the workgroup gathers the
//           indices of its notes there (any order).
//   sort    rank sort by (onset, index) inside the segment: the sorted onsets, offsets, the labels' offset tolerance
//           fmax(ratio * (off - on), min_tol) and the output notes' float32 total on + off are written in order.  The onset hit is
//           monotone in |ref_on - est_on|, so the output notes a label note can hit are one interval of the sorted segment: two
//           binary searches per label note give [lo, hi).
//   match   all of the above is done once; the thresholds only mask output notes.  Threshold k is one lane (the lanes are dealt
//           over the four waves) running Kuhn's algorithm, iteratively, on the workgroup's pitch: for every label note in order, a
//           depth-first search for an augmenting path over the candidates of its interval - first for a free candidate, then through
//           the matched ones.  Every augmenting path grows the matching by one and the search is exhaustive (a visited stamp per
//           output note and root), so the final size is the maximum (Berge); the size is unique, whichever matching is found.  The
//           match, stamp and stack arrays of lane k are rows k of the workspace: no recursion, no per-thread arrays.
// Each workgroup then adds its pitch's (tp, n_est, n_ref) to out[t, k] with one integer atomic per number.
//
// All time arithmetic is float64 in the definition's operations: subtract, fabs, rint(x * 1e6) / 1e6 (np.around(x, 6)), compare;
// seconds of an output index are double(index) * time_step.  Contraction is switched off for the whole file by the pragma below, so
// no product here is fused into an addition or subtraction.
#include "common.h"

#include <math.h>

namespace m2m {
namespace {

#pragma clang fp contract(off)

constexpr int NM_THREADS = 256;
constexpr int NM_PITCHES = 128;

// np.around(np.abs(a - b), 6) <= tol
__device__ inline bool nm_hit(double a, double b, double tol) {
  const double d = fabs(a - b);
  const double scaled = d * 1e6;
  return rint(scaled) / 1e6 <= tol;
}

struct NmArgs {
  const int32_t* notes;      // [R][L][3]
  const int32_t* counts;     // [R]
  const float* note_lp;      // [R][L][2] or null
  const double* lab;         // [3][n_labels]
  const int32_t* lab_off;    // [T + 1]
  const float* thr;          // [K] or null
  int R, L, sequential, n_labels, K;
  double time_step, onset_tol, offset_ratio, offset_min_tol;
  // workspace; NR = n_labels, NE = R * L.  Timeline t owns [lab_off[t], lab_off[t + 1]) of the NR arrays and its rows' part of NE.
  double *ref_on, *ref_off, *ref_tol;          // [NR] sorted by onset inside a pitch segment
  double *est_on, *est_off;                    // [NE]
  float* est_tot;                              // [NE]
  int *ref_lo, *ref_hi, *ref_idx, *est_idx;    // [NR] [NR] [NR] [NE]
  int *match, *vis;                            // [K][NE]
  int *stk_u, *stk_c;                          // [K][NR]
};

__device__ inline bool nm_before(double ka, int ia, double kb, int ib) { return ka < kb || (ka == kb && ia < ib); }

__global__ __launch_bounds__(NM_THREADS) void nm_match_kernel(NmArgs a, int32_t* __restrict__ out) {
  __shared__ int hist[2][NM_PITCHES];     // kept notes per pitch: [0] labels, [1] output
  __shared__ int s_bad, s_ref_base, s_est_base, s_ref_fill, s_est_fill;
  const int p = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
  const int r0 = a.sequential ? 0 : t, r1 = a.sequential ? a.R : t + 1;
  const int l0 = min(max(a.lab_off[t], 0), a.n_labels), l1 = min(max(a.lab_off[t + 1], l0), a.n_labels);
  const double* ls = a.lab;
  const double* le = a.lab + a.n_labels;
  const double* lpitch = a.lab + 2 * (int64_t)a.n_labels;
  const int K = a.K;

  if (tid < NM_PITCHES) { hist[0][tid] = 0; hist[1][tid] = 0; }
  if (tid == 0) { s_bad = 0; s_ref_fill = 0; s_est_fill = 0; }
  __syncthreads();

  // ---- bucket: the histogram of the timeline, then this pitch's notes
  for (int i = l0 + tid; i < l1; i += NM_THREADS) {
    if (!(le[i] > ls[i])) continue;
    const int q = (int)lpitch[i];
    if ((unsigned)q < (unsigned)NM_PITCHES) atomicAdd(&hist[0][q], 1);
  }
  for (int r = r0; r < r1; ++r) {
    const int c = a.counts[r];
    if (c < 0) { if (tid == 0) s_bad = 1; continue; }
    const int32_t* nr = a.notes + (int64_t)r * a.L * 3;
    for (int n = tid; n < min(c, a.L); n += NM_THREADS) {
      if (!((double)nr[n * 3 + 1] * a.time_step > (double)nr[n * 3 + 0] * a.time_step)) continue;
      const int q = nr[n * 3 + 2];
      if ((unsigned)q < (unsigned)NM_PITCHES) atomicAdd(&hist[1][q], 1);
    }
  }
  __syncthreads();
  if (s_bad) {                              // uniform, and the same in every workgroup of the timeline: nobody adds anything
    if (p == 0 && tid < K) out[((int64_t)t * K + tid) * 3 + 0] = -1;
    return;
  }
  if (tid == 0) {
    int rb = 0, eb = 0;
    for (int q = 0; q < p; ++q) { rb += hist[0][q]; eb += hist[1][q]; }
    s_ref_base = l0 + rb;
    s_est_base = r0 * a.L + eb;
  }
  __syncthreads();
  const int nr_p = hist[0][p], ne_p = hist[1][p];
  const int rbase = s_ref_base, ebase = s_est_base;
  if (nr_p == 0 && ne_p == 0) return;       // uniform

  for (int i = l0 + tid; i < l1; i += NM_THREADS)
    if (le[i] > ls[i] && (int)lpitch[i] == p) a.ref_idx[rbase + atomicAdd(&s_ref_fill, 1)] = i;
  for (int r = r0; r < r1; ++r) {
    const int c = min(a.counts[r], a.L);
    const int32_t* nr = a.notes + (int64_t)r * a.L * 3;
    for (int n = tid; n < c; n += NM_THREADS)
      if ((double)nr[n * 3 + 1] * a.time_step > (double)nr[n * 3 + 0] * a.time_step && nr[n * 3 + 2] == p)
        a.est_idx[ebase + atomicAdd(&s_est_fill, 1)] = r * a.L + n;
  }
  __syncthreads();

  // ---- sort by (onset, index): every note counts the notes before it
  for (int i = tid; i < nr_p; i += NM_THREADS) {
    const int ia = a.ref_idx[rbase + i];
    const double ka = ls[ia];
    int rank = 0;
    for (int j = 0; j < nr_p; ++j) {
      const int ib = a.ref_idx[rbase + j];
      rank += nm_before(ls[ib], ib, ka, ia) ? 1 : 0;
    }
    const double off = le[ia];
    a.ref_on[rbase + rank] = ka;
    a.ref_off[rbase + rank] = off;
    const double dur = off - ka;
    a.ref_tol[rbase + rank] = fmax(a.offset_ratio * dur, a.offset_min_tol);
  }
  for (int i = tid; i < ne_p; i += NM_THREADS) {
    const int ia = a.est_idx[ebase + i];
    const int32_t* na = a.notes + (int64_t)ia * 3;
    const int ka = na[0];                   // onset indices order as their seconds do (time_step > 0)
    int rank = 0;
    for (int j = 0; j < ne_p; ++j) {
      const int ib = a.est_idx[ebase + j];
      const int kb = a.notes[(int64_t)ib * 3];
      rank += (kb < ka || (kb == ka && ib < ia)) ? 1 : 0;
    }
    a.est_on[ebase + rank] = (double)ka * a.time_step;
    a.est_off[ebase + rank] = (double)na[1] * a.time_step;
    a.est_tot[ebase + rank] = a.note_lp ? a.note_lp[(int64_t)ia * 2 + 0] + a.note_lp[(int64_t)ia * 2 + 1] : 0.0f;
  }
  // rows k of the match / stamp arrays of this segment
  for (int64_t i = tid; i < (int64_t)K * ne_p; i += NM_THREADS) {
    const int64_t at = (i / ne_p) * ((int64_t)a.R * a.L) + ebase + (i % ne_p);
    a.match[at] = -1;
    a.vis[at] = -1;
  }
  __syncthreads();

  // ---- the interval of output notes every label note hits by onset: below it they are earlier and miss, above it later and miss
  for (int u = tid; u < nr_p; u += NM_THREADS) {
    const double on = a.ref_on[rbase + u];
    int lo = 0, hi = ne_p;
    while (lo < hi) {                       // first e that is not (earlier and a miss)
      const int mid = (lo + hi) >> 1;
      const double eo = a.est_on[ebase + mid];
      if (eo < on && !nm_hit(on, eo, a.onset_tol)) lo = mid + 1; else hi = mid;
    }
    const int first = lo;
    hi = ne_p;
    while (lo < hi) {                       // first e that is later and a miss
      const int mid = (lo + hi) >> 1;
      const double eo = a.est_on[ebase + mid];
      if (eo > on && !nm_hit(on, eo, a.onset_tol)) hi = mid; else lo = mid + 1;
    }
    a.ref_lo[rbase + u] = first;
    a.ref_hi[rbase + u] = lo;
  }
  __syncthreads();

  // ---- match: threshold k on one lane, the lanes dealt over the four waves
  const int k = (tid & 63) * (NM_THREADS / 64) + (tid >> 6);
  if (k >= K) return;
  const bool masked = a.note_lp != nullptr && a.thr != nullptr;
  const float thr = masked ? a.thr[k] : 0.0f;
  const bool offsets = a.offset_ratio >= 0.0;
  int* match = a.match + (int64_t)k * ((int64_t)a.R * a.L) + ebase;
  int* vis = a.vis + (int64_t)k * ((int64_t)a.R * a.L) + ebase;
  int* stk_u = a.stk_u + (int64_t)k * a.n_labels + rbase;
  int* stk_c = a.stk_c + (int64_t)k * a.n_labels + rbase;
  const double* ref_on = a.ref_on + rbase;
  const double* ref_off = a.ref_off + rbase;
  const double* ref_tol = a.ref_tol + rbase;
  const int* ref_lo = a.ref_lo + rbase;
  const int* ref_hi = a.ref_hi + rbase;
  const double* est_on = a.est_on + ebase;
  const double* est_off = a.est_off + ebase;
  const float* est_tot = a.est_tot + ebase;

  int n_est = 0;
  for (int e = 0; e < ne_p; ++e) n_est += (masked && est_tot[e] < thr) ? 0 : 1;

  // edge(u, e): e is kept under the threshold and hits u (the interval holds the onset hits; the test is repeated, it is cheap)
  auto edge = [&](int u, int e) -> bool {
    if (masked && est_tot[e] < thr) return false;
    if (!nm_hit(ref_on[u], est_on[e], a.onset_tol)) return false;
    return !offsets || nm_hit(ref_off[u], est_off[e], ref_tol[u]);
  };

  int tp = 0;
  for (int root = 0; root < nr_p; ++root) {
    int sp = 0;
    stk_u[0] = root;
    stk_c[0] = -1;                          // -1: the free candidates have not been looked at yet
    while (sp >= 0) {
      const int u = stk_u[sp];
      const int hi = ref_hi[u];
      int c = stk_c[sp];
      if (c < 0) {
        int free_e = -1;
        for (int e = ref_lo[u]; e < hi; ++e)
          if (match[e] < 0 && edge(u, e)) { free_e = e; break; }
        if (free_e >= 0) {                  // augment: level l takes the candidate it descended through
          match[free_e] = u;
          for (int l = sp - 1; l >= 0; --l) match[stk_c[l] - 1] = stk_u[l];
          ++tp;
          break;
        }
        c = ref_lo[u];
      }
      int next = -1;
      while (c < hi) {
        const int e = c++;
        if (vis[e] != root && edge(u, e)) { vis[e] = root; next = e; break; }
      }
      stk_c[sp] = c;
      if (next < 0) { --sp; continue; }
      if (sp + 1 >= nr_p) { --sp; continue; }   // cannot happen: the label notes of a path are distinct
      ++sp;
      stk_u[sp] = match[next];
      stk_c[sp] = -1;
    }
  }
  int32_t* o = out + ((int64_t)t * K + k) * 3;
  if (tp) atomicAdd(&o[0], tp);
  if (n_est) atomicAdd(&o[1], n_est);
  if (nr_p) atomicAdd(&o[2], nr_p);
}

}  // namespace
}  // namespace m2m

// ------------------------------------------------------------------ C ABI ---
using namespace m2m;

// the byte offsets of the workspace arrays for NR label notes, NE = R * L output notes and K thresholds; the total
static int64_t nm_layout(int64_t NR, int64_t NE, int64_t K, int64_t at[14]) {
  const int64_t sizes[14] = {8 * NR, 8 * NR, 8 * NR, 8 * NE, 8 * NE, 4 * NE, 4 * NR, 4 * NR, 4 * NR, 4 * NE,
                             4 * K * NE, 4 * K * NE, 4 * K * NR, 4 * K * NR};
  int64_t total = 0;
  for (int i = 0; i < 14; ++i) { at[i] = total; total += align_up(sizes[i], 8); }
  return total > 0 ? total : 8;
}

extern "C" int64_t m2m_score_note_workspace_bytes(int R, int L, int n_labels, int n_thresholds) {
  if (R < 1 || R > M2M_SCORE_MAX_ROWS || L < 1 || L > M2M_SCORE_MAX_TOKENS || n_labels < 0 || n_labels > M2M_SCORE_MAX_LABELS ||
      n_thresholds < 1 || n_thresholds > M2M_SCORE_MAX_THRESHOLDS)
    return -1;
  int64_t at[14];
  return nm_layout(n_labels, (int64_t)R * L, n_thresholds, at);
}

extern "C" int m2m_score_note_counts(const int32_t* notes_dev, const int32_t* counts_dev, const float* note_lp_dev, int R, int L,
                                     int sequential, double time_step, const double* labels_dev, const int32_t* label_offsets_dev,
                                     int n_labels, int n_timelines, double onset_tolerance, double offset_ratio,
                                     double offset_min_tolerance, const float* min_logprobs_dev, int n_thresholds, void* workspace_dev,
                                     int64_t workspace_bytes, int32_t* out_dev, void* stream) {
  const char* who = "m2m_score_note_counts";
  // every refusal is made on the arguments alone, before the first HIP call
  M2M_REQUIRE(R >= 1 && R <= M2M_SCORE_MAX_ROWS, "%s: %d rows out of range (1..%d)", who, R, M2M_SCORE_MAX_ROWS);
  M2M_REQUIRE(L >= 1 && L <= M2M_SCORE_MAX_TOKENS, "%s: L=%d out of range (1..%d)", who, L, M2M_SCORE_MAX_TOKENS);
  M2M_REQUIRE(sequential == 0 || sequential == 1, "%s: sequential must be 0 or 1", who);
  M2M_REQUIRE(n_timelines == (sequential ? 1 : R), "%s: %d timelines for %d rows (%s)", who, n_timelines, R,
              sequential ? "sequential: one" : "batched: one per row");
  M2M_REQUIRE(time_step > 0.0 && time_step <= 3600.0, "%s: time_step %g out of range (0..3600 s]", who, time_step);
  M2M_REQUIRE(n_labels >= 0 && n_labels <= M2M_SCORE_MAX_LABELS, "%s: %d label notes out of range (0..%d)", who, n_labels,
              M2M_SCORE_MAX_LABELS);
  M2M_REQUIRE(n_thresholds >= 1 && n_thresholds <= M2M_SCORE_MAX_THRESHOLDS, "%s: %d thresholds out of range (1..%d)", who, n_thresholds,
              M2M_SCORE_MAX_THRESHOLDS);
  M2M_REQUIRE(onset_tolerance >= 0.0 && onset_tolerance <= 3600.0, "%s: onset_tolerance %g out of range [0..3600 s]", who,
              onset_tolerance);
  M2M_REQUIRE(offset_ratio == offset_ratio && offset_ratio <= 1e6, "%s: offset_ratio %g out of range (negative: onsets only; at most 1e6)",
              who, offset_ratio);
  M2M_REQUIRE(offset_min_tolerance >= 0.0 && offset_min_tolerance <= 3600.0, "%s: offset_min_tolerance %g out of range [0..3600 s]", who,
              offset_min_tolerance);
  M2M_REQUIRE(notes_dev && counts_dev && label_offsets_dev && out_dev, "%s: null notes / counts / offsets / output", who);
  M2M_REQUIRE(labels_dev || n_labels == 0, "%s: null labels", who);
  M2M_REQUIRE(note_lp_dev || n_thresholds == 1, "%s: %d thresholds need the notes' log-probabilities (null note_lp)", who, n_thresholds);
  M2M_REQUIRE(min_logprobs_dev || !note_lp_dev, "%s: null min_logprobs with log-probabilities", who);
  int64_t at[14];
  const int64_t need = nm_layout(n_labels, (int64_t)R * L, n_thresholds, at);
  M2M_REQUIRE(workspace_dev && ((uintptr_t)workspace_dev & 7) == 0, "%s: null or misaligned workspace (8 bytes)", who);
  M2M_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed (m2m_score_note_workspace_bytes)", who,
              (long long)workspace_bytes, (long long)need);
  const hipStream_t s = (hipStream_t)stream;
  M2M_CHECK_HIP(hipMemsetAsync(out_dev, 0, (size_t)n_timelines * n_thresholds * 3 * sizeof(int32_t), s));
  char* w = (char*)workspace_dev;
  NmArgs a;
  a.notes = notes_dev; a.counts = counts_dev; a.note_lp = note_lp_dev; a.lab = labels_dev; a.lab_off = label_offsets_dev;
  a.thr = min_logprobs_dev;
  a.R = R; a.L = L; a.sequential = sequential; a.n_labels = n_labels; a.K = n_thresholds;
  a.time_step = time_step; a.onset_tol = onset_tolerance; a.offset_ratio = offset_ratio; a.offset_min_tol = offset_min_tolerance;
  a.ref_on = (double*)(w + at[0]); a.ref_off = (double*)(w + at[1]); a.ref_tol = (double*)(w + at[2]);
  a.est_on = (double*)(w + at[3]); a.est_off = (double*)(w + at[4]); a.est_tot = (float*)(w + at[5]);
  a.ref_lo = (int*)(w + at[6]); a.ref_hi = (int*)(w + at[7]); a.ref_idx = (int*)(w + at[8]); a.est_idx = (int*)(w + at[9]);
  a.match = (int*)(w + at[10]); a.vis = (int*)(w + at[11]); a.stk_u = (int*)(w + at[12]); a.stk_c = (int*)(w + at[13]);
  hipLaunchKernelGGL(nm_match_kernel, dim3((unsigned)NM_PITCHES, (unsigned)n_timelines), dim3(NM_THREADS), 0, s, a, out_dev);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}
