// Consensus selection for gfx950: the K candidate transcriptions of every clip scored against each other with the note-level
// metric, and the candidate the others agree with most.  The definition is music2midi_amd/consensus.py (pairwise_counts: tp[i, j] =
// note_metrics.match_counts(ref = candidate j, est = candidate i)[0]; expected_agreement; select); the integers are EQUAL to its and
// the utilities are its float64, bit for bit.
//
// m2m_consensus_pairwise_counts: one launch, grid (128 pitches, clips), on the caller's stream; the workspace is the caller's.  A hit
// needs equal pitches, so workgroup (p, b) owns pitch p of the K rows b * K .. b * K + K - 1:
//   bucket  the kept notes (end > start) of every candidate per pitch in LDS (16 x 128 ints); the exclusive sums give pitch p its own
//           segment inside every row's L slots of the workspace, and the workgroup gathers the indices of its notes there.
//   sort    rank sort by (onset index, note index) inside each segment: onsets, offsets and the tolerance the note has AS A
//           REFERENCE, fmax(ratio * (off - on), min_tol), are written in order.
//   pairs   every ordered pair (est i, ref j), i != j, owns L ints of four arrays; the segment bases of rows i and j address them.
//           A wave per pair resets match and stamp and finds, for every reference note, the interval of estimated notes it hits by
//           onset (two binary searches; the onset hit is monotone in the distance).
//   match   one lane per ordered pair (at most 240, dealt over the four waves) runs Kuhn's augmenting paths, iteratively, as
//           nm_match_kernel of note_match.hip does for one threshold: the hit test, the interval search and the path loop are its
//           operations in its order.  The stack entry and the interval are packed two 16-bit halves to an int (indices are <= 2048).
// Each workgroup adds its pitch's matching sizes to tp_out[b, i, j] with one integer atomic, and its kept-note counts to n_out[b, i]
// and the diagonal.  Every workspace entry a workgroup reads it has written in the same launch.
//
// m2m_consensus_select: one wave per clip; lane i sums agreement(tp[i, j], n[i], n[j]) over j != i in increasing j in float64 and
// divides by K - 1; the first maximum is chosen.
//
// Time arithmetic is float64 in the definition's operations; contraction is switched off for the whole file.
#include "common.h"

#include <math.h>

namespace m2m {
namespace {

#pragma clang fp contract(off)

constexpr int CS_THREADS = 256;
constexpr int CS_PITCHES = 128;
constexpr int CS_MAXK = M2M_CONSENSUS_MAX_CANDIDATES;

// np.around(np.abs(a - b), 6) <= tol
__device__ inline bool cs_hit(double a, double b, double tol) {
  const double d = fabs(a - b);
  const double scaled = d * 1e6;
  return rint(scaled) / 1e6 <= tol;
}

struct CsArgs {
  const int32_t* notes;      // [R][L][3]
  const int32_t* counts;     // [R]
  int R, L, K;
  double time_step, onset_tol, offset_ratio, offset_min_tol;
  // workspace; NE = R * L, NP = R * (K - 1) * L.  Row r owns [r * L, r * L + L) of the NE arrays, pair q of clip b
  // [(b * K * (K - 1) + q) * L, + L) of the NP arrays.
  double *on, *off, *tol;    // [NE] sorted by onset inside a pitch segment
  int* idx;                  // [NE]
  int *match, *vis;          // [NP] by estimated note
  int *stk, *lohi;           // [NP] by stack level / by reference note
};

__global__ __launch_bounds__(CS_THREADS) void cs_pairwise_kernel(CsArgs a, int32_t* __restrict__ tp_out, int32_t* __restrict__ n_out) {
  __shared__ int hist[CS_MAXK][CS_PITCHES];    // kept notes per candidate and pitch
  __shared__ int s_base[CS_MAXK], s_fill[CS_MAXK];
  __shared__ int s_bad, s_any;
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int K = a.K, L = a.L;
  const int64_t row0 = (int64_t)b * K;

  for (int i = tid; i < CS_MAXK * CS_PITCHES; i += CS_THREADS) (&hist[0][0])[i] = 0;
  if (tid < CS_MAXK) { s_base[tid] = 0; s_fill[tid] = 0; }
  if (tid == 0) { s_bad = 0; s_any = 0; }
  __syncthreads();

  // ---- bucket: the histogram of every candidate, then this pitch's notes
  for (int c = 0; c < K; ++c) {
    const int cnt = a.counts[row0 + c];
    if (cnt < 0) { if (tid == 0) s_bad = 1; continue; }
    const int32_t* nr = a.notes + (row0 + c) * L * 3;
    for (int n = tid; n < min(cnt, L); n += CS_THREADS) {
      if (!((double)nr[n * 3 + 1] * a.time_step > (double)nr[n * 3 + 0] * a.time_step)) continue;
      const int q = nr[n * 3 + 2];
      if ((unsigned)q < (unsigned)CS_PITCHES) atomicAdd(&hist[c][q], 1);
    }
  }
  __syncthreads();
  if (s_bad) {                                 // uniform, and the same in every workgroup of the clip: nobody adds anything
    if (p == 0 && tid == 0) tp_out[row0 * K] = -1;
    return;
  }
  if (tid < K) {
    int base = 0;
    for (int q = 0; q < p; ++q) base += hist[tid][q];
    s_base[tid] = base;
    const int n = hist[tid][p];
    if (n) {
      s_any = 1;
      atomicAdd(&n_out[row0 + tid], n);
      atomicAdd(&tp_out[(row0 + tid) * K + tid], n);
    }
  }
  __syncthreads();
  if (!s_any) return;                          // uniform

  for (int c = 0; c < K; ++c) {
    if (hist[c][p] == 0) continue;
    const int cnt = min(a.counts[row0 + c], L);
    const int32_t* nr = a.notes + (row0 + c) * L * 3;
    int* idx = a.idx + (row0 + c) * L + s_base[c];
    for (int n = tid; n < cnt; n += CS_THREADS)
      if ((double)nr[n * 3 + 1] * a.time_step > (double)nr[n * 3 + 0] * a.time_step && nr[n * 3 + 2] == p)
        idx[atomicAdd(&s_fill[c], 1)] = n;
  }
  __syncthreads();

  // ---- sort by (onset index, note index): every note counts the notes before it
  for (int c = 0; c < K; ++c) {
    const int n_c = hist[c][p];
    const int32_t* nr = a.notes + (row0 + c) * L * 3;
    const int64_t seg = (row0 + c) * L + s_base[c];
    for (int i = tid; i < n_c; i += CS_THREADS) {
      const int ia = a.idx[seg + i];
      const int ka = nr[ia * 3];                 // onset indices order as their seconds do (time_step > 0)
      int rank = 0;
      for (int j = 0; j < n_c; ++j) {
        const int ib = a.idx[seg + j];
        const int kb = nr[ib * 3];
        rank += (kb < ka || (kb == ka && ib < ia)) ? 1 : 0;
      }
      const double on = (double)ka * a.time_step;
      const double off = (double)nr[ia * 3 + 1] * a.time_step;
      a.on[seg + rank] = on;
      a.off[seg + rank] = off;
      const double dur = off - on;
      a.tol[seg + rank] = fmax(a.offset_ratio * dur, a.offset_min_tol);
    }
  }
  __syncthreads();

  // ---- per ordered pair (est i, ref j), a wave each: reset match / stamp, and the interval of estimated notes every reference note
  //      hits by onset: below it they are earlier and miss, above it later and miss
  const int n_pairs = K * (K - 1);
  const int64_t pair0 = (int64_t)b * n_pairs;
  for (int q = tid >> 6; q < n_pairs; q += CS_THREADS / 64) {
    const int i = q / (K - 1), jj = q % (K - 1), j = jj + (jj >= i ? 1 : 0);
    const int ne_p = hist[i][p], nr_p = hist[j][p];
    if (ne_p == 0 || nr_p == 0) continue;
    const int64_t pb = (pair0 + q) * L;
    int* match = a.match + pb + s_base[i];
    int* vis = a.vis + pb + s_base[i];
    for (int e = tid & 63; e < ne_p; e += 64) { match[e] = -1; vis[e] = -1; }
    const double* est_on = a.on + (row0 + i) * L + s_base[i];
    const double* ref_on = a.on + (row0 + j) * L + s_base[j];
    int* lohi = a.lohi + pb + s_base[j];
    for (int u = tid & 63; u < nr_p; u += 64) {
      const double on = ref_on[u];
      int lo = 0, hi = ne_p;
      while (lo < hi) {                          // first e that is not (earlier and a miss)
        const int mid = (lo + hi) >> 1;
        const double eo = est_on[mid];
        if (eo < on && !cs_hit(on, eo, a.onset_tol)) lo = mid + 1; else hi = mid;
      }
      const int first = lo;
      hi = ne_p;
      while (lo < hi) {                          // first e that is later and a miss
        const int mid = (lo + hi) >> 1;
        const double eo = est_on[mid];
        if (eo > on && !cs_hit(on, eo, a.onset_tol)) hi = mid; else lo = mid + 1;
      }
      lohi[u] = first | (lo << 16);
    }
  }
  __syncthreads();

  // ---- match: ordered pair k on one lane, the lanes dealt over the four waves
  const int k = (tid & 63) * (CS_THREADS / 64) + (tid >> 6);
  if (k >= n_pairs) return;
  const int i = k / (K - 1), jj = k % (K - 1), j = jj + (jj >= i ? 1 : 0);
  const int ne_p = hist[i][p], nr_p = hist[j][p];
  if (ne_p == 0 || nr_p == 0) return;
  const bool offsets = a.offset_ratio >= 0.0;
  const int64_t pb = (pair0 + k) * L;
  int* match = a.match + pb + s_base[i];
  int* vis = a.vis + pb + s_base[i];
  int* stk = a.stk + pb + s_base[j];           // level l: reference note | (candidate cursor + 1) << 16
  const int* lohi = a.lohi + pb + s_base[j];
  const int64_t rseg = (row0 + j) * L + s_base[j], eseg = (row0 + i) * L + s_base[i];
  const double* ref_on = a.on + rseg;
  const double* ref_off = a.off + rseg;
  const double* ref_tol = a.tol + rseg;
  const double* est_on = a.on + eseg;
  const double* est_off = a.off + eseg;

  // edge(u, e): e hits u (the interval holds the onset hits; the test is repeated, it is cheap)
  auto edge = [&](int u, int e) -> bool {
    if (!cs_hit(ref_on[u], est_on[e], a.onset_tol)) return false;
    return !offsets || cs_hit(ref_off[u], est_off[e], ref_tol[u]);
  };

  int tp = 0;
  for (int root = 0; root < nr_p; ++root) {
    int sp = 0;
    stk[0] = root;                             // cursor -1: the free candidates have not been looked at yet
    while (sp >= 0) {
      const int u = stk[sp] & 0xffff;
      const int lh = lohi[u];
      const int lo = lh & 0xffff, hi = lh >> 16;
      int c = (stk[sp] >> 16) - 1;
      if (c < 0) {
        int free_e = -1;
        for (int e = lo; e < hi; ++e)
          if (match[e] < 0 && edge(u, e)) { free_e = e; break; }
        if (free_e >= 0) {                     // augment: level l takes the candidate it descended through
          match[free_e] = u;
          for (int l = sp - 1; l >= 0; --l) match[(stk[l] >> 16) - 2] = stk[l] & 0xffff;
          ++tp;
          break;
        }
        c = lo;
      }
      int next = -1;
      while (c < hi) {
        const int e = c++;
        if (vis[e] != root && edge(u, e)) { vis[e] = root; next = e; break; }
      }
      stk[sp] = u | ((c + 1) << 16);
      if (next < 0) { --sp; continue; }
      if (sp + 1 >= nr_p) { --sp; continue; }  // cannot happen: the reference notes of a path are distinct
      ++sp;
      stk[sp] = match[next];
    }
  }
  if (tp) atomicAdd(&tp_out[(row0 + i) * K + j], tp);
}

__global__ __launch_bounds__(64) void cs_select_kernel(const int32_t* __restrict__ tp, const int32_t* __restrict__ n, int K,
                                                       int32_t* __restrict__ chosen, double* __restrict__ utility) {
  __shared__ double s_u[CS_MAXK];
  const int b = blockIdx.x, i = threadIdx.x;
  const int32_t* t = tp + (int64_t)b * K * K;
  const int32_t* nn = n + (int64_t)b * K;
  const bool bad = t[0] < 0;                     // uniform
  if (i < K) {
    double total = 0.0;
    if (!bad) {
      for (int j = 0; j < K; ++j) {
        if (j == i) continue;
        const int both = nn[i] + nn[j];
        const double ag = both == 0 ? 1.0 : (double)(2 * t[i * K + j]) / (double)both;
        total = total + ag;
      }
      total = total / (double)(K - 1);
    }
    s_u[i] = total;
    utility[(int64_t)b * K + i] = total;
  }
  __syncthreads();
  if (i == 0) {
    int best = 0;
    for (int c = 1; c < K; ++c)
      if (s_u[c] > s_u[best]) best = c;
    chosen[b] = bad ? -1 : best;
  }
}

}  // namespace
}  // namespace m2m

// ------------------------------------------------------------------ C ABI ---
using namespace m2m;

// the byte offsets of the workspace arrays for NE = R * L note slots and NP = R * (K - 1) * L pair slots; the total
static int64_t cs_layout(int64_t NE, int64_t NP, int64_t at[8]) {
  const int64_t sizes[8] = {8 * NE, 8 * NE, 8 * NE, 4 * NE, 4 * NP, 4 * NP, 4 * NP, 4 * NP};
  int64_t total = 0;
  for (int i = 0; i < 8; ++i) { at[i] = total; total += align_up(sizes[i], 8); }
  return total;
}

extern "C" int64_t m2m_consensus_workspace_bytes(int R, int L, int K) {
  if (R < 1 || R > M2M_SCORE_MAX_ROWS || L < 1 || L > M2M_SCORE_MAX_TOKENS || K < 2 || K > M2M_CONSENSUS_MAX_CANDIDATES || R % K != 0)
    return -1;
  int64_t at[8];
  return cs_layout((int64_t)R * L, (int64_t)R * (K - 1) * L, at);
}

extern "C" int m2m_consensus_pairwise_counts(const int32_t* notes_dev, const int32_t* counts_dev, int R, int L, int K, double time_step,
                                             double onset_tolerance, double offset_ratio, double offset_min_tolerance,
                                             void* workspace_dev, int64_t workspace_bytes, int32_t* tp_out_dev, int32_t* n_out_dev,
                                             void* stream) {
  const char* who = "m2m_consensus_pairwise_counts";
  // every refusal is made on the arguments alone, before the first HIP call
  M2M_REQUIRE(R >= 1 && R <= M2M_SCORE_MAX_ROWS, "%s: %d rows out of range (1..%d)", who, R, M2M_SCORE_MAX_ROWS);
  M2M_REQUIRE(L >= 1 && L <= M2M_SCORE_MAX_TOKENS, "%s: L=%d out of range (1..%d)", who, L, M2M_SCORE_MAX_TOKENS);
  M2M_REQUIRE(K >= 2 && K <= M2M_CONSENSUS_MAX_CANDIDATES, "%s: %d candidates out of range (2..%d)", who, K,
              M2M_CONSENSUS_MAX_CANDIDATES);
  M2M_REQUIRE(R % K == 0, "%s: %d rows are not whole clips of %d candidates", who, R, K);
  M2M_REQUIRE(time_step > 0.0 && time_step <= 3600.0, "%s: time_step %g out of range (0..3600 s]", who, time_step);
  M2M_REQUIRE(onset_tolerance >= 0.0 && onset_tolerance <= 3600.0, "%s: onset_tolerance %g out of range [0..3600 s]", who,
              onset_tolerance);
  M2M_REQUIRE(offset_ratio == offset_ratio && offset_ratio <= 1e6, "%s: offset_ratio %g out of range (negative: onsets only; at most 1e6)",
              who, offset_ratio);
  M2M_REQUIRE(offset_min_tolerance >= 0.0 && offset_min_tolerance <= 3600.0, "%s: offset_min_tolerance %g out of range [0..3600 s]", who,
              offset_min_tolerance);
  M2M_REQUIRE(notes_dev && counts_dev && tp_out_dev && n_out_dev, "%s: null notes / counts / output", who);
  int64_t at[8];
  const int64_t need = cs_layout((int64_t)R * L, (int64_t)R * (K - 1) * L, at);
  M2M_REQUIRE(workspace_dev && ((uintptr_t)workspace_dev & 7) == 0, "%s: null or misaligned workspace (8 bytes)", who);
  M2M_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes, %lld needed (m2m_consensus_workspace_bytes)", who,
              (long long)workspace_bytes, (long long)need);
  const hipStream_t s = (hipStream_t)stream;
  const int B = R / K;
  M2M_CHECK_HIP(hipMemsetAsync(tp_out_dev, 0, (size_t)B * K * K * sizeof(int32_t), s));
  M2M_CHECK_HIP(hipMemsetAsync(n_out_dev, 0, (size_t)B * K * sizeof(int32_t), s));
  char* w = (char*)workspace_dev;
  CsArgs a;
  a.notes = notes_dev; a.counts = counts_dev;
  a.R = R; a.L = L; a.K = K;
  a.time_step = time_step; a.onset_tol = onset_tolerance; a.offset_ratio = offset_ratio; a.offset_min_tol = offset_min_tolerance;
  a.on = (double*)(w + at[0]); a.off = (double*)(w + at[1]); a.tol = (double*)(w + at[2]); a.idx = (int*)(w + at[3]);
  a.match = (int*)(w + at[4]); a.vis = (int*)(w + at[5]); a.stk = (int*)(w + at[6]); a.lohi = (int*)(w + at[7]);
  hipLaunchKernelGGL(cs_pairwise_kernel, dim3((unsigned)CS_PITCHES, (unsigned)B), dim3(CS_THREADS), 0, s, a, tp_out_dev, n_out_dev);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}

extern "C" int m2m_consensus_select(const int32_t* tp_dev, const int32_t* n_dev, int B, int K, int32_t* chosen_out_dev,
                                    double* utility_out_dev, void* stream) {
  const char* who = "m2m_consensus_select";
  M2M_REQUIRE(B >= 1 && B <= M2M_SCORE_MAX_ROWS, "%s: %d clips out of range (1..%d)", who, B, M2M_SCORE_MAX_ROWS);
  M2M_REQUIRE(K >= 2 && K <= M2M_CONSENSUS_MAX_CANDIDATES, "%s: %d candidates out of range (2..%d)", who, K,
              M2M_CONSENSUS_MAX_CANDIDATES);
  M2M_REQUIRE(tp_dev && n_dev && chosen_out_dev && utility_out_dev, "%s: null counts / output", who);
  M2M_REQUIRE(((uintptr_t)utility_out_dev & 7) == 0, "%s: misaligned utility output (8 bytes)", who);
  hipLaunchKernelGGL(cs_select_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, tp_dev, n_dev, K, chosen_out_dev,
                     utility_out_dev);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}
