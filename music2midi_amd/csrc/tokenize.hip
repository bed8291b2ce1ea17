// Tokenising of note labels for gfx950: the note arrays of a batch -> token ids [B, width] int64, on the device.
// Replaces, for the batches it takes, ref: music2midi/tokenizer.py:86-141 (MidiTokenizer.__call__ / _tokenize); the definition is
// music2midi_amd/tokenizer.py (_quantize, _tokenize), which stays the oracle.  The work is integer placement plus four float64
// operations per note, repeated in the host's order (tk_index): the ids are equal to the host's, not close.
//
// One launch on the caller's stream, nothing returns to the host:
//   notes   one workgroup per clip.  Every note is quantised once; its two time indices go to LDS (16 bit each, one word per note)
//           and raise the onset / offset count of their index (one LDS word per index: onsets low, offsets high).  A block scan over
//           the indices of each group's length - time id, ONSET + its pitches, OFFSET + its pitches - gives every group's base and
//           the row's length.  One thread per index writes the time id and the markers, one thread per note its two pitch ids: the
//           rank inside a group is the number of kept notes before it in the array with the same index, counted over LDS (the host
//           writes a group's pitches in array order).  EOS, the fill and the length follow.  A row longer than `width` is cut inside
//           its row and keeps its true length.
#include "common.h"

#include <math.h>

namespace m2m {
namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_MAX_NOTES = M2M_TOKENIZE_MAX_NOTES;
constexpr int TK_MAX_TIME = M2M_TOKENIZE_MAX_TIME;
constexpr int TK_PER_THREAD = TK_MAX_TIME / TK_THREADS;      // indices one thread scans
constexpr int TK_EOS = 2, TK_ONSET = 3, TK_OFFSET = 4;
constexpr uint32_t TK_DROPPED = 0xFFFFu;                     // the index of a note the cutoff removed (n_time <= 4096)
static_assert(TK_MAX_TIME % TK_THREADS == 0 && TK_MAX_TIME < (int)TK_DROPPED && TK_MAX_NOTES < (1 << 16), "tokenize: LDS word layouts");

// MidiTokenizer._quantize (music2midi_amd/tokenizer.py), float64, one rounded operation per step of the host's expression:
//   steps = seconds / time_step;  steps = rint(nextafter(steps, steps + 1));  min(steps, n_time - 1)
// for seconds >= 0 (the caller has checked).  The next double above a non-negative one is its bit pattern plus one (0 -> the smallest
// subnormal, the largest finite -> inf, inf stays); above 2^53, where steps + 1 == steps and numpy's nextafter returns steps itself,
// both forms clip to n_time - 1.  The minimum is taken in double, before the conversion, so a quotient that overflows still clips.
// No contraction or reassociation may touch these lines, and no reciprocal replaces the division.
#pragma clang fp contract(off)
__host__ __device__ inline int tk_index(double seconds, double time_step, int n_time) {
  const double q = seconds / time_step;
  uint64_t bits;
  __builtin_memcpy(&bits, &q, sizeof bits);
  bits &= 0x7FFFFFFFFFFFFFFFull;                              // -0.0 / +0.0 -> +0.0 (seconds >= 0, time_step > 0)
  if (bits < 0x7FF0000000000000ull) ++bits;
  double up;
  __builtin_memcpy(&up, &bits, sizeof up);
  const double r = rint(up);
  const double top = (double)(n_time - 1);
  return r < top ? (int)r : n_time - 1;
}
// notes[:, 2] + pitch_token_offset in float64, through float32 as the host's id list goes (np.float32 -> np.int64 truncates)
__device__ inline int64_t tk_pitch_id(double pitch, int pitch_offset) { return (int64_t)(float)(pitch + (double)pitch_offset); }
__device__ inline int64_t tk_time_id(int idx, int time_offset) { return (int64_t)(float)((double)idx + (double)time_offset); }

struct TkArgs {
  const double* notes;       // [3][n_notes]: onset s, offset s, pitch
  const int32_t* offsets;    // [B + 1]
  int n_notes, pitch_offset, time_offset, n_time, has_cutoff, labels, width;
  double time_step, cutoff;
  int64_t fill, pad_id, row_stride;
};

// every id of the row goes through here: inside the row only, and with the labels' pad -> -100
__device__ inline void tk_put(int64_t* row, int pos, const TkArgs& a, int64_t id) {
  if (pos < a.width) row[pos] = (a.labels && id == a.pad_id) ? (int64_t)-100 : id;
}

__global__ __launch_bounds__(TK_THREADS) void tk_notes_kernel(TkArgs a, int64_t* __restrict__ ids, int32_t* __restrict__ lengths) {
  __shared__ uint32_t note_idx[TK_MAX_NOTES];   // onset index | offset index << 16; TK_DROPPED in both for a dropped note
  __shared__ uint32_t count[TK_MAX_TIME];       // per time index: notes starting there | notes ending there << 16
  __shared__ int base[TK_MAX_TIME];             // per time index: where its group starts in the row
  __shared__ int scan[TK_THREADS];
  __shared__ int s_bad;

  const int r = blockIdx.x, tid = threadIdx.x;
  int64_t* row = ids + (int64_t)r * a.row_stride;
  const int lo = a.offsets[r], hi = a.offsets[r + 1];
  const int n = hi - lo;
  if (tid == 0) s_bad = (lo < 0 || hi > a.n_notes || n < 0 || n > TK_MAX_NOTES) ? 1 : 0;
  for (int i = tid; i < a.n_time; i += TK_THREADS) count[i] = 0;
  __syncthreads();
  const bool readable = !s_bad;                 // uniform: the note loops below run only over [lo, hi) inside the packed array
  __syncthreads();
  const double* on_s = a.notes + lo;
  const double* off_s = a.notes + (int64_t)a.n_notes + lo;
  const double* pitch = a.notes + 2 * (int64_t)a.n_notes + lo;

  if (readable) {
    bool bad = false;
    for (int j = tid; j < n; j += TK_THREADS) {
      const double on = on_s[j], off = off_s[j], p = pitch[j];
      // (comparisons that are false for a NaN: a value the host would not place either)
      if (!(on >= 0.0 && on <= 1.79769313486231570e308 && fabs(off) <= 1.79769313486231570e308 && fabs(p) <= 32768.0)) {
        bad = true;
        continue;
      }
      uint32_t word = TK_DROPPED | (TK_DROPPED << 16);
      if (!a.has_cutoff || on < a.cutoff) {
        const double least = on + a.time_step;                 // every note lasts at least one step
        const int oi = tk_index(on, a.time_step, a.n_time);
        const int fi = tk_index(off > least ? off : least, a.time_step, a.n_time);
        atomicAdd(&count[oi], 1u);
        atomicAdd(&count[fi], 1u << 16);
        word = (uint32_t)oi | ((uint32_t)fi << 16);
      }
      note_idx[j] = word;
    }
    if (bad) s_bad = 1;
  }
  __syncthreads();
  if (s_bad) {                                  // uniform: the whole row is fill, the length says why
    for (int pos = tid; pos < a.width; pos += TK_THREADS) tk_put(row, pos, a, a.fill);
    if (tid == 0) lengths[r] = -1;
    return;
  }

  // group lengths: thread t owns indices [16 t, 16 t + 16)
  const int first = tid * TK_PER_THREAD;
  int mine = 0;
#pragma unroll
  for (int k = 0; k < TK_PER_THREAD; ++k) {
    const int i = first + k;
    if (i < a.n_time) {
      const uint32_t c = count[i];
      const int on = (int)(c & 0xFFFFu), off = (int)(c >> 16);
      mine += ((on | off) ? 1 : 0) + (on ? 1 + on : 0) + (off ? 1 + off : 0);
    }
  }
  scan[tid] = mine;
  __syncthreads();
  for (int s = 1; s < TK_THREADS; s <<= 1) {
    const int v = tid >= s ? scan[tid - s] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  const int total = scan[TK_THREADS - 1] + 1;   // + EOS; at most 6 * 1024 + 1
  int pos = scan[tid] - mine;
#pragma unroll
  for (int k = 0; k < TK_PER_THREAD; ++k) {
    const int i = first + k;
    if (i < a.n_time) {
      base[i] = pos;
      const uint32_t c = count[i];
      const int on = (int)(c & 0xFFFFu), off = (int)(c >> 16);
      if (on | off) {
        tk_put(row, pos, a, tk_time_id(i, a.time_offset));
        if (on) tk_put(row, pos + 1, a, (int64_t)TK_ONSET);
        if (off) tk_put(row, pos + 1 + (on ? 1 + on : 0), a, (int64_t)TK_OFFSET);
        pos += 1 + (on ? 1 + on : 0) + (off ? 1 + off : 0);
      }
    }
  }
  __syncthreads();

  // pitch ids: a note's rank in its onset group and in its offset group is counted over the kept notes before it
  for (int j = tid; j < n; j += TK_THREADS) {
    const uint32_t word = note_idx[j];
    const uint32_t oi = word & 0xFFFFu, fi = word >> 16;
    if (oi == TK_DROPPED) continue;
    int rank_on = 0, rank_off = 0;
    for (int jj = 0; jj < j; ++jj) {
      const uint32_t w = note_idx[jj];
      rank_on += (w & 0xFFFFu) == oi;
      rank_off += (w >> 16) == fi;
    }
    const int64_t id = tk_pitch_id(pitch[j], a.pitch_offset);
    tk_put(row, base[oi] + 2 + rank_on, a, id);
    const int on_there = (int)(count[fi] & 0xFFFFu);
    tk_put(row, base[fi] + 1 + (on_there ? 1 + on_there : 0) + 1 + rank_off, a, id);
  }

  if (tid == 0) {
    tk_put(row, total - 1, a, (int64_t)TK_EOS);
    lengths[r] = total;
  }
  for (int p = total + tid; p < a.width; p += TK_THREADS) tk_put(row, p, a, a.fill);
}

}  // namespace
}  // namespace m2m

// ------------------------------------------------------------------ C ABI ---
using namespace m2m;

extern "C" int m2m_tokenize_quantize(double seconds, double time_step, int n_time) {
  if (!(seconds >= 0.0) || !(time_step > 0.0 && time_step <= 3600.0) || n_time < 1 || n_time > M2M_TOKENIZE_MAX_TIME) return -1;
  return tk_index(seconds, time_step, n_time);
}

extern "C" int64_t m2m_tokenize_row_bound(int n_notes, int n_time) {
  if (n_notes < 0 || n_time < 1) return -1;
  const int64_t k = n_notes, T = n_time;
  const int64_t groups = 2 * k < T ? 2 * k : T, marked = k < T ? k : T;
  return 1 + 2 * k + groups + 2 * marked;
}

extern "C" int m2m_tokenize_notes(const double* notes_dev, const int32_t* offsets_dev, int n_notes, int B, double time_step,
                                  int pitch_offset, int time_offset, int n_time, int has_cutoff, double cutoff_time, int64_t fill,
                                  int labels, int64_t pad_id, int64_t* ids_out_dev, int width, int64_t row_stride,
                                  int32_t* lengths_out_dev, void* stream) {
  // every refusal is made on the arguments alone, before the first HIP call
  M2M_REQUIRE(B >= 1 && B <= M2M_TOKENIZE_MAX_ROWS, "m2m_tokenize_notes: %d clips out of range (1..%d)", B, M2M_TOKENIZE_MAX_ROWS);
  M2M_REQUIRE(n_notes >= 0 && (int64_t)n_notes <= (int64_t)B * M2M_TOKENIZE_MAX_NOTES,
              "m2m_tokenize_notes: %d notes out of range (0..%d per clip)", n_notes, M2M_TOKENIZE_MAX_NOTES);
  M2M_REQUIRE(time_step > 0.0 && time_step <= 3600.0, "m2m_tokenize_notes: time_step %g out of range (0..3600 s]", time_step);
  M2M_REQUIRE(n_time >= 1 && n_time <= M2M_TOKENIZE_MAX_TIME, "m2m_tokenize_notes: %d time ids out of range (1..%d)", n_time,
              M2M_TOKENIZE_MAX_TIME);
  M2M_REQUIRE(pitch_offset >= 5, "m2m_tokenize_notes: pitch_offset %d below the 5 special ids", pitch_offset);
  M2M_REQUIRE(time_offset >= pitch_offset && time_offset <= (1 << 30), "m2m_tokenize_notes: time_offset %d out of range (%d..2^30)",
              time_offset, pitch_offset);
  M2M_REQUIRE(has_cutoff == 0 || has_cutoff == 1, "m2m_tokenize_notes: has_cutoff must be 0 or 1");
  M2M_REQUIRE(labels == 0 || labels == 1, "m2m_tokenize_notes: labels must be 0 or 1");
  M2M_REQUIRE(width >= 1, "m2m_tokenize_notes: width %d below 1", width);
  M2M_REQUIRE(row_stride >= width, "m2m_tokenize_notes: row stride %lld below width %d", (long long)row_stride, width);
  M2M_REQUIRE(notes_dev && offsets_dev && ids_out_dev && lengths_out_dev, "m2m_tokenize_notes: null notes / offsets / ids / lengths");
  TkArgs a;
  a.notes = notes_dev; a.offsets = offsets_dev; a.n_notes = n_notes; a.pitch_offset = pitch_offset; a.time_offset = time_offset;
  a.n_time = n_time; a.has_cutoff = has_cutoff; a.labels = labels; a.width = width; a.time_step = time_step;
  a.cutoff = has_cutoff ? cutoff_time : 0.0; a.fill = fill; a.pad_id = pad_id; a.row_stride = row_stride;
  hipLaunchKernelGGL(tk_notes_kernel, dim3((unsigned)B), dim3(TK_THREADS), 0, (hipStream_t)stream, a, ids_out_dev, lengths_out_dev);
  M2M_CHECK_HIP(hipGetLastError());
  return M2M_OK;
}
