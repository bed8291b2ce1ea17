// Training augmentation for gfx950: peak normalisation + pitch shift of a waveform batch, on the device.
// Replaces ref: music2midi/dataset.py:131-133,157-160 (librosa.util.normalize, librosa.effects.pitch_shift); the definition is
// music2midi_amd/audio.py (normalize, pitch_shift), which stays the oracle.
//
// Six launches per call (a chunk of up to 1024 clips), all on the caller's stream, nothing returns to the host:
//   peak      max |y| of every clip whose normalise flag is set                                   grid (clips)
//   stft      zero-padded centred frames x periodic Hann -> real FFT-2048 -> S [clip][frame][1025]   grid (frames, clips)
//   vocoder   one thread per (clip, bin) walks the stretched frames: linear magnitude, phase as a unit phasor
//             multiplied by unit(b) conj(unit(a)) and renormalised each step -> P [clip][frame'][1025]  grid (ceil(1025/128), clips)
//   istft     inverse real FFT-2048 x Hann of every stretched frame, IN PLACE over its row of P      grid (frames', clips)
//   ola       gather: every stretched sample sums its <= 4 covering frames / summed squared window     grid (ceil(len'/256), clips)
//   resample  out[n] = sum_m x[m] h[n down - m up + half_len], zero beyond; step 0: the (normalised) copy  grid (ceil(T/256), clips)
// Clips of a batch have different steps, hence different stretched extents: grids are sized for the batch's largest and workgroups
// beyond a clip's own extent return before touching memory.  Every value depends on its own clip only (batch invariance).
//
// The real FFT-2048 is a complex FFT-1024 of z[n] = x[2n] + i x[2n+1] (radix-4 Stockham autosort in LDS, 256 threads, one butterfly
// per thread and pass) plus the split of pairs (k, 1024 - k); the inverse runs the same forward transform on the conjugate.
#include "common.h"

#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace m2m {
namespace {

constexpr int AG_NFFT = 2048;
constexpr int AG_HALF = 1024;          // complex FFT length
constexpr int AG_HOP = 512;
constexpr int AG_BINS = 1025;
constexpr int AG_THREADS = 256;
constexpr int AG_NSTEP = 2 * M2M_AUGMENT_MAX_STEP + 1;
constexpr int AG_CHUNK = 1024;         // clips per launch: their step / flag bytes travel as kernel arguments

struct AugStep {       // what one semitone step means for clips of T samples
  double rate;         // 2^(-step/12)
  int fs;              // stretched frames
  int len;             // stretched samples
  int up, down, half;  // resampling ratio, filter half length
  int n_out;           // min(T, ceil(len up / down)): samples the resampler writes, zero beyond
  int filt;            // offset of the step's filter in the table blob (floats)
};
struct AugArgs {
  AugStep st[AG_NSTEP];
  unsigned char code[AG_CHUNK];   // per clip: (step + 12) | normalise << 7
  int T, F;
};
struct AugTables {
  const float* window;    // [2048]
  const float2* tw1024;   // [1024] exp(-2 pi i k / 1024)
  const float2* tw2048;   // [1024] exp(-2 pi i k / 2048)
  const float* filt;      // every step's filter, AugStep::filt apart
};

__device__ inline float2 ag_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ inline float2 ag_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ inline float2 ag_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ inline float2 ag_conj(float2 a) { return make_float2(a.x, -a.y); }

// Forward complex FFT-1024 of z (LDS, natural order in and out) by all 256 threads: Stockham autosort, radix 4, five passes.
// Pass Ns in 1, 4, .. 256: thread j takes z[j + 256 r], twiddles them by W_(4 Ns)^(r (j mod Ns)) and writes the 4-point DFT to
// (j div Ns) 4 Ns + (j mod Ns) + r Ns.
__device__ inline void ag_fft1024(float2* z, const float2* __restrict__ tw1024, int tid) {
#pragma unroll
  for (int Ns = 1; Ns < AG_HALF; Ns *= 4) {
    const int k = tid & (Ns - 1);
    float2 v0 = z[tid], v1 = z[tid + 256], v2 = z[tid + 512], v3 = z[tid + 768];
    if (Ns > 1) {
      const int ts = k * (256 / Ns);
      v1 = ag_mul(v1, tw1024[ts]);
      v2 = ag_mul(v2, tw1024[2 * ts]);
      v3 = ag_mul(v3, tw1024[3 * ts]);
    }
    const float2 s02 = ag_add(v0, v2), d02 = ag_sub(v0, v2), s13 = ag_add(v1, v3), e13 = ag_sub(v1, v3);
    const float2 d13 = make_float2(e13.y, -e13.x);   // -i (v1 - v3)
    __syncthreads();
    const int j0 = ((tid - k) << 2) + k;
    z[j0] = ag_add(s02, s13);
    z[j0 + Ns] = ag_add(d02, d13);
    z[j0 + 2 * Ns] = ag_sub(s02, s13);
    z[j0 + 3 * Ns] = ag_sub(d02, d13);
    __syncthreads();
  }
}

// |y| maximum that keeps a NaN once seen (np.abs(y).max() is NaN then, and the clip becomes NaN as on the host)
__device__ inline float ag_nanmax(float m, float a) { return (a > m || a != a) ? a : m; }

__global__ __launch_bounds__(1024) void ag_peak_kernel(const float* __restrict__ wav, AugArgs a, float* __restrict__ peaks) {
  const int b = blockIdx.x;
  if (!(a.code[b] & 0x80)) return;                       // uniform
  __shared__ float red[1024];
  const float* w = wav + (int64_t)b * a.T;
  float m = 0.f;
  for (int i = threadIdx.x; i < a.T; i += 1024) m = ag_nanmax(m, fabsf(w[i]));
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 512; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = ag_nanmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) peaks[b] = red[0];
}

// sample i of clip b as the later stages see it: divided by the clip's peak when the flag is set and the peak is a normal number
__device__ inline float ag_sample(const float* w, int i, bool norm, float peak) {
  const float v = w[i];
  return norm ? v / peak : v;
}

__global__ __launch_bounds__(AG_THREADS) void ag_stft_kernel(const float* __restrict__ wav, AugArgs a, AugTables tb,
                                                             const float* __restrict__ peaks, float2* __restrict__ S) {
  const int b = blockIdx.y, f = blockIdx.x, tid = threadIdx.x;
  const int code = a.code[b];
  if ((code & 0x7F) == M2M_AUGMENT_MAX_STEP) return;      // step 0: a copy, no transform (uniform)
  __shared__ float2 z[AG_HALF];
  const int T = a.T;
  const float* w = wav + (int64_t)b * T;
  float peak = 1.f;
  bool norm = (code & 0x80) != 0;
  if (norm) { peak = peaks[b]; norm = !(peak < FLT_MIN); }
  const int base = f * AG_HOP - AG_NFFT / 2;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = tid + 256 * j, i0 = base + 2 * n, i1 = i0 + 1;
    const float x0 = (i0 >= 0 && i0 < T) ? ag_sample(w, i0, norm, peak) : 0.f;
    const float x1 = (i1 >= 0 && i1 < T) ? ag_sample(w, i1, norm, peak) : 0.f;
    z[n] = make_float2(x0 * tb.window[2 * n], x1 * tb.window[2 * n + 1]);
  }
  __syncthreads();
  ag_fft1024(z, tb.tw1024, tid);
  // split: X[k] = E + W2048^k O, X[1024 - k] = conj(E - W2048^k O) with E, O the transforms of the even / odd samples
  float2* row = S + ((int64_t)b * a.F + f) * AG_BINS;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = tid + 256 * j;
    const float2 zk = z[k], c = ag_conj(z[(AG_HALF - k) & (AG_HALF - 1)]);
    const float2 e = make_float2(0.5f * (zk.x + c.x), 0.5f * (zk.y + c.y));
    const float2 d = make_float2(0.5f * (zk.x - c.x), 0.5f * (zk.y - c.y));
    const float2 t = ag_mul(tb.tw2048[k], make_float2(d.y, -d.x));   // W^k (d / i)
    row[k] = ag_add(e, t);
    row[AG_HALF - k] = ag_conj(ag_sub(e, t));
  }
  if (tid == 0) row[512] = ag_conj(z[512]);               // E = Re Z, O = Im Z, W2048^512 = -i
}

// z = |z| u with u a unit phasor; unit(0) = 1 as np.angle(0) = 0.  Scaled by the larger component: no overflow or underflow of |z|^2.
__device__ inline void ag_polar(float2 v, float2* u, float* mag) {
  const float m = fmaxf(fabsf(v.x), fabsf(v.y));
  if (!(m > 0.f)) { *u = make_float2(1.f, 0.f); *mag = (m == m) ? 0.f : m; return; }
  const float xs = v.x / m, ys = v.y / m;
  const float r = sqrtf(xs * xs + ys * ys);
  *u = make_float2(xs / r, ys / r);
  *mag = m * r;
}

__global__ __launch_bounds__(128) void ag_vocoder_kernel(const float2* __restrict__ S, AugArgs a, float2* __restrict__ P) {
  const int b = blockIdx.y, k = blockIdx.x * 128 + threadIdx.x;
  const int si = a.code[b] & 0x7F;
  if (si == M2M_AUGMENT_MAX_STEP || k >= AG_BINS) return;
  const int F = a.F, FS = a.st[si].fs;
  const double rate = a.st[si].rate;
  const float2* s = S + (int64_t)b * F * AG_BINS + k;
  float2* p = P + (int64_t)b * (2 * F) * AG_BINS + k;
  float2 ph;
  float m0;
  ag_polar(s[0], &ph, &m0);
  for (int t = 0; t < FS; ++t) {
    // np.arange(0, F, rate)[t] is the float64 product t * rate; an fp32 one can land across an integer and pick another frame pair
    const double st = (double)t * rate;
    const int kk = (int)st;
    const float alpha = (float)(st - (double)kk);
    const float2 va = (kk < F) ? s[(int64_t)kk * AG_BINS] : make_float2(0.f, 0.f);
    const float2 vb = (kk + 1 < F) ? s[(int64_t)(kk + 1) * AG_BINS] : make_float2(0.f, 0.f);
    float2 ua, ub;
    float ma, mb;
    ag_polar(va, &ua, &ma);
    ag_polar(vb, &ub, &mb);
    const float mag = (1.0f - alpha) * ma + alpha * mb;
    p[(int64_t)t * AG_BINS] = make_float2(mag * ph.x, mag * ph.y);
    // acc += omega + wrap(angle(b) - angle(a) - omega)  ==  acc + angle(b) - angle(a)  (mod 2 pi): no growing fp32 angle
    ph = ag_mul(ph, ag_mul(ub, ag_conj(ua)));
    const float inv = 1.0f / sqrtf(ph.x * ph.x + ph.y * ph.y);
    ph = make_float2(ph.x * inv, ph.y * inv);
  }
}

// inverse real FFT-2048 of row t of P (the imaginary parts of bins 0 and 1024 are ignored, as np.fft.irfft does), times the window,
// written as 2048 floats over the same row (every bin is in LDS before the first store)
__global__ __launch_bounds__(AG_THREADS) void ag_istft_kernel(float2* __restrict__ P, AugArgs a, AugTables tb) {
  const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
  const int si = a.code[b] & 0x7F;
  if (si == M2M_AUGMENT_MAX_STEP || t >= a.st[si].fs) return;     // uniform
  __shared__ float2 z[AG_HALF];
  float2* row = P + ((int64_t)b * (2 * a.F) + t) * AG_BINS;
  // Z[k] = E + i O, Z[1024 - k] = conj(E) + i conj(O), E = (X[k] + conj X[1024 - k]) / 2, O = (X[k] - conj X[1024 - k]) / 2 W2048^-k;
  // the forward transform of conj(Z) is the conjugate of the inverse one
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = tid + 256 * j;
    float2 xk = row[k], xn = row[AG_HALF - k];
    if (k == 0) { xk.y = 0.f; xn.y = 0.f; }
    const float2 c = ag_conj(xn);
    const float2 e = make_float2(0.5f * (xk.x + c.x), 0.5f * (xk.y + c.y));
    const float2 d = make_float2(0.5f * (xk.x - c.x), 0.5f * (xk.y - c.y));
    const float2 o = ag_mul(d, ag_conj(tb.tw2048[k]));
    const float2 zk = make_float2(e.x - o.y, e.y + o.x);            // E + i O
    const float2 zn = make_float2(e.x + o.y, -e.y + o.x);           // conj(E) + i conj(O)
    z[k] = ag_conj(zk);
    if (k > 0) z[AG_HALF - k] = ag_conj(zn);
  }
  if (tid == 0) z[512] = row[512];                                  // Z[512] = conj(X[512]), stored conjugated
  __syncthreads();
  ag_fft1024(z, tb.tw1024, tid);
  float* orow = reinterpret_cast<float*>(row);
  const float sc = 1.0f / AG_HALF;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = tid + 256 * j;
    const float2 y = z[n];
    *reinterpret_cast<float2*>(orow + 2 * n) = make_float2(y.x * sc * tb.window[2 * n], -y.y * sc * tb.window[2 * n + 1]);
  }
}

// overlap-add as a gather + window normalisation + trim of the first 1024 samples
__global__ __launch_bounds__(AG_THREADS) void ag_ola_kernel(const float2* __restrict__ P, AugArgs a, AugTables tb, float* __restrict__ W) {
  const int b = blockIdx.y;
  const int n = blockIdx.x * AG_THREADS + threadIdx.x;
  const int si = a.code[b] & 0x7F;
  if (si == M2M_AUGMENT_MAX_STEP || n >= a.st[si].len) return;
  const int FS = a.st[si].fs;
  const float* fr = reinterpret_cast<const float*>(P + (int64_t)b * (2 * a.F) * AG_BINS);   // frame i at fr + i * 2050
  const int p = n + AG_NFFT / 2;
  const int lo = p < AG_NFFT ? 0 : (p - (AG_NFFT - AG_HOP)) / AG_HOP;
  const int hi = min(p / AG_HOP, FS - 1);
  float acc = 0.f, nrm = 0.f;
  for (int i = lo; i <= hi; ++i) {
    const int j = p - i * AG_HOP;
    const float wv = tb.window[j];
    acc += fr[(int64_t)i * (2 * AG_BINS) + j];
    nrm += wv * wv;
  }
  W[(int64_t)b * (2 * a.T) + n] = nrm > 1e-10f ? acc / nrm : acc;
}

__global__ __launch_bounds__(AG_THREADS) void ag_resample_kernel(const float* __restrict__ wav, const float* __restrict__ W, AugArgs a,
                                                                 AugTables tb, const float* __restrict__ peaks, float* __restrict__ out) {
  const int b = blockIdx.y;
  const int n = blockIdx.x * AG_THREADS + threadIdx.x;
  const int T = a.T;
  if (n >= T) return;
  const int code = a.code[b], si = code & 0x7F;
  float* o = out + (int64_t)b * T;
  if (si == M2M_AUGMENT_MAX_STEP) {
    float peak = 1.f;
    bool norm = (code & 0x80) != 0;
    if (norm) { peak = peaks[b]; norm = !(peak < FLT_MIN); }
    o[n] = ag_sample(wav + (int64_t)b * T, n, norm, peak);
    return;
  }
  const AugStep& st = a.st[si];
  if (n >= st.n_out) { o[n] = 0.f; return; }
  const float* x = W + (int64_t)b * (2 * T);
  const float* h = tb.filt + st.filt;
  const int64_t c = (int64_t)n * st.down, up = st.up, half = st.half;
  // taps 0 <= c - m up + half <= 2 half
  const int64_t lo64 = c - half <= 0 ? 0 : (c - half + up - 1) / up;
  const int64_t hi64 = (c + half) / up;
  const int lo = (int)lo64, hi = (int)(hi64 < st.len - 1 ? hi64 : st.len - 1);
  float acc = 0.f;
  for (int m = lo; m <= hi; ++m) acc = fmaf(x[m], h[c + half - (int64_t)m * up], acc);
  o[n] = acc;
}

// ------------------------------------------------------------------ host arithmetic (no device)
double ag_rate(int step) { return pow(2.0, -(double)step / 12.0); }

// fractions.Fraction(rate).limit_denominator(1000), exactly: the double is n / d with d a power of two
void ag_ratio(double rate, int* up, int* down) {
  int e = 0;
  const double mant = frexp(rate, &e);                          // rate = mant 2^e, 0.5 <= mant < 1; rate in [0.5, 2]: e in 0..2
  typedef __int128 i128;
  i128 n = (i128)ldexp(mant, 53), d = (i128)1 << (53 - e);
  const i128 N = n, D = d;
  const int64_t maxd = 1000;
  int64_t p0 = 0, q0 = 1, p1 = 1, q1 = 0;
  while (true) {
    const i128 aq = n / d;
    const i128 q2 = q0 + aq * q1;
    if (q2 > maxd) break;
    const int64_t np = (int64_t)(p0 + aq * p1);
    p0 = p1; q0 = q1; p1 = np; q1 = (int64_t)q2;
    const i128 r = n - aq * d;
    n = d; d = r;
    if (d == 0) break;
  }
  if (d == 0) { *up = (int)p1; *down = (int)q1; return; }   // the double itself has a denominator <= 1000 (0.5, 1, 2)
  const int64_t k = (maxd - q0) / q1;
  const int64_t b1p = p0 + k * p1, b1q = q0 + k * q1, b2p = p1, b2q = q1;
  // |b2 - x| <= |b1 - x|  with x = N / D
  i128 e2 = (i128)b2p * D - N * b2q, e1 = (i128)b1p * D - N * b1q;
  if (e2 < 0) e2 = -e2;
  if (e1 < 0) e1 = -e1;
  if (e2 * b1q <= e1 * b2q) { *up = (int)b2p; *down = (int)b2q; }
  else { *up = (int)b1p; *down = (int)b1q; }
}

double ag_i0(double x) {          // modified Bessel function of the first kind, order 0: power series (x <= 5 here)
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

// up * scipy.signal.firwin(2 half + 1, 1 / max(up, down), window=("kaiser", 5.0)) in fp32, as resample_poly builds it for fp32 input
void ag_design(int up, int down, std::vector<float>* h) {
  const int mx = up > down ? up : down, half = 10 * mx, taps = 2 * half + 1;
  const double fc = 1.0 / mx, alpha = 0.5 * (taps - 1), i0b = ag_i0(5.0);
  std::vector<double> hd(taps);
  double s = 0.0;
  for (int i = 0; i < taps; ++i) {
    const double m = i - alpha, y = M_PI * fc * m;
    const double sinc = (m == 0.0) ? 1.0 : sin(y) / y;
    const double r = m / alpha;
    const double arg = 1.0 - r * r;
    const double win = ag_i0(5.0 * sqrt(arg > 0.0 ? arg : 0.0)) / i0b;
    hd[i] = fc * sinc * win;
    s += hd[i];
  }
  h->resize(taps);
  for (int i = 0; i < taps; ++i) (*h)[i] = (float)(hd[i] / s) * (float)up;
}

int ag_plan(int T, int step, m2m_augment_plan_t* p) {
  memset(p, 0, sizeof(*p));
  const int F = 1 + T / AG_HOP;
  p->frames = F;
  p->cap_frames = 2 * F;
  p->cap_len = 2 * T;
  if (step == 0) { p->stretched_frames = F; p->stretched_len = T; p->up = p->down = 1; return M2M_OK; }
  const double rate = ag_rate(step);
  p->stretched_frames = (int)ceil((double)F / rate);        // len(np.arange(0, F, rate))
  p->stretched_len = (int)nearbyint((double)T / rate);      // Python's round: half to even
  ag_ratio(rate, &p->up, &p->down);
  p->taps = 20 * (p->up > p->down ? p->up : p->down) + 1;
  return M2M_OK;
}

}  // namespace
}  // namespace m2m

// ------------------------------------------------------------------ C ABI ---
using namespace m2m;

struct m2m_augment {
  void* dev_blob = nullptr;     // window | tw1024 | tw2048 | filters
  AugTables dev;
  int filt_off[AG_NSTEP];       // floats into the filter part of the blob, by step + 12
  int up[AG_NSTEP], down[AG_NSTEP];
};

extern "C" int m2m_augment_create(m2m_augment** out) {
  M2M_REQUIRE(out, "m2m_augment_create: null argument");
  m2m_augment* a = new m2m_augment();
  std::vector<float> filt;
  for (int i = 0; i < AG_NSTEP; ++i) {
    const int step = i - M2M_AUGMENT_MAX_STEP;
    a->filt_off[i] = (int)filt.size();
    a->up[i] = a->down[i] = 1;
    if (step == 0) continue;
    ag_ratio(ag_rate(step), &a->up[i], &a->down[i]);
    std::vector<float> h;
    ag_design(a->up[i], a->down[i], &h);
    filt.insert(filt.end(), h.begin(), h.end());
  }
  std::vector<float> win(AG_NFFT);
  std::vector<float2> tw1(AG_HALF), tw2(AG_HALF);
  for (int n = 0; n < AG_NFFT; ++n) win[n] = (float)(0.5 - 0.5 * cos(2.0 * M_PI * n / AG_NFFT));
  for (int k = 0; k < AG_HALF; ++k) {
    const double a1 = -2.0 * M_PI * k / 1024.0, a2 = -2.0 * M_PI * k / 2048.0;
    tw1[k] = make_float2((float)cos(a1), (float)sin(a1));
    tw2[k] = make_float2((float)cos(a2), (float)sin(a2));
  }
  const size_t o_win = 0, o_tw1 = o_win + AG_NFFT * sizeof(float), o_tw2 = o_tw1 + AG_HALF * sizeof(float2),
               o_f = o_tw2 + AG_HALF * sizeof(float2), total = o_f + filt.size() * sizeof(float);
  std::vector<unsigned char> host(total);
  memcpy(host.data() + o_win, win.data(), AG_NFFT * sizeof(float));
  memcpy(host.data() + o_tw1, tw1.data(), AG_HALF * sizeof(float2));
  memcpy(host.data() + o_tw2, tw2.data(), AG_HALF * sizeof(float2));
  memcpy(host.data() + o_f, filt.data(), filt.size() * sizeof(float));
  hipError_t e = hipMalloc(&a->dev_blob, total);
  if (e == hipSuccess) e = hipMemcpy(a->dev_blob, host.data(), total, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    set_error("m2m_augment_create: device allocation/copy failed: %s", hipGetErrorString(e));
    if (a->dev_blob) (void)hipFree(a->dev_blob);
    delete a;
    return M2M_ERR_HIP;
  }
  unsigned char* base = (unsigned char*)a->dev_blob;
  a->dev.window = (const float*)(base + o_win);
  a->dev.tw1024 = (const float2*)(base + o_tw1);
  a->dev.tw2048 = (const float2*)(base + o_tw2);
  a->dev.filt = (const float*)(base + o_f);
  *out = a;
  return M2M_OK;
}

extern "C" void m2m_augment_destroy(m2m_augment* a) {
  if (!a) return;
  if (a->dev_blob) (void)hipFree(a->dev_blob);
  delete a;
}

extern "C" int m2m_augment_plan(const m2m_augment* a, int T, int step, m2m_augment_plan_t* out) {
  (void)a;
  M2M_REQUIRE(out, "m2m_augment_plan: null argument");
  M2M_REQUIRE(T >= 1 && T <= M2M_AUGMENT_MAX_SAMPLES, "m2m_augment_plan: T=%d out of range (1..%d)", T, M2M_AUGMENT_MAX_SAMPLES);
  M2M_REQUIRE(step >= -M2M_AUGMENT_MAX_STEP && step <= M2M_AUGMENT_MAX_STEP, "m2m_augment_plan: step %d out of range (|step| <= %d)", step,
              M2M_AUGMENT_MAX_STEP);
  return ag_plan(T, step, out);
}

extern "C" int m2m_augment_filter(int step, float* out_host, int n) {
  M2M_REQUIRE(step >= -M2M_AUGMENT_MAX_STEP && step <= M2M_AUGMENT_MAX_STEP, "m2m_augment_filter: step %d out of range (|step| <= %d)", step,
              M2M_AUGMENT_MAX_STEP);
  M2M_REQUIRE(n >= 0 && (out_host || n == 0), "m2m_augment_filter: bad buffer");
  if (step == 0) return 0;
  int up = 1, down = 1;
  ag_ratio(ag_rate(step), &up, &down);
  std::vector<float> h;
  ag_design(up, down, &h);
  const int taps = (int)h.size();
  if (n > 0) memcpy(out_host, h.data(), (size_t)(n < taps ? n : taps) * sizeof(float));
  return taps;
}

// workspace: peaks [B] | S [B][F][1025] complex | P [B][2F][1025] complex | W [B][2T]
namespace {
struct AugLayout { int64_t peaks, S, P, W, total; };
AugLayout ag_layout(int B, int T) {
  const int64_t F = 1 + T / AG_HOP;
  AugLayout l;
  l.peaks = 0;
  l.S = align_up((int64_t)B * (int64_t)sizeof(float), 256);
  l.P = l.S + align_up((int64_t)B * F * AG_BINS * (int64_t)sizeof(float2), 256);
  l.W = l.P + align_up((int64_t)B * 2 * F * AG_BINS * (int64_t)sizeof(float2), 256);
  l.total = l.W + align_up((int64_t)B * 2 * T * (int64_t)sizeof(float), 256);
  return l;
}
}  // namespace

extern "C" int64_t m2m_augment_workspace_bytes(int B, int T) {
  M2M_REQUIRE(B >= 1 && B <= 65535, "m2m_augment_workspace_bytes: batch %d out of range (1..65535)", B);
  M2M_REQUIRE(T >= 1 && T <= M2M_AUGMENT_MAX_SAMPLES, "m2m_augment_workspace_bytes: T=%d out of range (1..%d)", T, M2M_AUGMENT_MAX_SAMPLES);
  return ag_layout(B, T).total;
}

extern "C" int m2m_pitch_shift_f32(const m2m_augment* a, const float* wav_dev, int B, int T, const int* steps_host,
                                   const unsigned char* normalize_host, float* out_dev, void* workspace_dev,
                                   const m2m_augment_stages* stages, void* stream) {
  // the limits first: they are checked on the arguments alone (no handle, no device)
  M2M_REQUIRE(B >= 1 && B <= 65535, "m2m_pitch_shift_f32: batch %d out of range (1..65535)", B);
  M2M_REQUIRE(T >= 1 && T <= M2M_AUGMENT_MAX_SAMPLES, "m2m_pitch_shift_f32: T=%d out of range (1..%d)", T, M2M_AUGMENT_MAX_SAMPLES);
  M2M_REQUIRE(steps_host, "m2m_pitch_shift_f32: null steps");
  for (int b = 0; b < B; ++b)
    M2M_REQUIRE(steps_host[b] >= -M2M_AUGMENT_MAX_STEP && steps_host[b] <= M2M_AUGMENT_MAX_STEP,
                "m2m_pitch_shift_f32: step %d of clip %d out of range (|step| <= %d)", steps_host[b], b, M2M_AUGMENT_MAX_STEP);
  M2M_REQUIRE(wav_dev && out_dev, "m2m_pitch_shift_f32: null waveform / output");
  {
    const uintptr_t w0 = (uintptr_t)wav_dev, o0 = (uintptr_t)out_dev, bytes = (uintptr_t)B * (uintptr_t)T * sizeof(float);
    M2M_REQUIRE(o0 + bytes <= w0 || w0 + bytes <= o0, "m2m_pitch_shift_f32: out_dev overlaps wav_dev (the stages read the input after writing)");
  }
  M2M_REQUIRE(a && workspace_dev, "m2m_pitch_shift_f32: null handle / workspace");

  const hipStream_t s = (hipStream_t)stream;
  const AugLayout L = ag_layout(B, T);
  unsigned char* ws = (unsigned char*)workspace_dev;
  float* peaks = (float*)(ws + L.peaks);
  float2* S = (float2*)(ws + L.S);
  float2* P = (float2*)(ws + L.P);
  float* W = (float*)(ws + L.W);
  const int F = 1 + T / AG_HOP;

  AugArgs args;
  memset(&args, 0, sizeof(args));
  args.T = T;
  args.F = F;
  for (int i = 0; i < AG_NSTEP; ++i) {
    const int step = i - M2M_AUGMENT_MAX_STEP;
    m2m_augment_plan_t p;
    ag_plan(T, step, &p);
    AugStep& st = args.st[i];
    st.rate = ag_rate(step);
    st.fs = p.stretched_frames;
    st.len = p.stretched_len;
    st.up = a->up[i];
    st.down = a->down[i];
    st.half = 10 * (st.up > st.down ? st.up : st.down);
    const int64_t full = ((int64_t)st.len * st.up + st.down - 1) / st.down;
    st.n_out = (int)(full < T ? full : T);
    st.filt = a->filt_off[i];
  }
  for (int b0 = 0; b0 < B; b0 += AG_CHUNK) {
    const int nb = B - b0 < AG_CHUNK ? B - b0 : AG_CHUNK;
    int fs_max = 0, len_max = 0;
    bool any_norm = false;
    for (int b = 0; b < nb; ++b) {
      const int step = steps_host[b0 + b], i = step + M2M_AUGMENT_MAX_STEP;
      const bool nz = normalize_host && normalize_host[b0 + b];
      args.code[b] = (unsigned char)(i | (nz ? 0x80 : 0));
      any_norm |= nz;
      if (step != 0) {
        fs_max = fs_max > args.st[i].fs ? fs_max : args.st[i].fs;
        len_max = len_max > args.st[i].len ? len_max : args.st[i].len;
      }
    }
    const float* wav = wav_dev + (int64_t)b0 * T;
    float* pk = peaks + b0;
    float2* Sc = S + (int64_t)b0 * F * AG_BINS;
    float2* Pc = P + (int64_t)b0 * 2 * F * AG_BINS;
    float* Wc = W + (int64_t)b0 * 2 * T;
    if (any_norm) hipLaunchKernelGGL(ag_peak_kernel, dim3((unsigned)nb), dim3(1024), 0, s, wav, args, pk);
    if (fs_max > 0) {
      hipLaunchKernelGGL(ag_stft_kernel, dim3((unsigned)F, (unsigned)nb), dim3(AG_THREADS), 0, s, wav, args, a->dev, pk, Sc);
      hipLaunchKernelGGL(ag_vocoder_kernel, dim3((unsigned)ceil_div(AG_BINS, 128), (unsigned)nb), dim3(128), 0, s, Sc, args, Pc);
      if (stages && stages->stft)
        M2M_CHECK_HIP(hipMemcpyAsync(stages->stft + (int64_t)b0 * F * AG_BINS * 2, Sc, (size_t)nb * F * AG_BINS * sizeof(float2),
                                     hipMemcpyDeviceToDevice, s));
      if (stages && stages->stretched_stft)
        M2M_CHECK_HIP(hipMemcpyAsync(stages->stretched_stft + (int64_t)b0 * 2 * F * AG_BINS * 2, Pc,
                                     (size_t)nb * 2 * F * AG_BINS * sizeof(float2), hipMemcpyDeviceToDevice, s));
      hipLaunchKernelGGL(ag_istft_kernel, dim3((unsigned)fs_max, (unsigned)nb), dim3(AG_THREADS), 0, s, Pc, args, a->dev);
      if (len_max > 0)
        hipLaunchKernelGGL(ag_ola_kernel, dim3((unsigned)ceil_div(len_max, AG_THREADS), (unsigned)nb), dim3(AG_THREADS), 0, s, Pc, args,
                           a->dev, Wc);
      if (stages && stages->stretched_wave)
        M2M_CHECK_HIP(hipMemcpyAsync(stages->stretched_wave + (int64_t)b0 * 2 * T, Wc, (size_t)nb * 2 * T * sizeof(float),
                                     hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(ag_resample_kernel, dim3((unsigned)ceil_div(T, AG_THREADS), (unsigned)nb), dim3(AG_THREADS), 0, s, wav, Wc, args,
                       a->dev, pk, out_dev + (int64_t)b0 * T);
    M2M_CHECK_HIP(hipGetLastError());
  }
  return M2M_OK;
}
