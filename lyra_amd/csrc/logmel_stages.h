// logmel_stages.h -- the log-mel front end of two frames in one FFT-1024, as device-inline functions: logmel_window, logmel_fft
// and logmel_band, the stages that logmel_body (misc_kernels.hip) and span_logmel share, and span_logmel / span_logmel_row, the
// estimator's log-mel of a span's frames.  256 threads; dsm = the workgroup's dynamic LDS, at least logmel_lds_bytes().
#pragma once
#include "kernels.h"

namespace lyra {

typedef double f64x2 __attribute__((ext_vector_type(2)));

// dsm: Z[1024] as f64x2, (re, im) = (frame 0, frame 1) interleaved; later (|X_0[k]|, |X_1[k]|).  Once the two spectra are
// separated, z[k], k > 512, is dead and holds the mel weights of bins 0..512 and the hop's mel vectors [2][160] floats.
constexpr int LOGMEL_WL = 1026;     // doubles: the mel weights of frame 0 (of both frames unless kRates)
constexpr int LOGMEL_WL1 = 2048;    // doubles, kRates only: frame 1's weights, behind the FFT buffer (logmel_rates_lds_bytes())
constexpr int LOGMEL_MEL = 1540;    // doubles: float [2][160], the two mel vectors
template <bool kRates>
__device__ __forceinline__ double* logmel_wl(double* dsm, int f) { return dsm + (kRates && f ? LOGMEL_WL1 : LOGMEL_WL); }

// the row of the four rates' MelP / NoiseP (8 / 16 / 32 / 48 kHz)
__device__ __forceinline__ int mel_rate_index(int rate) { return rate == 8000 ? 0 : rate == 32000 ? 2 : rate == 48000 ? 3 : 1; }

struct LogmelWin {   // what thread tid keeps of the window stage
  int16_t b0s, b1s, c0s, c1s;   // this hop's samples, frame 0 / 1: tid >= 64 holds tid - 64 (b), tid < 128 holds tid + 192 (c)
  int be0, be1, be2;            // edges of the thread's band item (frame 0, band tid) or (frame 1, band tid - 96)
  int ce0, ce1, ce2;            // edges of the second item (frame 1, band tid) of threads < 64
  double wsel0, wsel1, wsel2;   // frame 0's mel weights of bins tid, tid + 256 and (tid == 0) 512, on their way to LDS
  double vsel0, vsel1, vsel2;   // frame 1's (kRates)
  double w1r, w1i, w2r, w2i, w3r, w3i;   // the thread's twiddles of the second radix-4 pass
};

// window = [previous hop | this hop] x periodic Hann, zero-padded to 1024, of frame 0 (prev0, cur0) and, where `two`, frame 1
// into z as re / im.  The first radix-4 pass of a decimation-in-time transform combines x[n], x[n+256], x[n+512], x[n+768]:
// thread n reads its own three window samples of both frames (x[n+768] = 0; x[n+512] = 0 for n >= 128) straight from memory,
// does that butterfly in registers and writes the four results where the second pass expects them (4 * digit-reverse(n) + q) --
// no staging pass, no scatter of single samples.  P: window and twiddles; PA / PB: frame 0's / frame 1's filterbank (kRates:
// they may differ).  No barrier inside: the caller places one before it replaces the history or calls logmel_fft.
template <bool kRates>
__device__ __forceinline__ LogmelWin logmel_window(const MelP& P, const MelP& PA, const MelP& PB, bool two,
                                                   const int16_t* prev0, const int16_t* prev1, const int16_t* cur0,
                                                   const int16_t* cur1, f64x2* z, int tid) {
  LogmelWin r;
  const int n = tid;
  const bool has1 = n >= 64, has2 = n < 128;
  const int16_t a0 = prev0[n], a1 = prev1[n];
  r.b0s = has1 ? cur0[n - 64] : prev0[n + 256]; r.b1s = has1 ? cur1[n - 64] : prev1[n + 256];
  r.c0s = has2 ? cur0[n + 192] : (int16_t)0; r.c1s = has2 ? cur1[n + 192] : (int16_t)0;
  const double h0 = P.hann[n], h1 = P.hann[n + 256], h2 = has2 ? P.hann[n + 512] : 0.0;
  // twiddles of the second pass (L = 4), requested before the first butterfly; mel weights and band edges for the epilogue
  {
    const int t1 = (tid & 3) * 64;
    r.w1r = P.tw4_re[t1]; r.w1i = P.tw4_im[t1]; r.w2r = P.tw4_re[2 * t1]; r.w2i = P.tw4_im[2 * t1];
    r.w3r = P.tw4_re[3 * t1]; r.w3i = P.tw4_im[3 * t1];
  }
  r.wsel0 = PA.w[tid]; r.wsel1 = PA.w[tid + 256]; r.wsel2 = tid == 0 ? PA.w[512] : 0.0;
  r.vsel0 = 0.0; r.vsel1 = 0.0; r.vsel2 = 0.0;
  if constexpr (kRates) { r.vsel0 = PB.w[tid]; r.vsel1 = PB.w[tid + 256]; r.vsel2 = tid == 0 ? PB.w[512] : 0.0; }
  // band sums: 320 (frame, band) items on 256 threads -- thread t < 160 takes (frame 0, band t), thread t >= 160 (frame 1, band
  // t - 96), the 96 widest bands, and threads t < 64 then also (frame 1, band t), the narrow ones: the longest chain is ONE wide band
  const int my_band = tid < 160 ? tid : tid - 96;
  const int* bandp = (kRates && tid >= 160) ? PB.band : PA.band;
  r.be0 = bandp[my_band]; r.be1 = bandp[my_band + 1]; r.be2 = bandp[my_band + 2];
  r.ce0 = r.be0; r.ce1 = r.be1; r.ce2 = r.be2;
  if constexpr (kRates) { if (tid < 64) { r.ce0 = PB.band[tid]; r.ce1 = PB.band[tid + 1]; r.ce2 = PB.band[tid + 2]; } }
  {
    const double ar = (double)a0 * h0, ai = two ? (double)a1 * h0 : 0.0;
    const double br = (double)r.b0s * h1, bi = two ? (double)r.b1s * h1 : 0.0;
    const double cr = (double)r.c0s * h2, ci = two ? (double)r.c1s * h2 : 0.0;
    const double s0r = ar + cr, s0i = ai + ci, s1r = ar - cr, s1i = ai - ci;   // d = 0: b + d = b - d = b
    unsigned rv = __brev((unsigned)n) >> 24;                                    // reverse the four base-4 digits of n
    rv = ((rv & 0xAAu) >> 1) | ((rv & 0x55u) << 1);
    f64x2* o = z + 4 * rv;
    o[0] = (f64x2){s0r + br, s0i + bi};
    o[1] = (f64x2){s1r + bi, s1i - br};     // (a - c) - i b
    o[2] = (f64x2){s0r - br, s0i - bi};
    o[3] = (f64x2){s1r - bi, s1i + br};     // (a - c) + i b
  }
  return r;
}

// Behind logmel_window and a barrier: radix-4 passes 2..5 on z = dsm, the two magnitude spectra in place (|X_f[k]| =
// dsm[2 * k + f], k <= 512), then the mel weights that win carries into logmel_wl<kRates>(dsm, 0 / 1).  Ends behind a barrier.
template <bool kRates>
__device__ __forceinline__ void logmel_fft(const MelP& P, const LogmelWin& win, double* dsm, int tid) {
  f64x2* z = reinterpret_cast<f64x2*>(dsm);
  double w1r = win.w1r, w1i = win.w1i, w2r = win.w2r, w2i = win.w2i, w3r = win.w3r, w3i = win.w3i;
  // four more radix-4 passes; pass s combines four L-point transforms (L = 4^s) into one 4L-point one:
  //   y_q = sum_r (-i)^(r q) W_4L^(r k) F_r[k].  The twiddles of pass s+1 (L2-resident table) are requested before
  // the butterflies of pass s, so their latency hides behind the LDS round trip and the barrier.
#pragma unroll
  for (int s = 1; s < 5; ++s) {
    const int L = 1 << (2 * s);
    const int k = tid & (L - 1), g = tid >> (2 * s);
    f64x2* p = z + g * 4 * L + k;
    double n1r = 1.0, n1i = 0.0, n2r = 1.0, n2i = 0.0, n3r = 1.0, n3i = 0.0;
    if (s < 4) {
      const int Ln = 4 * L, kn = tid & (Ln - 1);
      const int t1 = kn * (256 >> (2 * (s + 1)));     // W_4L^k = W_1024^(k * 1024 / 4L)
      n1r = P.tw4_re[t1]; n1i = P.tw4_im[t1]; n2r = P.tw4_re[2 * t1]; n2i = P.tw4_im[2 * t1];
      n3r = P.tw4_re[3 * t1]; n3i = P.tw4_im[3 * t1];
    }
    const f64x2 xa = p[0], x1 = p[L], x2 = p[2 * L], x3 = p[3 * L];
    const double br = __builtin_fma(x1.x, w1r, -(x1.y * w1i)), bi = __builtin_fma(x1.x, w1i, x1.y * w1r);
    const double cr = __builtin_fma(x2.x, w2r, -(x2.y * w2i)), ci = __builtin_fma(x2.x, w2i, x2.y * w2r);
    const double dr = __builtin_fma(x3.x, w3r, -(x3.y * w3i)), di = __builtin_fma(x3.x, w3i, x3.y * w3r);
    const double s0r = xa.x + cr, s0i = xa.y + ci, s1r = xa.x - cr, s1i = xa.y - ci;
    const double s2r = br + dr, s2i = bi + di, s3r = br - dr, s3i = bi - di;
    p[0] = (f64x2){s0r + s2r, s0i + s2i};
    p[L] = (f64x2){s1r + s3i, s1i - s3r};         // (a - c) - i (b - d)
    p[2 * L] = (f64x2){s0r - s2r, s0i - s2i};
    p[3 * L] = (f64x2){s1r - s3i, s1i + s3r};     // (a - c) + i (b - d)
    w1r = n1r; w1i = n1i; w2r = n2r; w2i = n2i; w3r = n3r; w3i = n3i;
    __syncthreads();
  }
  LYRA_TSTAMP(112);
  // Z = FFT(a + i b):  A[k] = (Z[k] + conj(Z[N-k])) / 2,  B[k] = (Z[k] - conj(Z[N-k])) / (2 i).  In place: the item
  // for bin k <= 512 reads Z[k] and Z[N - k] and writes index k only; index k < 512 is read by no other item and
  // indices > 512 are never written, so no staging buffer (and no barrier before the writes) is needed.
  for (int k = tid; k <= 512; k += 256) {
    const int nk = (1024 - k) & 1023;
    const f64x2 zz = z[k], yy = z[nk];
    const double Ar = 0.5 * (zz.x + yy.x), Ai = 0.5 * (zz.y - yy.y);
    const double Br = 0.5 * (zz.y + yy.y), Bi = 0.5 * (yy.x - zz.x);
    z[k] = (f64x2){__builtin_sqrt(Ar * Ar + Ai * Ai), __builtin_sqrt(Br * Br + Bi * Bi)};
  }
  __syncthreads();
  LYRA_TSTAMP(113);
  // the mel weights go to the now dead upper half of the buffer: the band loops would otherwise wait for one L2 round trip
  // per bin
  double* wl = logmel_wl<kRates>(dsm, 0);
  wl[tid] = win.wsel0;
  wl[tid + 256] = win.wsel1;
  if (tid == 0) wl[512] = win.wsel2;
  if constexpr (kRates) {
    double* wl1 = logmel_wl<kRates>(dsm, 1);
    wl1[tid] = win.vsel0;
    wl1[tid + 256] = win.vsel1;
    if (tid == 0) wl1[512] = win.vsel2;
  }
  __syncthreads();
}

// One (frame f, band) item behind logmel_fft: the band's log-mel value.  e0 / e1 / e2 = the band's edges (bins whose lower band
// is b - 1 contribute v - v * w to band b, bins whose lower band is b contribute v * w; ascending bin order == the reference's
// scatter loop order per band; the next bin's operands are read one trip ahead), wt = the frame's weights in LDS.
__device__ __forceinline__ float logmel_band(const double* dsm, int f, int e0, int e1, int e2, const double* wt) {
  const double* mag = dsm + f;          // |X_f[i]| = mag[2 * i]
  double acc = 0.0;
  double v = mag[2 * e0], wv = wt[e0];
  for (int i = e0; i < e2; ++i) {
    const double vn = mag[2 * i + 2], wn = wt[i + 1];
    const double w = v * wv;
    acc += i < e1 ? v - w : w;
    v = vn; wv = wn;
  }
  float x = (float)acc;
  x = x > 500.f ? x : 500.f;
  // log evaluated in double and rounded once: identical on host and device (oracle/lyra_oracle.c log_f)
  return (float)log((double)x) / 10.f;
}

// The estimator's log-mel of one or two (`two`) consecutive frames of a span's list: the arithmetic of logmel_body with one
// filterbank P.  cur0 / cur1 = the frames, prev0 / prev1 = the hop in front of each (without a second frame: cur1 = cur0,
// prev1 = prev0).  first: the workgroup holds the list's first frame -- prev0 is slot_prev, the stream's N_PREV, and this
// workgroup alone writes it: `last`, the list's last frame, becomes N_PREV.  Read and write are a barrier apart.
// Output per frame, at out + frame * SPAN_MEL_ROW: the 160 log-mel bins and, beside them, Average() of the bins as
// noise_update_wave forms it (sequential float sum from 0.f, then / 160.f): it does not depend on the estimator's state, so
// it is taken off the serial scan.
__device__ __forceinline__ void span_logmel(const MelP& P, bool two, bool first, const int16_t* cur0, const int16_t* cur1,
                                            const int16_t* prev0, const int16_t* prev1, int16_t* slot_prev,
                                            const int16_t* last, float* out) {
  extern __shared__ __attribute__((aligned(16))) double dsm[];
  float* mel_lds = reinterpret_cast<float*>(dsm + LOGMEL_MEL);     // [2][160]
  const int tid = threadIdx.x;
  const LogmelWin win = logmel_window<false>(P, P, P, two, prev0, prev1, cur0, cur1, reinterpret_cast<f64x2*>(dsm), tid);
  __syncthreads();
  // every read of the old history is done: the list's last frame becomes the history (rows of 640 bytes, 16-byte aligned)
  if (first && tid < 40) *reinterpret_cast<i32x4*>(slot_prev + tid * 8) = *reinterpret_cast<const i32x4*>(last + tid * 8);
  logmel_fft<false>(P, win, dsm, tid);
  const double* wt = logmel_wl<false>(dsm, 0);
  auto band_item = [&](int f, int band) { mel_lds[f * 160 + band] = logmel_band(dsm, f, win.be0, win.be1, win.be2, wt); };
  if (tid < 160) band_item(0, tid);
  else if (two) band_item(1, tid - 96);
  if (tid < 64 && two) band_item(1, tid);
  __syncthreads();
  for (int i = tid; i < (two ? 320 : 160); i += 256) {
    const int f = i >= 160;
    out[f * SPAN_MEL_ROW + (i - f * 160)] = mel_lds[i];
  }
  if (tid == 0 || (tid == 64 && two)) {   // Average(cur): one lane per frame
    const int f = tid >> 6;
    float a = 0.f;
    for (int i = 0; i < 160; ++i) a = a + mel_lds[f * 160 + i];
    out[f * SPAN_MEL_ROW + 160] = a / 160.f;
  }
}

// span_logmel for workgroup wg of the span `row`, whose frames lie in pcm: the workgroup's pair of frames (f0, f0 + 1) -- an odd
// span ends in a workgroup of one -- and their neighbours.  Frame 0's previous hop is the span stream's N_PREV in `state`, never
// the buffer (the row in front may be another span's); a later frame's is the row in front.  mel rows: mel[row.region + f].
__device__ __forceinline__ void span_logmel_row(const MelP& P, const SpanDtxRow& row, int wg, uint8_t* state, const int16_t* pcm,
                                                float* mel) {
  const long long f0 = ((long long)wg - row.wg0) * 2;
  if (f0 >= row.n_frames) return;   // (workgroup-uniform, before any barrier)
  const bool two = f0 + 1 < row.n_frames, first = f0 == 0;
  int16_t* slot_prev = reinterpret_cast<int16_t*>(state + (size_t)row.id * st::NOISE_BYTES + st::N_PREV);
  const int16_t* cur0 = pcm + (size_t)(row.frame0 + f0) * 320;
  const int16_t* cur1 = two ? cur0 + 320 : cur0;
  const int16_t* prev0 = first ? slot_prev : cur0 - 320;
  const int16_t* prev1 = two ? cur0 : prev0;
  const int16_t* last = pcm + (size_t)(row.frame0 + row.n_frames - 1) * 320;
  span_logmel(P, two, first, cur0, cur1, prev0, prev1, slot_prev, last, mel + (size_t)(row.region + f0) * SPAN_MEL_ROW);
}
static_assert(st::N_PREV % 16 == 0 && st::NOISE_BYTES % 16 == 0 && SPAN_MEL_ROW % 4 == 0, "16-byte moves");

}  // namespace lyra
