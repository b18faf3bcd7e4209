// cng_frame.h -- comfort noise as device-inline functions: one frame of ComfortNoiseGenerator's inverse STFT (cng_kernel,
// span_cng_kernel) and one sample of the cross-fade of the generative and the comfort-noise hop (lossy_mix_kernel, span_cng_kernel).
#pragma once
#include "kernels.h"

namespace lyra {

constexpr double CNG_PI = 3.14159265358979323846;

// One frame: log-mel -> mel -> estimated FFT magnitudes -> counter-based random phase -> inverse FFT-1024.  256 threads, all
// of which call it (barriers inside).  P: filterbank and twiddles; feat: the frame's 160 log-mel floats; sd: the stream's phase
// key; hop: the frame's hop counter; re / im [1024] and mel [160]: doubles in LDS, overwritten.  Ends behind a barrier with the
// frame in re[]; cng_windowed(re, n) is then sample n as the overlap-add takes it.
__device__ __forceinline__ void cng_frame(const MelP& P, int tid, const float* feat, unsigned long long sd, unsigned long long hop,
                                          double* re, double* im, double* mel) {
  if (tid < 160) mel[tid] = (double)(float)exp((double)(feat[tid] * 10.f));   // std::exp(float * kNorm), float
  for (int i = tid; i < 1024; i += 256) { re[i] = 0.0; im[i] = 0.0; }
  __syncthreads();
  const double gain = __builtin_sqrt(1024.0 * 320.0 / (384.0 * 240.0));
  for (int i = P.start + tid; i <= P.end; i += 256) {
    // band[v + 1] = first bin whose lower band is >= v: find this bin's lower band ch (-1 .. 159)
    int lo = 0, hi = 161;   // band index domain v + 1
    while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (P.band[mid] <= i) lo = mid; else hi = mid; }
    const int ch = lo - 1;
    const double w = P.w[i];
    double v = 0.0;
    if (ch >= 0 && P.wsum[ch] > 0.0) v += w * mel[ch] / P.wsum[ch];
    if (ch + 1 < 160 && P.wsum[ch + 1] > 0.0) v += (1.0 - w) * mel[ch + 1] / P.wsum[ch + 1];
    const unsigned long long r = splitmix64_dev(sd ^ splitmix64_dev(hop * 1024ull + (unsigned long long)i));
    const double ang = (double)(r >> 11) * (1.0 / 9007199254740992.0) * 2.0 * CNG_PI;
    const double a = v * gain;
    const double xr = a * cos(ang), xi = a * sin(ang);
    // inverse DFT through the forward butterflies: conj in, conj out; inputs go to bit-reversed positions
    const int r0 = __brev((unsigned)i) >> 22;
    re[r0] = xr; im[r0] = (i == 0 || i == 512) ? 0.0 : -xi;
    if (i > 0 && i < 512) { const int r1 = __brev((unsigned)(1024 - i)) >> 22; re[r1] = xr; im[r1] = xi; }
  }
  __syncthreads();
#pragma unroll 1
  for (int p = 1; p <= 10; ++p) {
    const int len = 1 << p, half = len >> 1;
    for (int bf = tid; bf < 512; bf += 256) {
      int grp = bf >> (p - 1), k = bf & (half - 1);
      int i0 = grp * len + k, i1 = i0 + half;
      double wr = P.tw_re[half - 1 + k], wi = P.tw_im[half - 1 + k];
      double ur = re[i0], ui = im[i0];
      double xr = re[i1], xi = im[i1];
      double vr = xr * wr - xi * wi;
      double vi = xr * wi + xi * wr;
      re[i0] = ur + vr; im[i0] = ui + vi;
      re[i1] = ur - vr; im[i1] = ui - vi;
    }
    __syncthreads();
  }
}

// sample n (0..1023) of the frame that cng_frame left in re[], scaled and under the synthesis window
__device__ __forceinline__ double cng_windowed(const double* re, int n) {
  const double x = re[n] / 1024.0;
  const double v = 0.5 - 0.5 * cos(2.0 * CNG_PI * n / 1024.0);
  return x * v;
}

// Sample i of the cross-fade of MaybeOverlapAndInsert (lyra_decoder.cc:342-373) where both hops run: g / c = the generative
// and the comfort-noise hop, fade_w = the host-built table, fade / dir = where the fade starts and its direction.  Float
// products and sum are separate roundings; the conversion truncates.
__device__ __forceinline__ int16_t lossy_fade_sample(const float* fade_w, int fade, int dir, int i, const int16_t* g,
                                                     const int16_t* c) {
  const float w = fade_w[fade + i * dir - TWIN_FADE_LO];
  const float x = (float)g[i] * w;
  const float y = (float)c[i] * (1.f - w);
  return (int16_t)(int)(x + y);
}

}  // namespace lyra
