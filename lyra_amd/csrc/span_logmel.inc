// span_logmel.inc -- text of span_logmel_kernel (spans_dtx_kernels.hip) and span_logmel_map_kernel (spans_lossy_kernels.hip): the
// estimator's log-mel of two consecutive frames of a span's list in one FFT-1024 (logmel_window.inc, logmel_fft.inc and
// logmel_band.inc: the arithmetic of logmel_body).
// In scope: Pp (MelP), two (the workgroup has a second frame), cur0 / cur1 and prev0 / prev1 (the frames and the hop in front of
// each), first (the workgroup holds the list's first frame: prev0 is slot_prev, and it alone writes the slot), slot_prev (the
// stream's N_PREV), last (the list's last frame, which becomes N_PREV), out (the first frame's mel row).
// Output per frame: the 160 log-mel bins and, beside them, Average() of the bins as noise_update_wave forms it (sequential
// float sum from 0.f, then / 160.f): it does not depend on the estimator's state, so it is taken off the serial scan.
  typedef double f64x2 __attribute__((ext_vector_type(2)));
  constexpr bool kRates = false;   // one filterbank per call (logmel_*.inc)
  const MelP& P = Pp[0];
  const MelP& PA = P;
  const MelP& PB = P;
  extern __shared__ __attribute__((aligned(16))) double dsm[];
  f64x2* z = reinterpret_cast<f64x2*>(dsm);
  double* wl = dsm + 1026;                                   // LDS reuse as in logmel_body
  float* mel_lds = reinterpret_cast<float*>(dsm + 1540);     // [2][160]
  const int tid = threadIdx.x;
#include "logmel_window.inc"
  (void)ce0; (void)ce1; (void)ce2;   // (per-frame band edges: logmel_rates_kernel only)
  __syncthreads();
  // every read of the old history is done: the list's last frame becomes the history (rows of 640 bytes, 16-byte aligned)
  if (first && tid < 40) st16(slot_prev + tid * 8, ld16(last + tid * 8));
#include "logmel_fft.inc"
  int e0 = be0, e1 = be1, e2 = be2;
  const double* wt = wl;
  auto band_item = [&](int f, int band) {
#include "logmel_band.inc"
    mel_lds[f * 160 + band] = lm;
  };
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
