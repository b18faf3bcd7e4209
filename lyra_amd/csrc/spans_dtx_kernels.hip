// spans_dtx_kernels.hip -- lyra_hip_encode_spans_dtx_dev / lyra_hip_noise_spans_dev (api.hip, spans_api.inc): the NoiseEstimator
// of a DTX encoder over whole spans, in front of the chunked steps.  LyraEncoder::Encode (lyra_encoder.cc:113-156) hands the
// estimator the 16 kHz input audio and nothing else -- no encoder state, no features -- so the decisions of a whole recording
// can be computed before any encoder stage runs.  Two kernels:
//   span_logmel_kernel      the estimator's log-mel front end.  Its state is one hop of history (N_PREV), and inside a span that
//                           hop is the row in front of the frame: every frame of every span in ONE launch (the argument of
//                           span_resample_kernel).  The arithmetic is logmel_body's -- logmel_window.inc, logmel_fft.inc and
//                           logmel_band.inc are the text of both.
//   span_noise_scan_kernel  the recurrence.  It is serial in time but small (160 bins, five floats per bin, two integers): one
//                           wavefront per span walks its frames with the state in registers.  Same float operations in the same
//                           order as noise_update_wave (misc_kernels.hip), restated here because the state lives elsewhere.
#include "kernels.h"

namespace lyra {

namespace {
__device__ __forceinline__ i32x4 ld16(const void* p) { return *reinterpret_cast<const i32x4*>(p); }
__device__ __forceinline__ void st16(void* p, i32x4 v) { *reinterpret_cast<i32x4*>(p) = v; }
}  // namespace

// One workgroup per pair of consecutive frames (f0, f0 + 1) of ONE span (rows[] names the first workgroup of each span with
// frames; the lookup is on blockIdx alone); a span of an odd number of frames ends in a workgroup of one frame.
//   frame 0 of a span: previous hop from the span stream's N_PREV -- never from the buffer, the row in front may be another
//                      span's -- and the only workgroup that writes the slot: N_PREV = the span's last frame, what n_frames
//                      calls of logmel_kernel leave.  Read and write are one workgroup's, a barrier apart.
//   later frames:      previous hop = the row in front of the frame.
// Output per frame: the 160 log-mel bins and, beside them, Average() of the bins as noise_update_wave forms it (sequential
// float sum from 0.f, then / 160.f): it does not depend on the estimator's state, so it is taken off the serial scan.
__global__ __launch_bounds__(256) void span_logmel_kernel(const MelP* __restrict__ Pp, const SpanDtxRow* __restrict__ rows,
                                                           int n_rows, uint8_t* __restrict__ state,
                                                           const int16_t* __restrict__ pcm, float* __restrict__ mel) {
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
  int lo = 0, hi = n_rows - 1;   // the last row whose first workgroup is not behind this one
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[mid].wg0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const SpanDtxRow row = rows[lo];
  const long long f0 = ((long long)blockIdx.x - row.wg0) * 2;
  if (f0 >= row.n_frames) return;   // (workgroup-uniform, before any barrier)
  const bool two = f0 + 1 < row.n_frames;
  int16_t* slot_prev = reinterpret_cast<int16_t*>(state + (size_t)row.id * st::NOISE_BYTES + st::N_PREV);
  const int16_t* cur0 = pcm + (size_t)(row.frame0 + f0) * 320;
  const int16_t* cur1 = two ? cur0 + 320 : cur0;
  const int16_t* prev0 = f0 == 0 ? slot_prev : cur0 - 320;
  const int16_t* prev1 = two ? cur0 : prev0;
#include "logmel_window.inc"
  (void)ce0; (void)ce1; (void)ce2;   // (per-frame band edges: logmel_rates_kernel only)
  __syncthreads();
  // every read of the old history is done: the span's last frame becomes the history (rows of 640 bytes, 16-byte aligned)
  if (f0 == 0 && tid < 40) st16(slot_prev + tid * 8, ld16(pcm + (size_t)(row.frame0 + row.n_frames - 1) * 320 + tid * 8));
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
  float* out = mel + (size_t)(row.region + f0) * SPAN_MEL_ROW;
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
static_assert(st::N_PREV % 16 == 0 && st::NOISE_BYTES % 16 == 0 && SPAN_MEL_ROW % 4 == 0, "16-byte moves");

// One wavefront per span, lane l owns bins l, l + 64, l + 128 (< 160) as in noise_update_wave.  The slot is read once, the frames
// are walked in order -- ComputeIsNoise, then DecayBounds or the update -- and the slot is written once.  Mel rows do not depend
// on the state: the rows of the next four frames are requested while the current four are worked on.  Average(smoothed) does
// depend on it and stays a sequential 160-term chain: the 160 values go through LDS and lane 0 sums them.
__global__ __launch_bounds__(64) void span_noise_scan_kernel(NoiseP P, const SpanDtxRow* __restrict__ rows, int n_rows,
                                                              uint8_t* __restrict__ state, const float* __restrict__ mel,
                                                              int32_t* __restrict__ flag_out, int v_noise, int v_active,
                                                              long long* __restrict__ map, int32_t* __restrict__ counts) {
  typedef float f32x4_t __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) float sh[160];
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= n_rows) return;
  const SpanDtxRow row = rows[blockIdx.x];
  uint8_t* base = state + (size_t)row.id * st::NOISE_BYTES;
  int* hdr = reinterpret_cast<int*>(base);
  float* f_smooth = reinterpret_cast<float*>(base + st::N_SMOOTH);
  float* f_sq = reinterpret_cast<float*>(base + st::N_SQ);
  float* f_tmp = reinterpret_cast<float*>(base + st::N_TMPMIN);
  float* f_est = reinterpret_cast<float*>(base + st::N_EST);
  float* f_bound = reinterpret_cast<float*>(base + st::N_BOUND);
  float est[3], bound[3], sm[3], sq[3], tm[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int bin = lane + 64 * i;
    const bool ld = bin < 160;
    est[i] = ld ? f_est[bin] : 0.f;
    bound[i] = ld ? f_bound[bin] : 0.f;
    sm[i] = ld ? f_smooth[bin] : 0.f;
    sq[i] = ld ? f_sq[bin] : 0.f;
    tm[i] = ld ? f_tmp[bin] : 0.f;
  }
  int initialised = hdr[st::N_INIT / 4];
  int hops = hdr[st::N_HOPS / 4];
  int last_is_noise = hdr[st::N_IS_NOISE / 4];
  const float* m = mel + (size_t)row.region * SPAN_MEL_ROW;
  const long long n = row.n_frames;
  long long active = 0;
  constexpr int PF = 4;
  float nb[PF][3], na[PF];
  auto request = [&](long long fb) {   // the rows of frames fb .. fb + PF - 1 (past the span: zeros, unused)
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const bool in = fb + k < n;
      const float* r = m + (size_t)(in ? fb + k : 0) * SPAN_MEL_ROW;
#pragma unroll
      for (int i = 0; i < 3; ++i) nb[k][i] = in && lane + 64 * i < 160 ? r[lane + 64 * i] : 0.f;
      na[k] = in ? r[160] : 0.f;
    }
  };
  request(0);
  for (long long fb = 0; fb < n; fb += PF) {
    float cb[PF][3], ca[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      ca[k] = na[k];
#pragma unroll
      for (int i = 0; i < 3; ++i) cb[k][i] = nb[k][i];
    }
    request(fb + PF);
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      if (fb + k >= n) break;   // (wave-uniform)
      const float* cur = cb[k];
      bool differs = false;
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (lane + 64 * i < 160) differs = differs || (__builtin_fabsf(cur[i] - est[i]) > bound[i]);
      const bool is_noise = __builtin_amdgcn_ballot_w64(differs) == 0ull;   // ComputeIsNoise (wave-uniform)
      if (is_noise) {
#pragma unroll
        for (int i = 0; i < 3; ++i) bound[i] = bound[i] * P.bound_decay;   // DecayBounds
      } else {
        if (!initialised) {   // first update (noise_estimator.cc:180-186)
#pragma unroll
          for (int i = 0; i < 3; ++i) { sm[i] = cur[i]; sq[i] = cur[i] * cur[i]; tm[i] = cur[i]; }
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
          if (lane + 64 * i < 160) sh[lane + 64 * i] = sm[i];
        // lane 0 reads what the other lanes of this wavefront have just written
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the per-bin factor of SmoothingFactor() does not need the average: beside the summing lane
        float ebin[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float de = (sm[i] - est[i]) / 0.3f;
          ebin[i] = expf_via_double(-(de * de));
        }
        float a = 0.f;
        if (lane == 0) {   // Average(smoothed): sequential float sum from 0.f
          const f32x4_t* s4 = reinterpret_cast<const f32x4_t*>(sh);
#pragma unroll 4
          for (int i = 0; i < 40; ++i) {
            const f32x4_t v = s4[i];
            a = a + v.x; a = a + v.y; a = a + v.z; a = a + v.w;
          }
          a = a / 160.f;
        }
        const float avg_sm = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, a)));
        // (the next frame's writes to sh follow lane 0's reads: its sum is an operand of everything below)
        __builtin_amdgcn_wave_barrier();
        const float kPowDiff = 0.3f;
        const float dd = (avg_sm - ca[k]) / kPowDiff;
        const float correction = expf_via_double(-(dd * dd));
        const double logn = 5.075173815233827;   // std::log(160) in double (noise_bound_.size())
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const float sf = P.max_smoothing * correction * ebin[i];
          const float c2 = cur[i] * cur[i];
          const float nsm = sf * sm[i] + (1.f - sf) * cur[i];   // (-ffp-contract=off: every product rounded)
          const float nsq = sf * sq[i] + (1.f - sf) * c2;
          float nest, ntm;
          if (hops == 0) { nest = __builtin_fminf(tm[i], nsm); ntm = nsm; }                      // UpdateMinAndTemp
          else { nest = __builtin_fminf(est[i], nsm); ntm = __builtin_fminf(tm[i], nsm); }
          float var = nsq - nsm * nsm;
          var = var > 0.f ? var : 0.f;
          sm[i] = nsm; sq[i] = nsq; tm[i] = ntm; est[i] = nest;
          bound[i] = (float)((double)0.9f * __builtin_sqrt((double)var * logn));               // ComputeBounds
        }
        initialised = 1;
        hops = (hops + 1) % P.hops_per_update;
      }
      last_is_noise = is_noise ? 1 : 0;
      if (lane == 0) {
        const long long frame = row.frame0 + fb + k;
        flag_out[frame] = is_noise ? v_noise : v_active;
        if (map && !is_noise) map[row.region + active] = frame;
      }
      active += is_noise ? 0 : 1;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int bin = lane + 64 * i;
    if (bin < 160) { f_smooth[bin] = sm[i]; f_sq[bin] = sq[i]; f_tmp[bin] = tm[i]; f_est[bin] = est[i]; f_bound[bin] = bound[i]; }
  }
  if (lane == 0) {
    hdr[st::N_INIT / 4] = initialised;
    hdr[st::N_HOPS / 4] = hops;
    hdr[st::N_IS_NOISE / 4] = last_is_noise;
    counts[blockIdx.x] = (int32_t)active;
  }
}

}  // namespace lyra
