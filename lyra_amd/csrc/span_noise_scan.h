// span_noise_scan.h -- NoiseEstimator::ReceiveSamples' decision + recurrence over a list of frames, one wavefront, state in
// registers: the body of span_noise_scan_kernel, span_noise_scan_rates_kernel and span_lossy_scan_kernel.  Same float operations
// in the same order as noise_update_wave (misc_kernels.hip), restated here because the state lives elsewhere.
#pragma once
#include "kernels.h"

namespace lyra {

// One wavefront of 64 lanes (a workgroup of its own: static LDS of 160 floats), lane l owns bins l, l + 64, l + 128 (< 160).
// P: the estimator's constants; base: the stream's estimator slot, read once on entry and written once on exit; m: the list's
// mel rows (SPAN_MEL_ROW floats each: 160 bins, then their Average()); n: frames of the list.  The frames are walked in order
// -- ComputeIsNoise, then DecayBounds or the update.  Mel rows do not depend on the state: the rows of the next four frames
// are requested while the current four are worked on.  Average(smoothed) does depend on it and stays a sequential 160-term
// chain: the 160 values go through LDS and lane 0 sums them.
// Hooks, a struct passed by reference, says what the caller does with the decisions:
//   typename Hooks::Extra                    what on_frame needs of a list entry beside its mel row
//   load_extra(j, in)                        that of entry j (in == false: past the list, any value), requested with the row
//   on_entry(est, last_is_noise)             the slot's estimate and is_noise() before the first frame
//   on_frame(j, is_noise, active, est, x)    frame j applied: active = non-noise frames in front of it, est = the estimate after it
//   on_exit(active)                          the slot is written
template <typename Hooks>
__device__ __forceinline__ void span_noise_scan(const NoiseP& P, int lane, uint8_t* base, const float* m, long long n, Hooks& hooks) {
  typedef typename Hooks::Extra Extra;
  typedef float f32x4_t __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) float sh[160];
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
  hooks.on_entry(est, last_is_noise);
  long long active = 0;
  constexpr int PF = 4;
  float nb[PF][3], na[PF];
  Extra nx[PF];
  auto request = [&](long long fb) {   // the rows of frames fb .. fb + PF - 1 (past the list: zeros, unused)
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const bool in = fb + k < n;
      const float* r = m + (size_t)(in ? fb + k : 0) * SPAN_MEL_ROW;
#pragma unroll
      for (int i = 0; i < 3; ++i) nb[k][i] = in && lane + 64 * i < 160 ? r[lane + 64 * i] : 0.f;
      na[k] = in ? r[160] : 0.f;
      nx[k] = hooks.load_extra(in ? fb + k : 0, in);
    }
  };
  request(0);
  for (long long fb = 0; fb < n; fb += PF) {
    float cb[PF][3], ca[PF];
    Extra cx[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      ca[k] = na[k];
      cx[k] = nx[k];
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
      hooks.on_frame(fb + k, is_noise, active, est, cx[k]);
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
  }
  hooks.on_exit(active);
}

// The hooks of a DTX scan over the span `row`: flag_out[frame] = v_noise / v_active, map[region + c] = buffer frame of the
// span's c-th non-noise frame (map optional), *count = the span's non-noise frames.
struct SpanDtxScanHooks {
  struct Extra {};
  int lane;
  const SpanDtxRow& row;
  int32_t* flag_out;
  int v_noise, v_active;
  long long* map;
  int32_t* count;
  __device__ __forceinline__ Extra load_extra(long long, bool) const { return Extra(); }
  __device__ __forceinline__ void on_entry(const float (&)[3], int) const {}
  __device__ __forceinline__ void on_frame(long long j, bool is_noise, long long active, const float (&)[3], Extra) const {
    if (lane == 0) {
      const long long frame = row.frame0 + j;
      flag_out[frame] = is_noise ? v_noise : v_active;
      if (map && !is_noise) map[row.region + active] = frame;
    }
  }
  __device__ __forceinline__ void on_exit(long long active) const {
    if (lane == 0) *count = (int32_t)active;
  }
};

// the DTX scan of the wavefront's span rows[blockIdx.x] (blockIdx.x < the number of rows) with the constants P
__device__ __forceinline__ void span_dtx_scan(const NoiseP& P, const SpanDtxRow* rows, uint8_t* state, const float* mel,
                                              int32_t* flag_out, int v_noise, int v_active, long long* map, int32_t* counts) {
  const int lane = threadIdx.x;
  const SpanDtxRow row = rows[blockIdx.x];
  SpanDtxScanHooks hooks{lane, row, flag_out, v_noise, v_active, map, counts + blockIdx.x};
  span_noise_scan(P, lane, state + (size_t)row.id * st::NOISE_BYTES, mel + (size_t)row.region * SPAN_MEL_ROW, row.n_frames, hooks);
}

}  // namespace lyra
