// resample_pass.h -- the resampler's pass of one wavefront as device-inline functions: what the four resample kernels of
// misc_kernels.hip, ds_splice_row (decode_samples_rows.h) and the three span_resample kernels share.  A kernel keeps its head --
// which row, which design, where the samples lie -- and calls rs_stream_pass or rs_span_pass: one FIR, one clip, at every site.
#pragma once
#include "kernels.h"

namespace lyra {

constexpr int RS_H = st::RS_TAPS - 1;   // the FIR's history: the floats at the front of a wavefront's LDS row
// the row of tab [2][3] = [dir][8000, 32000, 48000] (rates_ensure); -1: 16 kHz (the pass is a copy) or no codec rate
__device__ __forceinline__ int rs_design_index(int rate) { return rate == 8000 ? 0 : rate == 32000 ? 1 : rate == 48000 ? 2 : -1; }

// A wavefront reads what its other lanes wrote to its own LDS row: no workgroup barrier is possible behind a wave-uniform early
// return and none is needed, but the order is pinned rather than assumed.
__device__ __forceinline__ void rs_wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// src[0 .. n_in) as floats to rsb[RS_H ..].  vec: 16-byte items (src 16-byte aligned and n_in a multiple of 8).
__device__ __forceinline__ void rs_load(float* rsb, const int16_t* src, int n_in, bool vec, int lane) {
  if (vec) {
    for (int c = lane; c * 8 < n_in; c += 64) {
      const i32x4 raw = *reinterpret_cast<const i32x4*>(src + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) rsb[RS_H + c * 8 + e] = (float)(int16_t)((raw[e >> 1] >> ((e & 1) * 16)) & 0xffff);
    }
  } else {
    for (int i = lane; i < n_in; i += 64) rsb[RS_H + i] = (float)src[i];
  }
}

// The polyphase FIR over the wavefront's row rsb = [RS_H history | n_in new samples]: n_in * up outputs (down == 1) or n_out
// outputs (down > 1; in_pos = the stream's input count in front of this pass, of which only in_pos % down matters).  Output i
// is `dst[i] = v`: Dst is int16_t* or a type with that operator (SpliceDst, decode_samples_rows.h).
template <typename Dst>
__device__ __forceinline__ void rs_fir(const ResampleP* P, const float* rsb, int n_in, int n_out, int in_pos, Dst dst, int lane) {
  auto clip = [](float acc) { return (int16_t)(acc < -32768.f ? -32768.f : (acc > 32767.f ? 32767.f : acc)); };   // ClipToInt16 (dsp_utils.h:56-72)
  if (P->down == 1) {
    // interpolation: output k * up + ph is phase ph of the window at input k -- a lane takes input positions
    // k = lane, lane + 64, ...: one window of 35 samples in registers feeds all `up` phases, coefficients are scalars
    for (int k = lane; k < n_in; k += 64) {
      float win[st::RS_TAPS];
#pragma unroll
      for (int j = 0; j < st::RS_TAPS; ++j) win[j] = rsb[k + j];
#pragma unroll
      for (int ph = 0; ph < 3; ++ph) {
        if (ph < P->up) {
          float acc = 0.f;
#pragma unroll
          for (int j = 0; j < st::RS_TAPS; ++j) acc = acc + P->coef[ph][j] * win[j];
          dst[k * P->up + ph] = clip(acc);
        }
      }
    }
  } else {
    // decimation: the first input index (0-based in this call) that yields an output follows from the carried phase
    const int first = (P->down - in_pos % P->down) % P->down;
    for (int o = lane; o < n_out; o += 64) {
      const int k = first + o * P->down;
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < st::RS_TAPS; ++j) acc = acc + P->coef[0][j] * rsb[k + j];
      dst[o] = clip(acc);
    }
  }
}

// The stream's slot after a pass over n_in samples: the row's last RS_H floats become the history, the phase moves on.
__device__ __forceinline__ void rs_slot_write(const float* rsb, int n_in, int in_pos, uint8_t* slot, int lane) {
  // (same wavefront wrote and read this row: no barrier needed before the history leaves it)
  if (lane < RS_H) reinterpret_cast<float*>(slot + st::RS_HIST)[lane] = rsb[n_in + lane];
  // only the decimation phase is ever used: kept modulo 6 = lcm of the `down` factors (1, 2, 3), so the counter never wraps
  // out of phase (the oracle keeps an unbounded counter)
  if (lane == 0) *reinterpret_cast<int*>(slot + st::RS_IN_POS) = (in_pos + n_in) % 6;
}

// One stream's call, one wavefront: n_in samples at src through the resampler of stream `id` (its slot in the resampler region
// `state`: history and phase read, then written back) to dst, in the wavefront's own LDS row rsb (RS_H + n_in floats).  The new
// samples are requested before the slot is addressed.  kBlockBarrier (resample_kernel): the row is handed over by a workgroup
// barrier that every wavefront reaches; one with on == false has loaded a valid row of another stream and leaves behind it.
template <bool kBlockBarrier = false, typename Dst>
__device__ __forceinline__ void rs_stream_pass(const ResampleP* P, float* rsb, int lane, uint8_t* state, int id, const int16_t* src,
                                               int n_in, bool vec, Dst dst, int n_out, bool on = true) {
  rs_load(rsb, src, n_in, vec, lane);
  uint8_t* slot = state + (size_t)id * st::RS_BYTES;
  const int in_pos = *reinterpret_cast<const int*>(slot + st::RS_IN_POS);
  if (lane < RS_H) rsb[lane] = reinterpret_cast<const float*>(slot + st::RS_HIST)[lane];
  if constexpr (kBlockBarrier) {
    __syncthreads();
    if (!on) return;
  } else {
    rs_wave_fence();
  }
  rs_fir<Dst>(P, rsb, n_in, n_out, in_pos, dst, lane);
  rs_slot_write(rsb, n_in, in_pos, slot, lane);
}

// Frame f of a span of n_frames frames, one wavefront: the frame's n_in samples at src (16-byte aligned, n_in a multiple of
// 8) to dst.
//   f == 0        history from the span stream's slot, and the only wavefront that writes it: RS_HIST = last[0 .. RS_H), the span's
//                 last input samples, RS_IN_POS advanced by n_frames * n_in mod 6 -- what n_frames calls of rs_stream_pass leave.
//   later frames  history = prev[0 .. RS_H), the samples in front of the frame.  Of the slot they read the phase word alone,
//                 which the frame-0 wavefront may be replacing meanwhile: old and new value differ by a multiple of n_in, n_in
//                 is a multiple of `down` and `down` divides 6, so rs_fir's `first` is the same from either.  A relaxed atomic
//                 load says that this is meant; an up-sampling pass has no phase and does not read it.  (last is not read.)
template <typename Dst>
__device__ __forceinline__ void rs_span_pass(const ResampleP* P, float* rsb, int lane, uint8_t* slot, long long f,
                                             long long n_frames, const int16_t* src, const int16_t* prev, const int16_t* last,
                                             int n_in, Dst dst, int n_out) {
  rs_load(rsb, src, n_in, true, lane);
  float* hist = reinterpret_cast<float*>(slot + st::RS_HIST);
  const int in_pos = f == 0 || P->down > 1
                         ? __hip_atomic_load(reinterpret_cast<const int*>(slot + st::RS_IN_POS), __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT)
                         : 0;
  if (lane < RS_H) rsb[lane] = f == 0 ? hist[lane] : (float)prev[lane];
  rs_wave_fence();
  rs_fir<Dst>(P, rsb, n_in, n_out, in_pos, dst, lane);
  if (f != 0) return;
  if (lane < RS_H) hist[lane] = (float)last[lane];
  if (lane == 0)
    __hip_atomic_store(reinterpret_cast<int*>(slot + st::RS_IN_POS), (in_pos + (int)(n_frames % 6) * (n_in % 6)) % 6,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
static_assert(RS_H < 160, "the history lies inside one frame at every rate");

}  // namespace lyra
