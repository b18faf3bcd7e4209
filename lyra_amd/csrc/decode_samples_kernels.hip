// decode_samples_kernels.hip -- the device-resident packet-loss state machine of lyra_hip_decode_samples_dev (api.hip,
// decode_samples_api.inc): LyraDecoder::SetEncodedPacket + DecodeSamples(n) for request sizes that are not tied to the hop
// (transition in decode_samples_plan.h).  One call = plan (decode stream) -> generative model on the rows that start a
// hop (decode stream) -> on the noise stream: comfort noise for the rows that start a comfort-noise hop in their first
// pass, the estimator's input gathered from whole received hops, the estimator, comfort noise for the rows that start
// their hop in the second pass (they read the UPDATED estimate), the slices, the output resampler.
#include "kernels.h"
#include "decode_samples_rows.h"

namespace lyra {

// One thread per row applies the transition and hands out the call's id lists and the four info words (ds_plan_row,
// decode_samples_rows.h); then 16 lanes per row move feature vectors through the stream's ring (ds_plan_move).  Counted in
// *err, one atomic per wavefront at most: sizes that are neither 0 nor a packet size of the codec, packets that found the
// ring full, rows whose plan left its proven bounds.
__global__ __launch_bounds__(256) void ds_plan_kernel(const int32_t* __restrict__ ids, int B,
                                                       const int32_t* __restrict__ pkt_bytes, int n_internal,
                                                       uint8_t* __restrict__ cng_state, int32_t* __restrict__ gen_ids,
                                                       int32_t* __restrict__ cng1_ids, int32_t* __restrict__ cng2_ids,
                                                       int32_t* __restrict__ est_ids, int32_t* __restrict__ info,
                                                       float* __restrict__ feats, float* __restrict__ ring,
                                                       unsigned* __restrict__ err) {
  __shared__ DsPlanLds sh;
  const int tid = threadIdx.x, b0 = blockIdx.x * 256, b = b0 + tid;
  int nerr = 0;
  ds_plan_lds_clear(sh, tid);
  if (b < B) {
    const int pb = pkt_bytes[b];
    const bool rx = mixed_received(pb);
    if (pb != 0 && !rx) nerr++;
    ds_plan_row(sh, tid, b, ids[b], rx, n_internal, true, nerr, cng_state, gen_ids, cng1_ids, cng2_ids, est_ids, info);
  }
  ds_wave_count(nerr, err, tid);
  ds_plan_move(sh, tid, b0, B, feats, ring);
}

// est_in[b][0..320) = the whole received hop that completes in this call: the hop the stream holds (the part an earlier
// call handed out included), or the call's new hop when it starts and ends here.  Rows without an estimator update leave.
__global__ __launch_bounds__(256) void ds_est_gather_kernel(const int32_t* __restrict__ ids, int B,
                                                             const int32_t* __restrict__ info,
                                                             const int16_t* __restrict__ gan_new, const int16_t* gan_held,
                                                             int16_t* __restrict__ est_in) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int f = info[(size_t)b * 4 + 1];
  if (!(f & DS_EST)) return;
  const uint2* src = reinterpret_cast<const uint2*>((f & DS_EST_NEW) ? gan_new + (size_t)b * 320 : gan_held + (size_t)ids[b] * 320);
  uint2* dst = reinterpret_cast<uint2*>(est_in + (size_t)b * 320);
  dst[lane] = src[lane];
  if (lane < 16) dst[64 + lane] = src[64 + lane];
}

// One wavefront per row: the row's one or two passes (RunModel slices + MaybeOverlapAndInsert, lyra_decoder.cc:342-373, the
// arithmetic of twin_assemble_kernel and lossy_mix_kernel with the same weight table), then the hops that started in this
// call become the stream's held hops.  Every branch on the info words is wave-uniform.  A slice starts at any sample of a
// hop, so the samples are read and written as single int16 (640 bytes per row at most).  Rows without an estimator update
// report the estimator's unchanged is_noise().
__global__ __launch_bounds__(256) void ds_slice_kernel(const int32_t* __restrict__ ids, int B, const int32_t* __restrict__ info,
                                                        const int16_t* __restrict__ gan_new, const int16_t* __restrict__ cng_new,
                                                        int16_t* gan_held, int16_t* cng_held,
                                                        const float* __restrict__ fade_w, int16_t* __restrict__ out,
                                                        int out_stride, const uint8_t* __restrict__ noise_state,
                                                        int32_t* __restrict__ is_noise, int32_t* __restrict__ is_cn) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool on = b < B;
  int4 w = make_int4(0, 0, 0, 0);
  int id = 0;
  if (on) {
    w = *reinterpret_cast<const int4*>(info + (size_t)b * 4);
    id = ids[b];
  }
  const int f = w.y;
  const int16_t* gn = gan_new + (size_t)b * 320;
  const int16_t* cn = cng_new + (size_t)b * 320;
  int16_t* gh = gan_held + (size_t)id * 320;
  int16_t* ch = cng_held + (size_t)id * 320;
  if (on) {
    int16_t* o = out + (size_t)b * out_stride;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int n = k ? (w.x >> 16) : (w.x & 0xffff);
      const bool gen = f & (k ? DS_S2_GEN : DS_S1_GEN), noise = f & (k ? DS_S2_CNG : DS_S1_CNG);
      const int dir = (f & (k ? DS_S2_TO_CNG : DS_S1_TO_CNG)) ? 1 : -1;
      const int fade = k ? (w.w >> 16) : (w.w & 0xffff);
      const int16_t* g = k || (f & DS_S1_GEN_NEW) ? gn : gh + (w.z & 0xffff);
      const int16_t* c = k || (f & DS_S1_CNG_NEW) ? cn : ch + (w.z >> 16);
      for (int i = lane; i < n; i += 64) {
        int16_t v;
        if (!noise) v = g[i];
        else if (!gen) v = c[i];
        else {
          const float wt = fade_w[fade + i * dir - TWIN_FADE_LO];
          const float x = (float)g[i] * wt;
          const float y = (float)c[i] * (1.f - wt);
          v = (int16_t)(int)(x + y);
        }
        o[i] = v;
      }
      o += n;
    }
    if (lane == 0) {
      if (is_cn) is_cn[b] = (f & DS_CN) ? 1 : 0;
      if (is_noise && !(f & DS_EST))
        is_noise[b] = *reinterpret_cast<const int*>(noise_state + (size_t)id * st::NOISE_BYTES + st::N_IS_NOISE);
    }
  }
  __syncthreads();   // pass 1 has read the held hops before the new ones replace them
  if (on) {
    if (f & DS_GEN_NEW)
      for (int i = lane; i < 80; i += 64) reinterpret_cast<uint2*>(gh)[i] = reinterpret_cast<const uint2*>(gn)[i];
    if (f & DS_CNG_NEW)
      for (int i = lane; i < 80; i += 64) reinterpret_cast<uint2*>(ch)[i] = reinterpret_cast<const uint2*>(cn)[i];
  }
}

}  // namespace lyra
