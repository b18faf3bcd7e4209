// lossy_kernels.hip -- the device-resident packet-loss state machine of lyra_hip_decode_lossy_dev (api.hip, lossy_api.inc):
// LyraDecoder::DecodeSamplesInternal for hop-synchronous receivers (lyra_decoder.cc:228-340; transition in lossy_plan.h).
// One tick = plan (decode stream) -> generative model on the masked id list (decode stream) -> comfort noise on its
// masked list, mix, NoiseEstimator on the received rows, output resampler (noise stream).
#include "kernels.h"
#include "lossy_plan.h"
#include "cng_frame.h"

namespace lyra {

// One thread per row: read the stream's control word, apply the tick, write it back, and hand out the tick's id lists
// (-1 = the row skips that leg) and mix info.  Then the rows that conceal get ZeroFeatureEstimator::Estimate's features
// (64 x 0.0f, zero_feature_estimator.h) in place of the RVQ decode of whatever their packet row holds.
// A packet_bytes value other than 0 and nbytes is "not received" and counted in *err.  MIXED: received iff packet_bytes
// is a size of the codec (mixed_received), counted iff neither that nor 0; bytes_from_bits as in rvq_decode_mixed_kernel.
__global__ __launch_bounds__(256) void lossy_plan_kernel(const int32_t* __restrict__ ids, int B,
                                                          const int32_t* __restrict__ pkt_bytes, int nbytes,
                                                          const uint8_t* __restrict__ rx_ring_row,
                                                          uint8_t* __restrict__ cng_state, int32_t* __restrict__ gen_ids,
                                                          int32_t* __restrict__ cng_ids, int32_t* __restrict__ est_ids,
                                                          int32_t* __restrict__ info, float* __restrict__ feats,
                                                          unsigned* __restrict__ err) {
  constexpr bool MIXED = false;
  constexpr int bytes_from_bits = 0;
#include "lossy_plan_tile.inc"
}

// lyra_hip_decode_lossy_mixed_dev: pkt_bytes is required (sizes, or with bytes_from_bits the schedule's bit counts)
__global__ __launch_bounds__(256) void lossy_plan_mixed_kernel(const int32_t* __restrict__ ids, int B,
                                                                const int32_t* __restrict__ pkt_bytes, int bytes_from_bits,
                                                                const uint8_t* __restrict__ rx_ring_row,
                                                                uint8_t* __restrict__ cng_state, int32_t* __restrict__ gen_ids,
                                                                int32_t* __restrict__ cng_ids, int32_t* __restrict__ est_ids,
                                                                int32_t* __restrict__ info, float* __restrict__ feats,
                                                                unsigned* __restrict__ err) {
  constexpr bool MIXED = true;
  constexpr int nbytes = 0;
#include "lossy_plan_tile.inc"
}

// One wavefront per row, lane l writes samples l + 64 j.  The arithmetic of twin_assemble_kernel (MaybeOverlapAndInsert,
// lyra_decoder.cc:342-373) with gen_n = cng_n = 320: where both hops run, sample i is (int16)(gan * w + cng * (1 - w)),
// w = fade_w[fade + i * dir] (the same host-built table).  Unreceived rows report the estimator's unchanged is_noise().
__global__ __launch_bounds__(256) void lossy_mix_kernel(const int32_t* __restrict__ ids, int B, const int32_t* __restrict__ info,
                                                         const int16_t* __restrict__ gan, const int16_t* __restrict__ cng,
                                                         const float* __restrict__ fade_w, int16_t* __restrict__ out,
                                                         const uint8_t* __restrict__ noise_state,
                                                         int32_t* __restrict__ is_noise, int32_t* __restrict__ is_cn) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  const int f = info[b];
  const int16_t* g = gan + (size_t)b * 320;
  const int16_t* c = cng + (size_t)b * 320;
  int16_t* o = out + (size_t)b * 320;
  const bool gen = f & LOSSY_GEN, noise = f & LOSSY_CNG;
  const int fade = (f >> 8) * 320, dir = (f & LOSSY_TO_CNG) ? 1 : -1;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const int i = lane + 64 * j;
    o[i] = !noise ? g[i] : !gen ? c[i] : lossy_fade_sample(fade_w, fade, dir, i, g, c);
  }
  if (lane == 0) {
    if (is_cn) is_cn[b] = (f & LOSSY_CN) ? 1 : 0;
    if (is_noise && !(f & LOSSY_RX))
      is_noise[b] = *reinterpret_cast<const int*>(noise_state + (size_t)ids[b] * st::NOISE_BYTES + st::N_IS_NOISE);
  }
}

}  // namespace lyra
