// lossy_plan.h -- one tick of LyraDecoder's packet-loss state machine for a hop-synchronous receiver.
//
// LyraDecoder::SetEncodedPacket + DecodeSamplesInternal (lyra_decoder.cc:172-209, :228-340) when every 20 ms tick either
// delivers one packet or none and then asks for exactly one hop (320 internal samples).  The reference's loop then runs
// exactly once per tick, both conditioned hops are always consumed whole, and its integers stay multiples of 320:
//   concealment_progress  cp    in {0, 320, ..., 1280}  (1280 = GetConcealmentDurationSamples, :41-51)
//   fade_progress         fade  in {0, 320, 640}        (640 = GetFadeDurationSamples, :53-62)
//   fade_direction        dir   kFadeToCNG (+1) / kFadeFromCNG (-1)
// The three are kept per stream in one 32-bit word whose zero value is the reference's initial state (0, 0, kFadeFromCNG):
// bits 0-7 cp / 320, bits 8-15 fade / 320, bit 16 dir == kFadeToCNG.  The word lives in bytes LOSSY_CTL.. of the stream's
// comfort-noise slot (state_layout.h R_CNG), so context creation and lyra_hip_reset_streams give the initial state.
// Host and device code (and a plain C++ compiler: tests/test_lossy_plan_cpu.py) share this function.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LYRA_LOSSY_HD __host__ __device__
#else
#define LYRA_LOSSY_HD
#endif

namespace lyra {

constexpr int LOSSY_CTL = 8;            // byte offset of the control word in a stream's R_CNG slot (C_HOP 0..7, C_OLA 64..)
constexpr int LOSSY_CONCEAL = 1280;     // GetConcealmentDurationSamples
constexpr int LOSSY_FADE = 640;         // GetFadeDurationSamples

struct LossyTick {
  uint32_t ctl;       // control word after the tick
  int cp, fade, dir;  // ... unpacked
  int run_gen;        // the generative model runs this tick (from the packet if received, else from zero features)
  int run_cng;        // the comfort-noise generator runs (on the decoder-side noise estimate before this tick's update)
  int feed_est;       // the decoder-side NoiseEstimator receives the generative hop (received ticks only)
  int mix_fade;       // fade_progress and direction the cross-fade starts from (when both hops run)
  int mix_dir;
  int comfort_noise;  // is_comfort_noise() after the tick (fade == 640)
};

LYRA_LOSSY_HD inline uint32_t lossy_pack(int cp, int fade, int dir) {
  return (uint32_t)(cp / 320) | ((uint32_t)(fade / 320) << 8) | ((dir > 0 ? 1u : 0u) << 16);
}

// received: SetEncodedPacket was called before this tick's DecodeSamples(hop).
LYRA_LOSSY_HD inline LossyTick lossy_tick(uint32_t ctl, bool received) {
  int cp = (int)(ctl & 255u) * 320, fade = (int)((ctl >> 8) & 255u) * 320, dir = (ctl >> 16) & 1u ? 1 : -1;
  // SetEncodedPacket (:172-209): both hop FIFOs are empty between ticks, so concealment_progress becomes -0
  if (received) cp = 0;
  // DecodeSamplesInternal, one pass (:240-262)
  if (received) dir = -1;                           // kFadeFromCNG
  else if (cp == LOSSY_CONCEAL) dir = 1;            // kFadeToCNG
  else cp += 320;
  int gen = 1, cng = 1, next = fade + dir * 320;
  if (dir == 1 && fade == LOSSY_FADE) { next = LOSSY_FADE; gen = 0; }
  else if (dir == -1 && fade == 0) { next = 0; cng = 0; }
  LossyTick t;
  t.ctl = lossy_pack(cp, next, dir);
  t.cp = cp; t.fade = next; t.dir = dir;
  t.run_gen = gen; t.run_cng = cng; t.feed_est = received ? 1 : 0;
  t.mix_fade = fade; t.mix_dir = dir;
  t.comfort_noise = next == LOSSY_FADE ? 1 : 0;
  return t;
}

// What the plan kernel hands the noise-stream leg per row (one int32).
constexpr int32_t LOSSY_GEN = 1, LOSSY_CNG = 2, LOSSY_RX = 4, LOSSY_CN = 8, LOSSY_TO_CNG = 16;
LYRA_LOSSY_HD inline int32_t lossy_info(const LossyTick& t) {
  return (t.run_gen ? LOSSY_GEN : 0) | (t.run_cng ? LOSSY_CNG : 0) | (t.feed_est ? LOSSY_RX : 0) |
         (t.comfort_noise ? LOSSY_CN : 0) | (t.mix_dir > 0 ? LOSSY_TO_CNG : 0) | ((t.mix_fade / 320) << 8);
}

// ---- mixed bitrates (lyra_hip_decode_lossy_mixed_dev, LYRA_HIP_STEP_MIXED_BITRATE) --------------------------------------
// Packet rows are MAX_PACKET_BYTES apart; a row is received iff its size is one of the codec's (PacketSizeToNumQuantizedBits,
// lyra_config.h:99-106); 0 is "no packet", any other size is counted as an error and treated as no packet.
constexpr int MAX_PACKET_BYTES = 23;    // LYRA_HIP_MAX_PACKET_BYTES
LYRA_LOSSY_HD inline bool mixed_received(int pb) { return pb == 8 || pb == 15 || pb == MAX_PACKET_BYTES; }
// v is a size, or with from_bits (run_steps, decode-only) a bit count of the schedule: size (bits + 7) / 8, negative -> -1
LYRA_LOSSY_HD inline int mixed_bytes(int v, int from_bits) { return !from_bits ? v : v < 0 ? -1 : (int)(((unsigned)v + 7u) >> 3); }

}  // namespace lyra
