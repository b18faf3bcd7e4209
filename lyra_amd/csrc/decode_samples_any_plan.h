// decode_samples_any_plan.h -- BufferedResampler's leftover (buffered_resampler.cc:63-147) on integers, for
// lyra_hip_decode_samples_any_dev: DecodeSamples(n) for ANY n of 0..4 hops at the four codec rates.
//
// A request that is not a whole number of 16 kHz samples leaves 1 or 2 resampled samples for the next call (at most 2 at
// 48 kHz, 1 at 32 kHz, none at 8 and 16 kHz).  Per stream the leftover is a count and up to two int16, kept in the unused
// bytes 4..15 of the stream's R_RS_D slot (state_layout.h): all zero = empty, which is what context creation, a reset and
// every blob written before this call existed hold there.  ds_any_step is one call's bookkeeping:
//   used  = min(L, n)                        samples served from the leftover
//   n_int = n > L ? ceil((n - L) * 16000 / rate) : 0   internal samples the reference loop generates
//   left  = leftover count after the call
// n_int runs through ds_plan (decode_samples_plan.h) in rounds of at most one hop: round r takes
// clamp(n_int - 320 r, 0, 320) samples, and a call has ds_any_rounds(n, rate) <= 4 of them.
// Host and device code and a plain C++ compiler share this file.
#pragma once
#include <stdint.h>

#include "decode_samples_plan.h"

namespace lyra {

constexpr int DSA_MAX_HOPS = 4;                          // LYRA_HIP_DECODE_SAMPLES_MAX_HOPS
constexpr int DSA_MAX_INTERNAL = DSA_MAX_HOPS * DS_HOP;  // n_int never exceeds it (tests/test_decode_samples_any_plan_cpu.py)
constexpr int DSA_LEFT_MAX = 2;
constexpr int DSA_LEFT_COUNT = 4;     // byte offset in the R_RS_D slot: int32 count 0..DSA_LEFT_MAX (decode stream writes it)
constexpr int DSA_LEFT_SAMPLES = 8;   // int16[2], the oldest first (noise stream writes them); 12..15 stay zero

struct DsaStep { int used, n_int, left; };

LYRA_LOSSY_HD inline bool ds_any_valid(int num_samples, int sample_rate_hz) {
  if (sample_rate_hz != 8000 && sample_rate_hz != 16000 && sample_rate_hz != 32000 && sample_rate_hz != 48000) return false;
  return num_samples >= 0 && num_samples <= DSA_MAX_HOPS * (sample_rate_hz / 50);
}

// internal samples for m external ones, m >= 0: ceil(m * 16000 / rate)
LYRA_LOSSY_HD inline int ds_any_internal(int m, int sample_rate_hz) {
  return (int)(((long)m * 16000 + sample_rate_hz - 1) / sample_rate_hz);
}

// left_count: the stream's leftover count before the call (0..DSA_LEFT_MAX); (num_samples, rate) pass ds_any_valid
LYRA_LOSSY_HD inline DsaStep ds_any_step(int left_count, int num_samples, int sample_rate_hz) {
  DsaStep s;
  s.used = left_count < num_samples ? left_count : num_samples;
  s.n_int = num_samples > left_count ? ds_any_internal(num_samples - left_count, sample_rate_hz) : 0;
  // what the resampler makes of n_int samples (down-sampling: n_int is even, the decimation phase stays 0)
  const int made = sample_rate_hz >= 16000 ? s.n_int * (sample_rate_hz / 16000) : s.n_int / (16000 / sample_rate_hz);
  s.left = s.n_int ? made - (num_samples - s.used) : left_count - s.used;
  return s;
}

// rounds of the call: every row's n_int is at most ceil(n * 16000 / rate)
LYRA_LOSSY_HD inline int ds_any_rounds(int num_samples, int sample_rate_hz) {
  return (ds_any_internal(num_samples, sample_rate_hz) + DS_HOP - 1) / DS_HOP;
}
LYRA_LOSSY_HD inline int ds_any_round_total(int n_int, int round) {
  const int v = n_int - DS_HOP * round;
  return v < 0 ? 0 : v > DS_HOP ? DS_HOP : v;
}

}  // namespace lyra
