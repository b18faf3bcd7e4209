// decode_samples_streams_plan.h -- what lyra_hip_decode_samples_streams_dev adds to decode_samples_any_plan.h: a sample rate,
// a request size and an output offset PER ROW of one call.
//
// Row b of the call is row b of lyra_hip_decode_samples_any_dev(num_samples[b], sample_rates[b]); the only new decisions are
//   the row verdict:  is (rate, n) a request of the any-size call, does it fit the rounds the call enqueues (max_hops: a
//                     launch count, so the host fixes it before the device has seen the rows), and does [offset, offset + n)
//                     lie inside the caller's buffer of n_pcm samples.  A row that fails runs as a row without a packet and
//                     with a request of 0 samples;
//   the rounds of a batch:  the largest ds_any_rounds over its rows, at least 1 (the plan that delivers the packets);
//   the packed layout:  rows back to back in batch order, offsets the running sum of the sizes.
// The plan kernel (decode_samples_streams_kernels.hip), lyra_hip_decode_samples_streams_begin's host check
// (decode_samples_streams_api.inc), MixedAnySizeDeviceLyraDecoder (host/lyra_mixed_device_decoder.cc) and the tests use these
// functions and no second copy.  Host and device code and a plain C++ compiler share this file.
#pragma once
#include <stdint.h>

#include "decode_samples_any_plan.h"

namespace lyra {

// samples between rows when the caller gives no offsets: the largest request (4 hops at 48 kHz,
// LYRA_HIP_DECODE_SAMPLES_MAX_HOPS * LYRA_HIP_MAX_EXT_HOP)
constexpr int DSS_ROW_STRIDE = DSA_MAX_HOPS * 960;

enum DssVerdict : int32_t { DSS_OK = 0, DSS_BAD_RATE = 1, DSS_BAD_SIZE = 2, DSS_BAD_ROUNDS = 3, DSS_BAD_OFFSET = 4 };

// the per-call words of a row, written by round 0 of the plan kernel: ds_plan_any_kernel's four, then the row as validated
//   [0] old leftover count  [1] used  [2] n_int  [3] new count  [4] DssVerdict  [5] n (0 for an invalid row)  [6] rate  [7] 0
constexpr int DSS_CALL_WORDS = 8;

LYRA_LOSSY_HD inline long dss_default_offset(int b) { return (long)b * DSS_ROW_STRIDE; }

// (rate, n) alone: what a host check can decide without the buffer
LYRA_LOSSY_HD inline int dss_size_verdict(int sample_rate_hz, int num_samples) {
  if (sample_rate_hz != 8000 && sample_rate_hz != 16000 && sample_rate_hz != 32000 && sample_rate_hz != 48000) return DSS_BAD_RATE;
  if (!ds_any_valid(num_samples, sample_rate_hz)) return DSS_BAD_SIZE;
  return DSS_OK;
}

// the row verdict; the first failing test names it
LYRA_LOSSY_HD inline int dss_row_verdict(int sample_rate_hz, int num_samples, int max_hops, long offset, long n_pcm_samples) {
  const int v = dss_size_verdict(sample_rate_hz, num_samples);
  if (v != DSS_OK) return v;
  if (ds_any_rounds(num_samples, sample_rate_hz) > max_hops) return DSS_BAD_ROUNDS;
  // (offset + n cannot overflow: n <= DSS_ROW_STRIDE and the comparison is made on the side that stays small)
  if (offset < 0 || offset > n_pcm_samples || (long)num_samples > n_pcm_samples - offset) return DSS_BAD_OFFSET;
  return DSS_OK;
}

// rounds a batch needs: 1..DSA_MAX_HOPS over rows that pass dss_size_verdict (others ask for nothing)
inline int dss_batch_rounds(const int32_t* sample_rates, const int32_t* num_samples, int B) {
  int R = 1;
  for (int b = 0; b < B; ++b) {
    if (dss_size_verdict(sample_rates[b], num_samples[b]) != DSS_OK) continue;
    const int r = ds_any_rounds(num_samples[b], sample_rates[b]);
    if (r > R) R = r;
  }
  return R;
}

// packed layout: offsets[b] = sum of num_samples[0..b), returns the total (negative sizes count as 0)
inline long dss_packed_offsets(const int32_t* num_samples, int B, long* offsets) {
  long total = 0;
  for (int b = 0; b < B; ++b) {
    if (offsets) offsets[b] = total;
    if (num_samples[b] > 0) total += num_samples[b];
  }
  return total;
}

}  // namespace lyra
