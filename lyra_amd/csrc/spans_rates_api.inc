// spans_rates_api.inc -- part of api.hip, behind spans_mixed_api.inc: the span calls with a sample rate per span
// (include/lyra_hip_spans_rates.h).  The steps of a span call run at 16 kHz and never see the external rate, so these are the
// uniform calls' bodies -- spans_call_dev, encode_spans_planned_dev (spans_api.inc) and decode_spans_lossy_sized_dev
// (spans_lossy_api.inc) -- with a SpanExt that holds the caller's array of rates: the rows of the passes over every frame carry
// their span's rate and the passes are the kernels of spans_rates_kernels.hip, launch for launch the uniform call's.
// External-rate rows are MAX_EXT_HOP samples apart, packet rows as in the twin each call is named after.  Device-buffer forms
// only: the header says why.
#include "../../include/lyra_hip_spans_rates.h"

namespace {

// what the forms of a rates call check before anything else: the context and the array of rates itself (its values: span_check)
int span_rates_head(lyra_hip_ctx* c, const char* what, int side, const int* num_bits, const int32_t* sample_rates) {
  const int rc = span_check_head(c, what, side, num_bits, 16000);
  if (rc) return rc;
  if (!sample_rates) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  return 0;
}

}  // namespace

extern "C" {

int lyra_hip_encode_spans_rates_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                    const int16_t* d_pcm_ext, const int32_t* sample_rates, int16_t* d_pcm16,
                                    const int32_t* num_bits, int dtx, uint8_t* d_packets, int32_t* d_packet_bytes) {
  const char* what = "encode_spans_rates";
  const int rc = span_rates_head(c, what, sp::SIDE_ENC, nullptr, sample_rates);
  if (rc) return rc;
  if (!num_bits) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  return encode_spans_planned_dev(c, what, spans, n_spans, lane_ids, n_lanes, d_pcm_ext, 0, d_pcm16, 0, num_bits, dtx != 0,
                                  d_packets, d_packet_bytes, sample_rates);
}

int lyra_hip_decode_spans_lossy_rates_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                          int n_lanes, const uint8_t* d_packets, const int32_t* packet_bytes,
                                          const int32_t* sample_rates, int16_t* d_pcm16, int16_t* d_pcm_ext, int32_t* d_is_noise,
                                          int32_t* d_is_comfort_noise) {
  const char* what = "decode_spans_lossy_rates";
  const int rc = span_rates_head(c, what, sp::SIDE_DEC, nullptr, sample_rates);
  if (rc) return rc;
  return decode_spans_lossy_sized_dev(c, what, spans, n_spans, lane_ids, n_lanes, d_packets, packet_bytes, 0, true, 0, d_pcm16,
                                      d_pcm_ext, d_is_noise, d_is_comfort_noise, sample_rates);
}

int lyra_hip_decode_spans_rates_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                    const uint8_t* d_packets, int num_bits, const int32_t* sample_rates, int16_t* d_pcm16,
                                    int16_t* d_pcm_ext) {
  const char* what = "decode_spans_rates";
  const int rc = span_rates_head(c, what, sp::SIDE_DEC, &num_bits, sample_rates);
  if (rc) return rc;
  return spans_call_dev(c, sp::SIDE_DEC, spans, n_spans, lane_ids, n_lanes, d_packets, num_bits, d_pcm_ext,
                        SpanExt{16000, d_pcm16, sample_rates}, what);
}

}  // extern "C"
