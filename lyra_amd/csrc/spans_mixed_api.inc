// spans_mixed_api.inc -- part of api.hip, behind spans_lossy_api.inc: the span calls with a bitrate per frame
// (include/lyra_hip_spans_mixed.h).  Nothing in the codec state depends on the bitrate, so these are the uniform calls' bodies --
// encode_spans_planned_dev (spans_api.inc), decode_spans_lossy_sized_dev and spans_lossy_plan_sized (spans_lossy_api.inc) -- with
// a bit count or packet size that travels with every row of every step (spans_mixed_kernels.hip) to rvq_encode_mixed_kernel /
// rvq_decode_mixed_kernel on the side's own stream.  Packet rows are MAX_PACKET_BYTES apart.
#include "../../include/lyra_hip_spans_mixed.h"

extern "C" {

int lyra_hip_encode_spans_mixed_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                    const int16_t* d_pcm_ext, int sample_rate_hz, int16_t* d_pcm16, const int32_t* num_bits, int dtx,
                                    uint8_t* d_packets, int32_t* d_packet_bytes) {
  const char* what = "encode_spans_mixed";
  if (!c) return LYRA_HIP_EINVAL;
  if (!num_bits) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  return encode_spans_planned_dev(c, what, spans, n_spans, lane_ids, n_lanes, d_pcm_ext, sample_rate_hz, d_pcm16, 0, num_bits,
                                  dtx != 0, d_packets, d_packet_bytes);
}

// host-buffer form: bytes past packet_bytes of a row, and the rows of noise frames, read back as zeros
int lyra_hip_encode_spans_mixed(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                const int16_t* pcm_ext, int sample_rate_hz, const int32_t* num_bits, int dtx, uint8_t* packets,
                                int32_t* packet_bytes) {
  const char* what = "encode_spans_mixed";
  const int rc = span_check_head(c, what, sp::SIDE_ENC, nullptr, sample_rate_hz);
  if (rc) return rc;
  if (!num_bits || !packet_bytes) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  SpanBuf B[] = {{SPAN_IN, (void*)pcm_ext, (size_t)sample_rate_hz / 50 * 2}, {SPAN_OUT, packets, (size_t)MAX_PACKET_BYTES, true},
                 {SPAN_OUT, packet_bytes, sizeof(int32_t)}, {SPAN_WORK, nullptr, sample_rate_hz != 16000 ? (size_t)640 : 0}};
  return span_staged(c, what, sp::SIDE_ENC, spans, n_spans, B, [&] {
    return lyra_hip_encode_spans_mixed_dev(c, spans, n_spans, lane_ids, n_lanes, (const int16_t*)B[0].d, sample_rate_hz,
                                           (int16_t*)B[3].d, num_bits, dtx, B[1].d, (int32_t*)B[2].d);
  });
}

int lyra_hip_decode_spans_lossy_mixed_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                          int n_lanes, const uint8_t* d_packets, const int32_t* packet_bytes, int sample_rate_hz,
                                          int16_t* d_pcm16, int16_t* d_pcm_ext, int32_t* d_is_noise, int32_t* d_is_comfort_noise) {
  return decode_spans_lossy_sized_dev(c, "decode_spans_lossy_mixed", spans, n_spans, lane_ids, n_lanes, d_packets, packet_bytes, 0,
                                      true, sample_rate_hz, d_pcm16, d_pcm_ext, d_is_noise, d_is_comfort_noise);
}

// host-buffer form: is_noise / is_comfort_noise may be null, pcm_ext at 16000 too
int lyra_hip_decode_spans_lossy_mixed(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                      const uint8_t* packets, const int32_t* packet_bytes, int sample_rate_hz, int16_t* pcm16,
                                      int16_t* pcm_ext, int32_t* is_noise, int32_t* is_comfort_noise) {
  const char* what = "decode_spans_lossy_mixed";
  const int rc = span_check_head(c, what, sp::SIDE_DEC, nullptr, sample_rate_hz);
  if (rc) return rc;
  const bool ext = sample_rate_hz != 16000;
  auto opt = [](void* host, size_t bytes) { return SpanBuf{host ? SPAN_OUT : SPAN_WORK, host, host ? bytes : 0}; };
  SpanBuf B[] = {{SPAN_IN, (void*)packets, (size_t)MAX_PACKET_BYTES}, {SPAN_OUT, pcm16, 640},
                 ext ? SpanBuf{SPAN_OUT, pcm_ext, (size_t)sample_rate_hz / 50 * 2} : SpanBuf{SPAN_WORK, nullptr, 0},
                 opt(is_noise, sizeof(int32_t)), opt(is_comfort_noise, sizeof(int32_t))};
  return span_staged(c, what, sp::SIDE_DEC, spans, n_spans, B, [&] {
    return lyra_hip_decode_spans_lossy_mixed_dev(c, spans, n_spans, lane_ids, n_lanes, B[0].d, packet_bytes, sample_rate_hz,
                                                 (int16_t*)B[1].d, (int16_t*)B[2].d, (int32_t*)B[3].d, (int32_t*)B[4].d);
  });
}

int lyra_hip_spans_lossy_plan_mixed(const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes, int max_streams,
                                    const int32_t* packet_bytes, const uint32_t* ctl_in, lyra_hip_span_lossy_counts* counts,
                                    int64_t* gen_frames, uint8_t* gen_bytes, int64_t* rx_frames, int64_t* cng_frames,
                                    int32_t* cng_versions, int32_t* versions, int32_t* info, lyra_hip_span_chunk* chunks, int cap,
                                    int* n_steps) {
  return spans_lossy_plan_sized(spans, n_spans, lane_ids, n_lanes, max_streams, packet_bytes, slp::SIZE_PER_FRAME, ctl_in, counts,
                                gen_frames, gen_bytes, rx_frames, cng_frames, cng_versions, versions, info, chunks, cap, n_steps);
}

}  // extern "C"
