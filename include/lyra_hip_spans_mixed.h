/* lyra_hip_spans_mixed.h -- time-parallel spans with a bitrate per FRAME: the span calls of lyra_hip.h ("Time-parallel spans") for
 * recordings whose bitrate changes between hops, as LyraEncoder::set_bitrate makes them and LyraDecoder::SetEncodedPacket reads
 * them.  Five functions, a header of their own; everything else -- the context, lyra_hip_span, lyra_hip_span_chunk,
 * lyra_hip_span_lossy_counts, LYRA_HIP_MAX_PACKET_BYTES, the error codes -- is lyra_hip.h's, which this header includes. */
#ifndef LYRA_HIP_SPANS_MIXED_H_
#define LYRA_HIP_SPANS_MIXED_H_

#include "lyra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Time-parallel spans, per-frame bitrates -------------------------------------------------------------------------------------
 * Neither side keeps state that depends on the bitrate (lyra_hip.h, lyra_hip_encode_mixed_dev): the quantizer is a pure function
 * of the hop's features, and the RVQ decode of the hop's packet.  So the planner, the lanes, the warm-up, the ring phases and the
 * hand-over of the uniform span calls apply UNCHANGED, and what these calls add is a bit count or packet size that travels with
 * every row of every step.  Per span frame and per span stream they give BIT FOR BIT what the hop-by-hop mixed calls give:
 *   encode   row f and packet_bytes[f] are those of lyra_hip_encode_mixed_dev(sample_rate_hz, num_bits = num_bits[f], dtx) for that
 *            stream on that hop;
 *   decode   pcm16, pcm_ext, is_noise, is_comfort_noise of frame f are those of lyra_hip_decode_lossy_mixed_dev with that hop's
 *            packet_bytes[f];
 *   state    lyra_hip_export_streams of the span streams afterwards returns the hop-by-hop stream's bytes.  A span continues a
 *            live stream (mid-burst included on the decode side) and may be continued hop by hop, or by a uniform span call: a
 *            stream may move between the uniform and the mixed span calls.
 *   Packet rows are LYRA_HIP_MAX_PACKET_BYTES apart in both directions.  Spans, lanes, frame-major buffers, alignment, rates and
 *   the workspace d_pcm16 are the uniform calls'; lanes come back reset; frames outside every span are untouched in every buffer.
 *   num_bits (encode) and packet_bytes (decode) are HOST arrays [frames] like spans and lane_ids, copied at call time; only the
 *   entries of span frames are read.
 *   Each call is ONE call of its side for rules (1) to (3) of "Streams" and runs on lyra_hip_stream() / lyra_hip_stream_decode(),
 *   the packets too: the quantizer stream is not used.  Per step a call enqueues as many kernels as its uniform twin.
 *   The `_dev` forms allocate nothing beyond the side's grow-only scratch, and every refusal comes before the first kernel:
 *   LYRA_HIP_EINVAL with nothing enqueued and no state changed.  lyra_hip_encode_mixed_errors() reads 0 after any of them.
 *   The host-buffer forms stage frames 0 .. the last span's end, run, synchronise and write the spans' frames of the outputs.
 * Per-span sample rates: lyra_hip_spans_rates.h, which includes this header.
 * Out of scope: request sizes other than one hop on spans. */

/* LyraEncoder::Encode with set_bitrate between hops, over spans.  num_bits is a HOST array [frames]: a multiple of 4 in 4..184 for
 * EVERY frame of every span (frames outside spans are not read), else LYRA_HIP_EINVAL with nothing enqueued.  Bytes past
 * packet_bytes[f] of a row are never written (`_dev`) / read back as zero (host form).  sample_rate_hz and d_pcm16: as
 * lyra_hip_encode_spans_ext_dev (d_pcm16 may be NULL at 16000).  dtx != 0: as lyra_hip_encode_spans_dtx_dev -- it needs
 * lyra_hip_set_encoder_sample_rate(sample_rate_hz), blocks the host once, and num_bits is still checked for every span frame,
 * noise or not.  d_packet_bytes [frames] is required: (num_bits[f] + 7) / 8, or 0 for a DTX noise frame, whose row is not written
 * (host form: left zero). */
int lyra_hip_encode_spans_mixed_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                    int n_lanes, const int16_t* d_pcm_ext /* [frames][rate / 50] */, int sample_rate_hz,
                                    int16_t* d_pcm16 /* [frames][320] workspace; may be NULL at 16000 */,
                                    const int32_t* num_bits /* HOST [frames] */, int dtx,
                                    uint8_t* d_packets /* [frames][23] */, int32_t* d_packet_bytes /* [frames], required */);
int lyra_hip_encode_spans_mixed(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                const int16_t* pcm_ext, int sample_rate_hz, const int32_t* num_bits, int dtx, uint8_t* packets,
                                int32_t* packet_bytes);

/* lyra_hip_decode_spans_lossy[_dev] with the size chosen per frame as SetEncodedPacket does: HOST packet_bytes[f] in
 * {0, 8, 15, 23}; anything else on a span frame: LYRA_HIP_EINVAL, nothing enqueued, no state changed.  Everything else -- outputs,
 * optional pointers, state, streams, the one host wait at its start, the "do not mix" rules -- is lyra_hip_decode_spans_lossy_dev's. */
int lyra_hip_decode_spans_lossy_mixed_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                          int n_lanes, const uint8_t* d_packets /* [frames][23] */,
                                          const int32_t* packet_bytes /* HOST [frames]: 0 / 8 / 15 / 23 */, int sample_rate_hz,
                                          int16_t* d_pcm16 /* [frames][320], required */,
                                          int16_t* d_pcm_ext /* [frames][rate / 50]; may be NULL at 16000 */,
                                          int32_t* d_is_noise /* [frames] or NULL */,
                                          int32_t* d_is_comfort_noise /* [frames] or NULL */);
int lyra_hip_decode_spans_lossy_mixed(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                      int n_lanes, const uint8_t* packets, const int32_t* packet_bytes, int sample_rate_hz,
                                      int16_t* pcm16, int16_t* pcm_ext, int32_t* is_noise, int32_t* is_comfort_noise);

/* lyra_hip_spans_lossy_plan without packet_size: sizes 0 / 8 / 15 / 23 per frame.  Same outputs, and for the same receive pattern
 * the same values, except that gen_bytes (in the place of gen_received) holds 0 for a concealed tick and the packet's size for a
 * tick fed from its packet.  LYRA_HIP_EINVAL for what lyra_hip_spans_lossy_plan refuses and for any other size on a span frame. */
int lyra_hip_spans_lossy_plan_mixed(const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes, int max_streams,
                                    const int32_t* packet_bytes, const uint32_t* ctl_in, lyra_hip_span_lossy_counts* counts,
                                    int64_t* gen_frames, uint8_t* gen_bytes, int64_t* rx_frames, int64_t* cng_frames,
                                    int32_t* cng_versions, int32_t* versions, int32_t* info, lyra_hip_span_chunk* chunks, int cap,
                                    int* n_steps);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif  /* LYRA_HIP_SPANS_MIXED_H_ */
