/* lyra_hip_spans_rates.h -- time-parallel spans with a sample rate per SPAN: the span calls of lyra_hip.h ("Time-parallel spans")
 * and of lyra_hip_spans_mixed.h for a batch of recordings at 8, 16, 32 and 48 kHz side by side.  Three functions on device
 * buffers, a header of their own; everything else -- the context, lyra_hip_span, LYRA_HIP_MAX_EXT_HOP,
 * LYRA_HIP_MAX_PACKET_BYTES, the error codes -- comes with lyra_hip_spans_mixed.h, which this header includes. */
#ifndef LYRA_HIP_SPANS_RATES_H_
#define LYRA_HIP_SPANS_RATES_H_

#include "lyra_hip_spans_mixed.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Time-parallel spans, per-span sample rates -----------------------------------------------------------------------------------
 * The codec core, the planner, the lanes, the warm-up and the hand-over all run at 16 kHz and never see the external rate; the
 * resampler's state is 34 input samples and a phase; the DTX estimator reads the 16 kHz audio alone, and the decoder-side
 * estimator is a 16 kHz one at every rate.  So these calls are the span forms of lyra_hip_encode_rates_dev /
 * lyra_hip_decode_lossy_rates_dev: the rate travels with each span instead of with the call.  sample_rates is a HOST array
 * [n_spans] like spans, copied at call time: sample_rates[s] in {8000, 16000, 32000, 48000} is the rate of spans[s].
 *   External-rate PCM is frame-major [frames][LYRA_HIP_MAX_EXT_HOP] int16, 16-byte aligned: a frame of span s holds
 *   sample_rates[s] / 50 samples at the front of its row; the rest of the row is never read by encode and never written by decode.
 *   d_pcm16 [frames][320], 16-byte aligned, is ALWAYS required.  After encode it holds the 16 kHz audio of every span frame (for a
 *   16 kHz span a copy of the row's first 320 samples; no resampler slot is touched); after decode the 16 kHz output, and a
 *   16 kHz span gets its 320 samples copied into its d_pcm_ext row as lyra_hip_decode_lossy_rates_dev does.
 * Per span frame and per span stream everything is BIT FOR BIT what lyra_hip_encode_rates_dev / lyra_hip_decode_lossy_rates_dev
 * give hop by hop at that stream's rate (plain decode: lyra_hip_decode_dev + lyra_hip_resample_dev(DECODER)), which by lyra_hip.h's
 * own statement equals the uniform calls at that rate; lyra_hip_export_streams returns the same bytes afterwards.  A span
 * continues a live stream -- mid-burst and with a non-zero decimation phase included -- and may be continued hop by hop, by a
 * uniform span call at its rate, or by another of these calls.
 *   With dtx each span's NoiseEstimator runs with the constants and the mel filterbank of its own rate;
 *   lyra_hip_set_encoder_sample_rate is not read.
 *   Spans, lanes, streams and ordering are the uniform calls': each call is ONE call of its side, everything completes on
 *   lyra_hip_stream() / lyra_hip_stream_decode(), the DTX encode and the lossy decode block the host once as their uniform twins
 *   do, lanes come back reset, frames outside every span are untouched in every buffer, and per step a call enqueues as many
 *   kernels as its uniform twin.  LYRA_HIP_SUBBATCHES > 1 and lyra_hip_set_serial are supported.
 *   Any rate other than the four, a null sample_rates, a null or misaligned d_pcm16 / d_pcm_ext, and whatever the uniform twin
 *   refuses: LYRA_HIP_EINVAL before the first kernel, with no state changed and lyra_hip_rates_errors() unchanged.
 *   Device-buffer (`_dev`) forms on the padded layout only.  Host-buffer forms and a packed (unpadded) external-rate layout, which
 *   takes a sixth of this one's memory at 8 kHz: lyra_hip_spans_packed.h, which includes this header.
 * Out of scope: request sizes other than one hop on spans. */

/* lyra_hip_encode_spans_mixed_dev with a rate per span.  num_bits HOST [frames] (a multiple of 4 in 4..184 on every span frame),
 * dtx, d_packets rows LYRA_HIP_MAX_PACKET_BYTES apart and the required d_packet_bytes: as there. */
int lyra_hip_encode_spans_rates_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                    int n_lanes, const int16_t* d_pcm_ext /* [frames][LYRA_HIP_MAX_EXT_HOP] */,
                                    const int32_t* sample_rates /* HOST [n_spans] */,
                                    int16_t* d_pcm16 /* [frames][320], required */,
                                    const int32_t* num_bits /* HOST [frames] */, int dtx,
                                    uint8_t* d_packets /* [frames][23] */, int32_t* d_packet_bytes /* [frames], required */);

/* lyra_hip_decode_spans_lossy_mixed_dev with a rate per span: HOST packet_bytes[f] in {0, 8, 15, 23}, packet rows
 * LYRA_HIP_MAX_PACKET_BYTES apart.  d_pcm16 and d_pcm_ext are both required; d_is_noise / d_is_comfort_noise are optional. */
int lyra_hip_decode_spans_lossy_rates_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                          int n_lanes, const uint8_t* d_packets /* [frames][23] */,
                                          const int32_t* packet_bytes /* HOST [frames]: 0 / 8 / 15 / 23 */,
                                          const int32_t* sample_rates /* HOST [n_spans] */,
                                          int16_t* d_pcm16 /* [frames][320], required */,
                                          int16_t* d_pcm_ext /* [frames][LYRA_HIP_MAX_EXT_HOP], required */,
                                          int32_t* d_is_noise /* [frames] or NULL */,
                                          int32_t* d_is_comfort_noise /* [frames] or NULL */);

/* lyra_hip_decode_spans_ext_dev (no loss, one num_bits for the call, packet rows (num_bits + 7) / 8 apart) with a rate per span:
 * the fast path of a file transcode.  Nothing blocks the host. */
int lyra_hip_decode_spans_rates_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                    int n_lanes, const uint8_t* d_packets /* [frames][(num_bits + 7) / 8] */, int num_bits,
                                    const int32_t* sample_rates /* HOST [n_spans] */,
                                    int16_t* d_pcm16 /* [frames][320], required */,
                                    int16_t* d_pcm_ext /* [frames][LYRA_HIP_MAX_EXT_HOP], required */);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif  /* LYRA_HIP_SPANS_RATES_H_ */
