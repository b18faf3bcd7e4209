/* lyra_hip_spans_packed.h -- time-parallel spans with a sample rate per span on a PACKED external-rate buffer, and from host
 * buffers: the calls of lyra_hip_spans_rates.h (which this header includes) without the padding of every external-rate row to
 * LYRA_HIP_MAX_EXT_HOP samples.  An 8 kHz recording takes a sixth of the padded layout's memory and bus traffic; four recordings
 * of equal length at 8 / 16 / 32 / 48 kHz take 2,080 samples per hop set against 3,840. */
#ifndef LYRA_HIP_SPANS_PACKED_H_
#define LYRA_HIP_SPANS_PACKED_H_

#include "lyra_hip_spans_rates.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The packed layout -------------------------------------------------------------------------------------------------------
 * External-rate PCM is ONE flat int16 array of n_ext_samples samples, 16-byte aligned on the device.  ext_offsets is a HOST array
 * [n_spans] of 64-bit sample offsets, copied at call time: frame first_frame + k of span s lies at
 *     ext_offsets[s] + k * (sample_rates[s] / 50),
 * sample_rates[s] / 50 samples long, the span's frames back to back.  ext_offsets == NULL stands for the back-to-back layout of
 * lyra_hip_spans_packed_layout: span after span in the order of the list.  first_frame keeps indexing every frame-major buffer:
 * the 16 kHz audio [frames][320], packets, num_bits / packet_bytes, flags.
 *   Bounds: every offset is a multiple of 8 samples (with hops of 160 / 320 / 640 / 960 samples every row is then 16-byte
 *   aligned), and a span with frames starts below 2^34 samples (32 GiB of int16): the kernel carries a span's base in units of 8
 *   samples in a 32-bit word and computes every address in 64 bits.
 *   Refused with LYRA_HIP_EINVAL before the first kernel, with nothing enqueued, no state changed and no error counter moved:
 *   n_ext_samples < 0; a negative offset; an offset that is no multiple of 8; a span with frames whose range leaves
 *   [0, n_ext_samples) or starts at 2^34 or later; two spans with frames whose ranges share a sample (the arrays are host arrays,
 *   so this IS checked, unlike the device-side offsets of lyra_hip_decode_streams_dev); a misaligned d_pcm_ext; and whatever the
 *   call's twin in lyra_hip_spans_rates.h refuses.
 * Everything else is the twin's: d_pcm16 is required, lanes, streams and ordering, the one host wait of the DTX encode and of the
 * lossy decode, LYRA_HIP_SUBBATCHES and lyra_hip_set_serial, each span's DTX estimator at its own rate, as many kernels per step.
 * Only the resampler pass addresses the external-rate buffer (span_resample_packed_kernel): encode reads exactly the spans'
 * samples and writes none; decode writes exactly n_frames * sample_rates[s] / 50 samples from each span's offset and nothing in
 * front, behind or between spans.  A 16 kHz span is copied, 320 samples per frame, and touches no resampler slot.
 * Per span frame and per span stream everything -- packets, sizes, 16 kHz rows, external-rate samples, flags, exported blobs, lanes
 * returned reset -- is BIT FOR BIT what the `_rates_dev` twin gives for the same spans on the padded layout, hence what the
 * hop-by-hop rates calls give.  A span continues a live stream, mid-burst and with a non-zero decimation phase included, and may
 * be continued by any other call of its side.
 * Out of scope: request sizes other than one hop on spans; pipelined forms. */

/* The back-to-back layout; needs no context and no device.  Returns the number of samples: the sum of
 * n_frames * sample_rates[s] / 50 in span order, and fills ext_offsets (optional, [n_spans]) with each span's base -- a span of no
 * frames gets the running sum and takes nothing.  -1: a rate that is none of the four, a negative n_frames, a null spans or
 * sample_rates with n_spans > 0, n_spans < 0. */
long long lyra_hip_spans_packed_layout(const lyra_hip_span* spans, int n_spans, const int32_t* sample_rates,
                                       long long* ext_offsets /* [n_spans] or NULL */);

/* lyra_hip_encode_spans_rates_dev on the packed layout. */
int lyra_hip_encode_spans_packed_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                     int n_lanes, const int16_t* d_pcm_ext /* [n_ext_samples], 16-byte aligned */,
                                     long long n_ext_samples, const long long* ext_offsets /* HOST [n_spans] or NULL */,
                                     const int32_t* sample_rates /* HOST [n_spans] */,
                                     int16_t* d_pcm16 /* [frames][320], required */,
                                     const int32_t* num_bits /* HOST [frames] */, int dtx,
                                     uint8_t* d_packets /* [frames][23] */, int32_t* d_packet_bytes /* [frames], required */);

/* lyra_hip_decode_spans_lossy_rates_dev on the packed layout. */
int lyra_hip_decode_spans_lossy_packed_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                           int n_lanes, const uint8_t* d_packets /* [frames][23] */,
                                           const int32_t* packet_bytes /* HOST [frames]: 0 / 8 / 15 / 23 */,
                                           const int32_t* sample_rates /* HOST [n_spans] */,
                                           int16_t* d_pcm16 /* [frames][320], required */,
                                           int16_t* d_pcm_ext /* [n_ext_samples], 16-byte aligned, required */,
                                           long long n_ext_samples, const long long* ext_offsets /* HOST [n_spans] or NULL */,
                                           int32_t* d_is_noise /* [frames] or NULL */,
                                           int32_t* d_is_comfort_noise /* [frames] or NULL */);

/* lyra_hip_decode_spans_rates_dev on the packed layout.  Nothing blocks the host. */
int lyra_hip_decode_spans_packed_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                     int n_lanes, const uint8_t* d_packets /* [frames][(num_bits + 7) / 8] */, int num_bits,
                                     const int32_t* sample_rates /* HOST [n_spans] */,
                                     int16_t* d_pcm16 /* [frames][320], required */,
                                     int16_t* d_pcm_ext /* [n_ext_samples], 16-byte aligned, required */,
                                     long long n_ext_samples, const long long* ext_offsets /* HOST [n_spans] or NULL */);

/* ---- Host buffers --------------------------------------------------------------------------------------------------------------
 * The same calls on host buffers in the same layout (a host pcm_ext needs no alignment; the offsets' rules hold).  Every check
 * comes first; then ONE upload that holds exactly the spans' samples (encode) or packet rows (decode) -- on the device the spans
 * lie back to back in every buffer, whatever first_frame and ext_offsets say, so no byte outside a span is staged --, the `_dev`
 * form, and ONE download of the spans' own outputs (the decodes: one of the samples, one of the optional frame-major outputs).
 * Where the caller's layout is the back-to-back one (ext_offsets == NULL, or equal to it) the samples travel straight from / to
 * its buffer; otherwise through a host copy in that layout.  The 16 kHz audio lives in the call's staging: the decode forms return it in
 * pcm16 [frames][320] if that is given, the encode form returns none.  Output bytes outside the spans' frames and sample ranges are
 * not written; packet bytes behind packet_bytes[f] and the rows of DTX noise frames read back as zeros, as in
 * lyra_hip_encode_spans_mixed.  The calls block until the outputs are there, as their uniform host twins do, and take and free
 * their staging per call.  Refusals are the `_dev` forms' (a null host buffer that a span frame needs included), with no
 * output byte written. */
int lyra_hip_encode_spans_packed(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                 const int16_t* pcm_ext /* [n_ext_samples] */, long long n_ext_samples,
                                 const long long* ext_offsets /* [n_spans] or NULL */, const int32_t* sample_rates /* [n_spans] */,
                                 const int32_t* num_bits /* [frames] */, int dtx, uint8_t* packets /* [frames][23] */,
                                 int32_t* packet_bytes /* [frames], required */);
int lyra_hip_decode_spans_lossy_packed(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                       int n_lanes, const uint8_t* packets /* [frames][23] */,
                                       const int32_t* packet_bytes /* [frames]: 0 / 8 / 15 / 23 */,
                                       const int32_t* sample_rates /* [n_spans] */, int16_t* pcm16 /* [frames][320] or NULL */,
                                       int16_t* pcm_ext /* [n_ext_samples] */, long long n_ext_samples,
                                       const long long* ext_offsets /* [n_spans] or NULL */, int32_t* is_noise /* [frames] or NULL */,
                                       int32_t* is_comfort_noise /* [frames] or NULL */);
int lyra_hip_decode_spans_packed(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                 const uint8_t* packets /* [frames][(num_bits + 7) / 8] */, int num_bits,
                                 const int32_t* sample_rates /* [n_spans] */, int16_t* pcm16 /* [frames][320] or NULL */,
                                 int16_t* pcm_ext /* [n_ext_samples] */, long long n_ext_samples,
                                 const long long* ext_offsets /* [n_spans] or NULL */);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif  /* LYRA_HIP_SPANS_PACKED_H_ */
