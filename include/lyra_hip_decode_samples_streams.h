/* lyra_hip_decode_samples_streams.h -- DecodeSamples(n) on the device with a sample rate and a request size PER STREAM.
 *
 * lyra_hip_decode_samples_any_dev (lyra_hip_decode_samples_any.h) takes one num_samples and one sample_rate_hz for the whole
 * batch; lyra_hip_decode_streams_dev (lyra_hip_decode_streams.h) takes a rate per stream but serves exactly one hop.  A host
 * whose receivers differ in both -- an 8 kHz leg that pulls 160 samples beside a 48 kHz callback of 1024 and a 32 kHz one of
 * 441 -- had to make one call per (rate, size) class.  The calls below serve them in one.
 *
 * lyra_hip_decode_samples_streams_dev
 *   Meaning of a row: row b is, bit for bit, row b of lyra_hip_decode_samples_any_dev(..., d_num_samples[b],
 *   d_sample_rates[b], ...): samples, both flags and every byte of stream state (the loss state machine, the feature FIFO,
 *   held hops, estimator, resampler slot, leftover count and samples, comfort-noise generator).  A stream may move between
 *   this call and the uniform call from request to request without a reset.  Packet conventions, the FIFO depth and
 *   lyra_hip_decode_samples_errors are those of lyra_hip_decode_samples_dev.
 *   Output: row b's d_num_samples[b] samples go to d_pcm + d_pcm_offsets[b] (in samples); a NULL d_pcm_offsets stands for
 *   b * (LYRA_HIP_DECODE_SAMPLES_MAX_HOPS * LYRA_HIP_MAX_EXT_HOP).  Offsets have no alignment rule: rows of 441 samples may lie
 *   back to back.  An offset is valid when it is non-negative and [offset, offset + n) lies inside [0, n_pcm_samples).
 *   Rounds: the reference loop runs in rounds of at most one hop, and the number of rounds is a launch count, so the host must
 *   know it: the call enqueues max_hops (1..LYRA_HIP_DECODE_SAMPLES_MAX_HOPS) of them.  A row is in range when
 *   ceil(n * 16000 / rate) <= 320 * max_hops (the leftover only shortens it).
 *   Invalid rows: a row whose rate is not 8000 / 16000 / 32000 / 48000, whose n is outside 0 .. 4 * rate / 50, which needs more
 *   rounds than max_hops or whose offset is bad runs as a row with NO packet and a request of 0 samples: nothing is written to
 *   d_pcm, no byte of its state changes, its packet is not delivered, its flags are those of a 0-sample request.  It is counted
 *   once in lyra_hip_rates_errors.  Valid rows of the same call are unaffected.
 *   Argument errors: a null d_stream_ids, d_packets, d_packet_bytes, d_sample_rates, d_num_samples or d_pcm, B out of range,
 *   max_hops outside 1..4 or a negative n_pcm_samples is LYRA_HIP_EINVAL with nothing enqueued.
 *   Equivalence: with every rate and every size equal, offsets b * n and max_hops the rounds of that request (1 for n == 0)
 *   the call produces what lyra_hip_decode_samples_any_dev produces.
 *   Streams and ordering: one decode-side call and one noise call under rules (1) to (3) of "Streams"; outputs complete on
 *   the noise stream; LYRA_HIP_SUBBATCHES > 1 accepted (not split); lyra_hip_set_serial supported.
 *
 * lyra_hip_decode_samples_streams_begin / _end
 *   The two-deep host-buffer form, as lyra_hip_decode_samples_any_begin / _end.  begin() checks on the host: stream ids (range,
 *   duplicates), every rate, every size and every packet size (0, 8, 15 or 23); a failed check is LYRA_HIP_EINVAL with nothing
 *   enqueued and nothing changed.  It computes max_hops from its arrays, lays the rows back to back in batch order (offsets =
 *   the running sum of num_samples), allocates everything it needs, copies its arguments into pinned staging (the caller's
 *   arrays are free on return) and enqueues the call.  end() delivers the OLDEST begun request: the packed samples
 *   (sum of num_samples int16; may be NULL when that sum is 0) and, where asked for, both flag arrays [B].
 *   LYRA_HIP_EINVAL, nothing enqueued: a third begin(), an end() with nothing in flight, and a begin() while
 *   lyra_hip_decode_begin, lyra_hip_decode_streams_begin, lyra_hip_decode_samples_begin or lyra_hip_decode_samples_any_begin has
 *   a request in flight; those refuse in turn while a request of this pipeline is.  lyra_hip_export_streams /
 *   lyra_hip_import_streams are refused while a request is outstanding. */
#ifndef LYRA_HIP_DECODE_SAMPLES_STREAMS_H_
#define LYRA_HIP_DECODE_SAMPLES_STREAMS_H_

#include "lyra_hip_decode_samples_any.h"

#ifdef __cplusplus
extern "C" {
#endif

int lyra_hip_decode_samples_streams_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B,
                                        const uint8_t* d_packets /* [B][23] */, const int32_t* d_packet_bytes /* [B] */,
                                        const int32_t* d_sample_rates /* [B] */, const int32_t* d_num_samples /* [B] */,
                                        int max_hops /* 1..4 */, int16_t* d_pcm, long n_pcm_samples,
                                        const int32_t* d_pcm_offsets /* [B] samples, or NULL */,
                                        int32_t* d_is_noise /* [B], or NULL */, int32_t* d_is_comfort_noise /* [B], or NULL */);
int lyra_hip_decode_samples_streams_begin(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B,
                                          const uint8_t* packets /* [B][23] */, const int32_t* packet_bytes /* [B] */,
                                          const int32_t* sample_rates /* [B] */, const int32_t* num_samples /* [B] */);
int lyra_hip_decode_samples_streams_end(lyra_hip_ctx* ctx, int16_t* pcm /* packed */, int32_t* is_noise /* [B], or NULL */,
                                        int32_t* is_comfort_noise /* [B], or NULL */);

#ifdef __cplusplus
}
#endif
#endif  /* LYRA_HIP_DECODE_SAMPLES_STREAMS_H_ */
