/* lyra_hip_decode_streams.h -- decoders of any sample rate and packet size in one batch: the hop-synchronous receiver.
 *
 * LyraDecoder::Create takes one setting per object, the sample rate (lyra_decoder.cc:86-142); the bitrate comes with each
 * packet's size (SetEncodedPacket, lyra_decoder.cc:172-179).  lyra_hip_decode_lossy_rates_dev (lyra_hip.h, "Per-stream sample
 * rates") serves both per row, into rows padded to LYRA_HIP_MAX_EXT_HOP samples; here the rows may be packed back to back, the
 * 16 kHz hop is optional, and the call has a two-deep host-buffer form.  At most one packet and exactly one hop per stream and
 * call; other request sizes: lyra_hip_decode_samples_dev.  The counterpart of lyra_hip_encode_streams.h.
 *
 * lyra_hip_decode_streams_dev
 *   Row b is, bit for bit, row b of lyra_hip_decode_lossy_rates_dev: the 16 kHz hop (where d_pcm16 is given), the
 *   d_sample_rates[b] / 50 external samples, both flags and every byte of the stream's state -- loss state, generative model,
 *   decoder-side estimator, resampler slot, comfort-noise generator.  A stream may move between the two calls, and between
 *   either and the uniform calls at its rate, from hop to hop without a reset.  With d_pcm_offsets == NULL, n_pcm_samples ==
 *   B * LYRA_HIP_MAX_EXT_HOP and d_pcm16 given the call IS lyra_hip_decode_lossy_rates_dev.
 *   Audio: row b's samples go to d_pcm + d_pcm_offsets[b]; d_pcm_offsets == NULL stands for b * LYRA_HIP_MAX_EXT_HOP.
 *   n_pcm_samples is the length of d_pcm.  The rule for an offset is the encode side's, so one layout serves both directions:
 *   non-negative, a multiple of 8 samples, and [offset, offset + rate / 50) inside [0, n_pcm_samples).  Every valid row length
 *   is a multiple of 160 samples, so rows laid back to back in any order always qualify.  A row with an invalid offset is
 *   treated exactly as a row with an invalid rate: its tick runs as at 16 kHz (d_pcm16, loss state, estimator and flags as
 *   usual), nothing is written to d_pcm for it, its resampler slot is neither read nor written, and it is counted in
 *   lyra_hip_rates_errors; it never writes outside the buffer.  Valid rows that overlap are a caller error: the audio in the
 *   overlap is unspecified, nothing outside the rows is touched.  A 16 kHz row has no resampler (lyra_decoder.cc:129): its
 *   slot is untouched and it receives the 320 samples of the hop.
 *   d_packet_bytes as in lyra_hip_decode_lossy_mixed_dev: 0 (no packet on this hop) / 8 / 15 / 23; anything else counts as
 *   "no packet" and is counted in lyra_hip_decode_lossy_errors.
 *   d_pcm16 == NULL: the 16 kHz hop goes to library scratch (allocated on the first such call).
 *   Streams and ordering: one decode-side call under rules (1) to (3) of "Streams"; outputs complete on the noise stream;
 *   LYRA_HIP_SUBBATCHES > 1 accepted (not split); lyra_hip_set_serial supported.  A null required pointer (d_stream_ids,
 *   d_packets, d_packet_bytes, d_sample_rates, d_pcm), B out of range or n_pcm_samples < 0: LYRA_HIP_EINVAL, nothing enqueued.
 *
 * lyra_hip_decode_streams_begin / _end
 *   The two-deep host-buffer form: begin() copies ids, packets, packet_bytes and rates into pinned staging at call time -- 23
 *   bytes and three words per stream; the caller's arrays are free on return, and begin() does not synchronise --, lays the rows
 *   out back to back in batch order (offsets = the running sum of sample_rates[b] / 50), enqueues the call with d_pcm16 ==
 *   NULL and, behind it on the noise stream, one download of the packed samples and the two flag arrays.  end() waits for the
 *   OLDEST begun hop only and copies out: pcm PACKED, sum of sample_rates[b] / 50 samples; is_noise / is_comfort_noise [B] or
 *   NULL.  With begin(n + 1) issued before end(n) the copies run under the kernels.
 *   begin() checks on the host -- stream ids (range, duplicates), every rate (one of the four), every packet size (0 / 8 / 15 /
 *   23) -- and returns LYRA_HIP_EINVAL with nothing enqueued and nothing changed.  Likewise a third begin(), an end() with
 *   nothing in flight, and mixing with lyra_hip_decode_begin or lyra_hip_decode_samples_begin while either kind has a request
 *   in flight (those two refuse in turn while a hop of this pipeline is).  Everything the hop allocates is allocated before its
 *   upload is enqueued, so an allocation failure (LYRA_HIP_EHIP) enqueues nothing either; only a HIP error raised while the
 *   upload and the kernels are being enqueued can leave part of a hop on the streams: the hop is then not in flight (no end()
 *   is owed) and the streams it named are in an unspecified state.
 *   lyra_hip_export_streams / lyra_hip_import_streams are refused while a hop is outstanding, as for the other pipelined
 *   calls; lyra_hip_reset_streams drains the context first. */
#ifndef LYRA_HIP_DECODE_STREAMS_H_
#define LYRA_HIP_DECODE_STREAMS_H_

#include "lyra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lyra_hip_decode_streams_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const uint8_t* d_packets /* [B][23] */,
                                const int32_t* d_packet_bytes /* [B] */, const int32_t* d_sample_rates /* [B] */,
                                int16_t* d_pcm /* n_pcm_samples */, long n_pcm_samples,
                                const int32_t* d_pcm_offsets /* [B] samples, or NULL: b * LYRA_HIP_MAX_EXT_HOP */,
                                int16_t* d_pcm16 /* [B][320], or NULL */, int32_t* d_is_noise /* [B], or NULL */,
                                int32_t* d_is_comfort_noise /* [B], or NULL */);
int lyra_hip_decode_streams_begin(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const uint8_t* packets /* [B][23] */,
                                  const int32_t* packet_bytes /* [B] */, const int32_t* sample_rates /* [B] */);
int lyra_hip_decode_streams_end(lyra_hip_ctx* ctx, int16_t* pcm /* packed */, int32_t* is_noise /* [B], or NULL */,
                                int32_t* is_comfort_noise /* [B], or NULL */);

#ifdef __cplusplus
}
#endif
#endif  /* LYRA_HIP_DECODE_STREAMS_H_ */
