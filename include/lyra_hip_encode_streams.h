/* lyra_hip_encode_streams.h -- encoders of any sample rate, bitrate and DTX setting in one batch.
 *
 * A LyraEncoder is created with three settings of its own: sample rate, bitrate and enable_dtx (lyra_encoder.cc:44-111).
 * lyra_hip_encode_rates_dev (lyra_hip.h, "Per-stream sample rates") serves the first two per row; here the third is per row
 * too, the audio rows may be packed back to back, and the call has a two-deep host-buffer form.
 *
 * lyra_hip_encode_streams_dev
 *   Row b is, bit for bit, row b of lyra_hip_encode_rates_dev called with dtx = (d_dtx[b] != 0): the packet, packet_bytes and
 *   every byte of the stream's state.  A row with d_dtx[b] == 0 neither reads nor writes its encoder-side NoiseEstimator slot,
 *   the estimator's log-mel history included -- the reference creates no estimator for such an encoder (lyra_encoder.cc:80).
 *   A stream may move between this call and lyra_hip_encode_rates_dev, and change its flag, from hop to hop without a reset:
 *   the estimator simply does not see the hops on which the flag is off.  d_dtx == NULL: no row uses DTX (no estimator
 *   launch at all); with d_pcm_offsets == NULL as well the call is lyra_hip_encode_rates_dev(dtx = 0).
 *   Audio: row b holds d_sample_rates[b] / 50 samples at d_pcm_ext + d_pcm_offsets[b]; d_pcm_offsets == NULL stands for
 *   b * LYRA_HIP_MAX_EXT_HOP.  n_pcm_samples is the length of d_pcm_ext.  Every valid row length is a multiple of 160 samples,
 *   so rows laid back to back are always aligned.  A row whose offset is negative, is no multiple of 8 samples (16 bytes) or
 *   puts [offset, offset + rate / 50) outside [0, n_pcm_samples) is treated exactly as a row with an invalid rate: it is
 *   absent from the hop (packet_bytes[b] = 0, no state of the stream advances), it is counted in lyra_hip_rates_errors, and
 *   nothing of it is read.  Invalid bit counts behave as in lyra_hip_encode_mixed_dev, invalid rates as in
 *   lyra_hip_encode_rates_dev.
 *   Streams and ordering: one encode-side call under rules (1) to (3) of "Streams"; packets complete on the quantizer stream;
 *   LYRA_HIP_SUBBATCHES > 1 accepted (not split); lyra_hip_set_serial supported; lyra_hip_set_encoder_sample_rate is not read.
 *   With d_dtx given it enqueues as many kernels as lyra_hip_encode_rates_dev(dtx = 1).  A null required pointer, B out of
 *   range or n_pcm_samples < 0: LYRA_HIP_EINVAL, nothing enqueued.
 *
 * lyra_hip_encode_streams_begin / _end
 *   The two-deep host-buffer form (as lyra_hip_encode_begin / _end): begin() uploads a hop and enqueues its kernels and the
 *   download of its packets; end() hands over the oldest begun hop.  With begin(n + 1) issued before end(n) the copies run
 *   under the kernels.  `pcm` is PACKED: row b holds sample_rates[b] / 50 samples, rows back to back, and goes up as one copy
 *   of that size.  begin() returns only after that upload has completed: `pcm` may be overwritten at once.  With another
 *   hop of this pipeline in flight the upload rides on the context's noise stream (lyra_hip_stream_noise), which is also
 *   where decode-side calls finish: in a process that decodes on the SAME context begin() may then wait for decoder
 *   kernels as well (results are unaffected); an encoder context of its own, as MixedBatchLyraEncoder has, waits for the
 *   upload only.
 *   begin() checks on the host -- stream ids (range, duplicates), every rate (one of the four), every bit count (a multiple
 *   of 4 in 4..184) -- and returns LYRA_HIP_EINVAL with nothing enqueued and nothing changed.  Likewise a third begin(), an
 *   end() with nothing in flight, and mixing with lyra_hip_encode_begin while either kind has a call in flight.
 *   end(): packets [B][23] (rows of empty packets and the bytes behind a shorter packet are zero), packet_bytes [B].
 *   lyra_hip_export_streams / lyra_hip_import_streams are refused while a request is outstanding, as for the other pipelined
 *   calls; lyra_hip_reset_streams drains the context first. */
#ifndef LYRA_HIP_ENCODE_STREAMS_H_
#define LYRA_HIP_ENCODE_STREAMS_H_

#include "lyra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int lyra_hip_encode_streams_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const int16_t* d_pcm_ext,
                                long n_pcm_samples,
                                const int32_t* d_pcm_offsets /* [B] samples, or NULL: b * LYRA_HIP_MAX_EXT_HOP */,
                                const int32_t* d_sample_rates /* [B] */, const int32_t* d_num_bits /* [B] */,
                                const int32_t* d_dtx /* [B] 0 / non-zero, or NULL: no row uses DTX */,
                                uint8_t* d_packets /* [B][23] */, int32_t* d_packet_bytes /* [B], required */);
int lyra_hip_encode_streams_begin(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B,
                                  const int16_t* pcm /* packed: row b = sample_rates[b] / 50 samples, rows back to back */,
                                  const int32_t* sample_rates, const int32_t* num_bits, const int32_t* dtx /* or NULL */);
int lyra_hip_encode_streams_end(lyra_hip_ctx* ctx, uint8_t* packets /* [B][23] */, int32_t* packet_bytes /* [B], required */);

#ifdef __cplusplus
}
#endif
#endif  /* LYRA_HIP_ENCODE_STREAMS_H_ */
