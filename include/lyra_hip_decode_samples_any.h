/* lyra_hip_decode_samples_any.h -- LyraDecoder::DecodeSamples(n) on the device for ANY n of 0..4 hops.
 *
 * lyra_hip_decode_samples_dev (lyra_hip.h, "Packet loss on the device path") refuses a request of more than one hop and one
 * that is not a whole number of 16 kHz samples, because it has no BufferedResampler (buffered_resampler.cc:63-147): at 32 and
 * 48 kHz such a request leaves 1 or 2 resampled samples for the next call.  The calls below keep that leftover per stream and
 * run the reference loop for up to LYRA_HIP_DECODE_SAMPLES_MAX_HOPS hops inside one call, so the sizes audio back ends ask for
 * -- 128, 256, 441, 512, 1024 frames -- stay on the device path.
 *
 * lyra_hip_decode_samples_any_dev
 *   0 <= num_samples <= LYRA_HIP_DECODE_SAMPLES_MAX_HOPS * sample_rate_hz / 50 at 8000, 16000, 32000 or 48000 Hz; anything
 *   else is LYRA_HIP_EINVAL with nothing enqueued, as are a null d_stream_ids, d_packets or d_packet_bytes, a null d_pcm_ext
 *   with num_samples > 0 and B out of range.  The size is the same for every row of a call and free to change from call to call.
 *   Packets: the conventions of lyra_hip_decode_samples_dev -- d_packet_bytes[b] 0 (no packet) / 8 / 15 / 23, at most one
 *   packet per stream and call, the bounded FIFO of LYRA_HIP_DECODE_SAMPLES_FIFO vectors, errors counted in
 *   lyra_hip_decode_samples_errors.  A caller with more packets for a stream makes num_samples == 0 calls.
 *   Meaning: row b is SetEncodedPacket (if it got a packet) + DecodeSamples(num_samples) of a LyraDecoder created at
 *   sample_rate_hz, BufferedResampler included.  With L the stream's leftover count: used = min(L, n) samples come from the
 *   leftover, n_int = n > L ? ceil((n - L) * 16000 / rate) : 0 internal samples run through the reference loop (equal to the
 *   reference's float expression for every n in range and L in 0..2), are resampled, the first n - used delivered and the
 *   rest kept.  The loop runs in rounds of at most one hop, at most 4 per call; the packet is delivered in the first.
 *   State: the leftover -- a count of 0..2 and up to two int16 -- lives in the stream's state, travels with
 *   lyra_hip_export_streams / lyra_hip_import_streams (blob size, version and fingerprint unchanged; a count above 2 is
 *   refused) and is emptied by lyra_hip_reset_streams.
 *   Compatibility: for a request that obeys the size rule of lyra_hip_decode_samples_dev on a stream whose leftover is empty
 *   the call is, bit for bit, that call: samples, flags and every byte of state.  A stream may move between the two calls
 *   while its leftover is empty.  lyra_hip_decode_samples_dev IGNORES a leftover that is not empty: calling it then is a caller
 *   error that is not detected.  A request of up to 4 hops equals the same samples asked for in any split into smaller
 *   requests with no packet in between, bit for bit.
 *   Streams and ordering: one decode-side call and one noise call under rules (1) to (3) of "Streams"; outputs complete on
 *   the noise stream; LYRA_HIP_SUBBATCHES > 1 accepted (not split); lyra_hip_set_serial supported.
 *
 * lyra_hip_decode_samples_any_begin / _end
 *   The two-deep host-buffer form, as lyra_hip_decode_samples_begin / _end: begin() copies ids, sizes and packets into pinned
 *   staging (the caller's arrays are free on return; it does not synchronise) and enqueues the call into a row buffer of its
 *   own; end() downloads the OLDEST begun request, [B][num_samples] int16, and waits for it only.  begin() checks stream ids
 *   (range, duplicates), null pointers and the request size on the host: LYRA_HIP_EINVAL, nothing enqueued.  Likewise a third
 *   begin(), an end() with nothing in flight, and a begin() while lyra_hip_decode_begin, lyra_hip_decode_streams_begin or
 *   lyra_hip_decode_samples_begin has a request in flight (those refuse in turn while a request of this pipeline is).
 *   lyra_hip_export_streams / lyra_hip_import_streams are refused while a request is outstanding. */
#ifndef LYRA_HIP_DECODE_SAMPLES_ANY_H_
#define LYRA_HIP_DECODE_SAMPLES_ANY_H_

#include "lyra_hip.h"

#define LYRA_HIP_DECODE_SAMPLES_MAX_HOPS 4

#ifdef __cplusplus
extern "C" {
#endif

int lyra_hip_decode_samples_any_dev(lyra_hip_ctx* ctx, const int32_t* d_stream_ids, int B, const uint8_t* d_packets /* [B][23] */,
                                    const int32_t* d_packet_bytes /* [B] */, int num_samples, int sample_rate_hz,
                                    int16_t* d_pcm_ext /* [B][num_samples] */, int32_t* d_is_noise /* [B], or NULL */,
                                    int32_t* d_is_comfort_noise /* [B], or NULL */);
int lyra_hip_decode_samples_any_begin(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const uint8_t* packets /* [B][23] */,
                                      const int32_t* packet_bytes /* [B] */, int num_samples, int sample_rate_hz);
int lyra_hip_decode_samples_any_end(lyra_hip_ctx* ctx, int16_t* pcm /* [B][num_samples] */);

#ifdef __cplusplus
}
#endif
#endif  /* LYRA_HIP_DECODE_SAMPLES_ANY_H_ */
