/* lyra_hip_bridge.h -- a conference bridge on the device: decode, mix-minus, encode in one call.
 *
 * What a media server does between its decoders and its encoders: every participant of a call hears the sum of the others.
 * Both codec chains run at 16 kHz internally and packets carry no sample rate, so the bridge needs no resampler: one kernel
 * sits between the lossy decode's 16 kHz hop and the feature extractor's input.  Endpoints at other rates resample themselves.
 *
 * The mix.  For one tick of B rows, x_b[320] is row b of the 16 kHz hop.
 *   source_b = false if d_muted[b] != 0; false if LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE is set and the row's
 *              is_comfort_noise after this tick is non-zero; true otherwise.
 *   S_r[k]   = sum over the members j of room r with source_j of x_j[k], in int32;
 *   y_b[k]   = clamp(S_r[k] - (source_b ? x_b[k] : 0), -32768, 32767) for a member b of room r.
 *   A row that no room names hears zeros and is heard by nobody.  Integer arithmetic only: exact, order-free, no gain.
 * Membership is an inverted index in DEVICE memory: d_order[n_members] holds row numbers with a room's rows contiguous,
 * d_room_start[n_rooms + 1] holds the room boundaries.  lyra_hip_bridge_plan builds both from one room label per row.
 * The index is the caller's and the kernel does not trust it: a d_order entry outside [0, B) is skipped and counted
 * (lyra_hip_bridge_errors, as the other error counters: synchronises, optionally clears), d_room_start values are clamped to
 * [0, n_members], and a room that would end before it starts is empty.  A row named twice is a caller error: the audio of the
 * rooms that name it is unspecified, nothing outside the mix buffer is written.  Rooms of more than
 * LYRA_HIP_BRIDGE_MAX_ROOM members may overflow the int32 sum (32,767 * 32,768 < 2^31); the planner refuses them.
 *
 * lyra_hip_bridge_plan (no context, no GPU; like lyra_hip_spans_plan)
 *   rooms[b] >= 0: the label of row b's room; < 0: row b is in no room.  Rooms come in ascending label order, rows in
 *   ascending order inside a room.  order holds B entries, room_start B + 1.  Returns 0, or LYRA_HIP_EINVAL for a null
 *   pointer, B < 0 or a room of more than LYRA_HIP_BRIDGE_MAX_ROOM members (the outputs are unspecified then).
 *
 * lyra_hip_bridge_mix_dev
 *   The mix alone, a stateless helper on the encode-side stream as lyra_hip_resample_dev(side 0) is: d_mix is zeroed (one
 *   memset, so rows in no room read zeros) and then written by one kernel; it completes on lyra_hip_stream().  d_muted and
 *   d_is_comfort_noise may be NULL (nobody muted / no row skipped: a d_is_comfort_noise that is given is applied, there is no
 *   flag here).  d_pcm16 and d_mix must be 16-byte aligned and distinct.  A null required pointer, B out of range, n_rooms or
 *   n_members outside [0, B] or a misaligned buffer: LYRA_HIP_EINVAL, nothing enqueued.
 *
 * lyra_hip_bridge_tick_dev
 *   One tick of the bridge.  The contract is a composition, bit for bit, outputs and every byte of per-stream state:
 *     decode leg  lyra_hip_decode_lossy_mixed_dev(sample_rate_hz = 16000) on d_packets / d_packet_bytes (0 / 8 / 15 / 23),
 *     the mix     as above over that hop and the flags of this tick,
 *     encode leg  lyra_hip_encode_streams_dev with every rate 16000 and row b at offset 320 * b of the mix, d_num_bits, d_dtx.
 *   Invalid packet sizes and bit counts behave as in those two calls and are counted in their error words.  The bridge keeps
 *   no per-stream state of its own: a stream may move between this call and the calls it composes from tick to tick without
 *   a reset.  d_pcm16, d_mix, d_is_noise and d_is_comfort_noise are optional outputs (NULL: library scratch, allocated on first
 *   use, alternated by call parity); where given, d_pcm16 and d_mix must be 16-byte aligned.
 *   Ordering: for rules (1) to (3) of "Streams" (lyra_hip.h) the tick is one decode-side call followed by one encode-side
 *   call, and the encode leg reads THIS tick's mix: the encode-side stream waits for an event recorded on the noise stream
 *   behind the lossy mix (not behind the estimator that follows it).  Outgoing packets complete on the quantizer stream,
 *   d_pcm16 and the flags on the noise stream, d_mix on the encode-side stream; lyra_hip_stream_wait and
 *   lyra_hip_synchronize cover all three.  LYRA_HIP_SUBBATCHES > 1 accepted (not split); lyra_hip_set_serial supported.
 *   A null required pointer (d_stream_ids, d_packets, d_packet_bytes, d_num_bits, d_out_packets, d_out_packet_bytes, and
 *   d_order / d_room_start where n_members / n_rooms > 0), B out of range, n_rooms or n_members outside [0, B], a misaligned
 *   d_pcm16 / d_mix, unknown flag bits: LYRA_HIP_EINVAL, nothing enqueued.
 *
 * lyra_hip_bridge_begin / _end
 *   The two-deep host-buffer form.  begin() validates on the host -- stream ids (range, duplicates), packet sizes (0 / 8 / 15 /
 *   23), bit counts, room sizes through the planner -- and returns LYRA_HIP_EINVAL with nothing enqueued and nothing changed.
 *   It builds the index into pinned staging, does ONE upload on the decode-side stream and enqueues the tick; it does not
 *   synchronise and the caller's arrays are free on return.  rooms as in lyra_hip_bridge_plan; muted and dtx [B] or NULL.
 *   One download of outgoing packets, sizes and both flags is enqueued behind both legs; end() waits for the OLDEST tick only.
 *   out_packets [B][LYRA_HIP_MAX_PACKET_BYTES] (zero behind each packet's bytes) and out_packet_bytes [B] are required,
 *   is_noise / is_comfort_noise [B] or NULL.  Everything the tick allocates is allocated before anything is enqueued.  A third
 *   begin(), an end() with nothing in flight, and mixing with another pipelined host-buffer form -- lyra_hip_encode_begin,
 *   lyra_hip_decode_begin, lyra_hip_encode_streams_begin, lyra_hip_decode_streams_begin and the three
 *   lyra_hip_decode_samples*_begin -- while either kind has something in flight are refused, in both directions; begin() is
 *   refused as well while a lyra_hip_twin_* request is being assembled or fetched.  lyra_hip_export_streams / lyra_hip_import_streams refuse while a tick
 *   is outstanding; lyra_hip_reset_streams drains the context first. */
#ifndef LYRA_HIP_BRIDGE_H_
#define LYRA_HIP_BRIDGE_H_

#include "lyra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LYRA_HIP_BRIDGE_MAX_ROOM 32767
#define LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE 1u   /* flags: a row that plays comfort noise after this tick is no source */

typedef struct lyra_hip_bridge_tick {
  const int32_t* d_stream_ids;       /* [B] */
  int B;
  const uint8_t* d_packets;          /* [B][23] incoming */
  const int32_t* d_packet_bytes;     /* [B] 0 / 8 / 15 / 23 */
  const int32_t* d_order;            /* [n_members] row numbers, a room's rows contiguous */
  const int32_t* d_room_start;       /* [n_rooms + 1] */
  int n_rooms;
  int n_members;
  const int32_t* d_muted;            /* [B], or NULL */
  unsigned flags;                    /* LYRA_HIP_BRIDGE_* */
  const int32_t* d_num_bits;         /* [B] outgoing bit counts */
  const int32_t* d_dtx;              /* [B], or NULL: no outgoing stream uses DTX */
  uint8_t* d_out_packets;            /* [B][23] */
  int32_t* d_out_packet_bytes;       /* [B] */
  int16_t* d_pcm16;                  /* [B][320], or NULL: what every participant said */
  int16_t* d_mix;                    /* [B][320], or NULL: what every participant hears */
  int32_t* d_is_noise;               /* [B], or NULL */
  int32_t* d_is_comfort_noise;       /* [B], or NULL */
} lyra_hip_bridge_tick;

int lyra_hip_bridge_plan(const int32_t* rooms /* [B] */, int B, int32_t* order /* [B] */, int32_t* room_start /* [B + 1] */,
                         int* n_rooms, int* n_members);
int lyra_hip_bridge_mix_dev(lyra_hip_ctx* ctx, const int16_t* d_pcm16 /* [B][320] */, int B, const int32_t* d_order,
                            const int32_t* d_room_start, int n_rooms, int n_members, const int32_t* d_muted /* or NULL */,
                            const int32_t* d_is_comfort_noise /* or NULL */, int16_t* d_mix /* [B][320] */);
int lyra_hip_bridge_tick_dev(lyra_hip_ctx* ctx, const lyra_hip_bridge_tick* tick);
int lyra_hip_bridge_begin(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const uint8_t* packets /* [B][23] */,
                          const int32_t* packet_bytes /* [B] */, const int32_t* rooms /* [B] */,
                          const int32_t* muted /* [B], or NULL */, unsigned flags, const int32_t* num_bits /* [B] */,
                          const int32_t* dtx /* [B], or NULL */);
int lyra_hip_bridge_end(lyra_hip_ctx* ctx, uint8_t* out_packets /* [B][23] */, int32_t* out_packet_bytes /* [B] */,
                        int32_t* is_noise /* [B], or NULL */, int32_t* is_comfort_noise /* [B], or NULL */);
long lyra_hip_bridge_errors(lyra_hip_ctx* ctx, int clear);

#ifdef __cplusplus
}
#endif
#endif  /* LYRA_HIP_BRIDGE_H_ */
