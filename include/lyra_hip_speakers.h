/* lyra_hip_speakers.h -- the conference bridge with loudest-N selection: every participant hears the few loudest talkers of
 * its room, and the server learns who is speaking.
 *
 * What production media servers do in place of a full mix: the sum of 15 open microphones is mostly noise, and a mix of many
 * talkers is never judged noise by the outgoing DTX.  The calls below are those of the full-mix bridge header with one more
 * argument, max_speakers, and two more outputs, the levels and the speaker flags; "no selection" is the full-mix bridge.
 * The selection is exact, integer only and stateless: no smoothing or hysteresis across ticks, no per-stream state.
 *
 * The mix.  For one tick of B rows, x_b[320] is row b of the 16 kHz hop; d_order / d_room_start are the inverted membership
 * index of the full-mix bridge (row numbers with a room's rows contiguous; the room boundaries), built by its planner.
 *   level_b   = sum over k of x_b[k]^2, exact (at most 320 * 2^30 < 2^39), written as int64 for EVERY row of the batch;
 *   source_b  = false if d_muted[b] != 0; false if LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE is set and the row's
 *               is_comfort_noise after this tick is non-zero; true otherwise;
 *   candidate = a member whose d_order entry is valid, with source_b and level_b > 0;
 *   speakers  = the max_speakers candidates of a room with the largest level; among equal levels the one at the earlier
 *               position in d_order wins;
 *   S_r[k]    = int32 sum of the speakers' x[k];  y_b[k] = clamp(S_r[k] - (speaker_b ? x_b[k] : 0), -32768, 32767) for a
 *               member b of room r.  A row that no room names hears zeros.
 *   is_speaker[b] = 1 for speakers, 0 for everyone else, rows in no room included.
 * Where every room has at most max_speakers candidates the mix is bit for bit the full mix (a zero-level row adds zero).
 * max_speakers lies in [1, LYRA_HIP_SPEAKERS_MAX]; anything else is LYRA_HIP_EINVAL with nothing enqueued.
 * The index is not trusted, exactly as in the full-mix bridge: a d_order entry outside [0, B) is skipped and counted in that
 * bridge's error word (its errors call reads it), once per call; d_room_start values are clamped to [0, n_members]; a row
 * named twice or a room above the planner's bound gives unspecified audio, levels and flags; in every case nothing is written
 * outside the mix, level and flag buffers.
 *
 * lyra_hip_speakers_mix_dev
 *   The selection mix alone, a stateless helper on the encode-side stream; it completes on lyra_hip_stream().  d_muted,
 *   d_is_comfort_noise (applied where given), d_levels and d_is_speaker may be NULL.  d_pcm16 and d_mix must be 16-byte aligned
 *   and distinct.  A null required pointer, B out of range, n_rooms or n_members outside [0, B], a misaligned buffer or
 *   max_speakers outside [1, 8]: LYRA_HIP_EINVAL, nothing enqueued.
 *
 * lyra_hip_speakers_tick_dev
 *   One tick.  The contract is a composition, bit for bit, outputs and every byte of per-stream state:
 *     decode leg  lyra_hip_decode_lossy_mixed_dev(sample_rate_hz = 16000) on d_packets / d_packet_bytes (0 / 8 / 15 / 23),
 *     the mix     as above over that hop and the flags of this tick,
 *     encode leg  lyra_hip_encode_streams_dev with every rate 16000 and row b at offset 320 * b of the mix, d_num_bits, d_dtx.
 *   Optional outputs (NULL: library scratch, allocated on first use before anything is enqueued, alternated by call parity):
 *   d_pcm16, d_mix (16-byte aligned where given), d_is_noise, d_is_comfort_noise, d_levels, d_is_speaker.
 *   Ordering: as the full-mix tick -- one decode-side call followed by one encode-side call; the encode-side stream waits for
 *   an event recorded on the noise stream behind the lossy mix.  Outgoing packets complete on the quantizer stream, d_pcm16 and
 *   the noise flags on the noise stream, d_mix, d_levels and d_is_speaker on the encode-side stream; lyra_hip_stream_wait and
 *   lyra_hip_synchronize cover all three.  LYRA_HIP_SUBBATCHES > 1 accepted (not split); lyra_hip_set_serial supported.
 *   Refusals as the full-mix tick's, and max_speakers outside [1, 8]: LYRA_HIP_EINVAL, nothing enqueued.
 *
 * lyra_hip_speakers_begin / _end
 *   The two-deep host-buffer form: the validation, the one upload and the one download of the full-mix form, with
 *   max_speakers checked on the host; levels and speaker flags ride in the one download (levels / is_speaker [B] or NULL).
 *   It shares the full-mix form's two slots: at most two ticks of either kind are in flight together, every other pipelined
 *   host-buffer form excludes it (in both directions), an end() of the other kind on the oldest tick is refused and consumes
 *   nothing, lyra_hip_export_streams / lyra_hip_import_streams refuse while a tick is outstanding and lyra_hip_reset_streams
 *   drains the context first. */
#ifndef LYRA_HIP_SPEAKERS_H_
#define LYRA_HIP_SPEAKERS_H_

#include "lyra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LYRA_HIP_SPEAKERS_MAX 8
#define LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE 1u   /* flags: a row that plays comfort noise after this tick is no source */

typedef struct lyra_hip_speakers_tick {
  const int32_t* d_stream_ids;       /* [B] */
  int B;
  const uint8_t* d_packets;          /* [B][23] incoming */
  const int32_t* d_packet_bytes;     /* [B] 0 / 8 / 15 / 23 */
  const int32_t* d_order;            /* [n_members] row numbers, a room's rows contiguous */
  const int32_t* d_room_start;       /* [n_rooms + 1] */
  int n_rooms;
  int n_members;
  const int32_t* d_muted;            /* [B], or NULL */
  unsigned flags;                    /* LYRA_HIP_SPEAKERS_* */
  const int32_t* d_num_bits;         /* [B] outgoing bit counts */
  const int32_t* d_dtx;              /* [B], or NULL: no outgoing stream uses DTX */
  uint8_t* d_out_packets;            /* [B][23] */
  int32_t* d_out_packet_bytes;       /* [B] */
  int16_t* d_pcm16;                  /* [B][320], or NULL: what every participant said */
  int16_t* d_mix;                    /* [B][320], or NULL: what every participant hears */
  int32_t* d_is_noise;               /* [B], or NULL */
  int32_t* d_is_comfort_noise;       /* [B], or NULL */
  int max_speakers;                  /* 1 .. LYRA_HIP_SPEAKERS_MAX */
  int64_t* d_levels;                 /* [B], or NULL: sum of squares of every row's hop */
  int32_t* d_is_speaker;             /* [B], or NULL: 1 where the row is among its room's speakers */
} lyra_hip_speakers_tick;

int lyra_hip_speakers_mix_dev(lyra_hip_ctx* ctx, const int16_t* d_pcm16 /* [B][320] */, int B, const int32_t* d_order,
                              const int32_t* d_room_start, int n_rooms, int n_members, const int32_t* d_muted /* or NULL */,
                              const int32_t* d_is_comfort_noise /* or NULL */, int max_speakers, int16_t* d_mix /* [B][320] */,
                              int64_t* d_levels /* [B], or NULL */, int32_t* d_is_speaker /* [B], or NULL */);
int lyra_hip_speakers_tick_dev(lyra_hip_ctx* ctx, const lyra_hip_speakers_tick* tick);
int lyra_hip_speakers_begin(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const uint8_t* packets /* [B][23] */,
                            const int32_t* packet_bytes /* [B] */, const int32_t* rooms /* [B] */,
                            const int32_t* muted /* [B], or NULL */, unsigned flags, const int32_t* num_bits /* [B] */,
                            const int32_t* dtx /* [B], or NULL */, int max_speakers);
int lyra_hip_speakers_end(lyra_hip_ctx* ctx, uint8_t* out_packets /* [B][23] */, int32_t* out_packet_bytes /* [B] */,
                          int32_t* is_noise /* [B], or NULL */, int32_t* is_comfort_noise /* [B], or NULL */,
                          int64_t* levels /* [B], or NULL */, int32_t* is_speaker /* [B], or NULL */);

#ifdef __cplusplus
}
#endif
#endif  /* LYRA_HIP_SPEAKERS_H_ */
