/* lyra_hip_shared_bridge.h -- the conference bridge with loudest-N selection and SHARED ENCODERS: every distinct mix of a room
 * is encoded once, and the packet goes to everyone who hears that mix.
 *
 * With max_speakers = N a room has at most 1 + N distinct mixes per tick: the common mix that every non-speaker hears, and one
 * mix-minus per speaker.  The loudest-N tick (lyra_hip_speakers.h) still runs one encoder chain per participant; this tick
 * runs E = n_rooms * (1 + N) of them, whatever the size of the rooms, and fans the E packets out.  What that needs and the
 * stateless selection does not is a stable assignment of speakers to encoders -- a talker who remains a speaker stays on the
 * same encoder stream while the loudness ranks around them change -- kept in a slot table, the only state the feature adds.
 * Bitrate and DTX are therefore settings of an ENCODER ROW (a room and a slot), not of a listener.
 *
 * The mix.  For one tick of B participant rows, x_b, level_b, source_b, the candidates and the speakers of room r are those of
 * lyra_hip_speakers.h, word for word (the same two kernels compute them); the speaker list of a room is in selection order,
 * loudest first.  S_r[k] is the int32 sum of the speakers' x[k]; the clamp is to [-32768, 32767].
 *
 * Slot table.  d_slots[n_table_rooms][LYRA_HIP_SHARED_SLOTS] int32, read and written: participant STREAM IDS (the values of
 * d_stream_ids, not row numbers, so the caller may reorder its batch between ticks) or -1 for a free slot.  Room r of the tick
 * uses table row d_room_keys[r]; a NULL d_room_keys means key r.  In the `_dev` form the table is the caller's, cleared with a
 * memset to 0xFF.  Update rule for room r with key q:
 *   1. for j = 0 .. N - 1 ascending: slot j is kept if d_slots[q][j] is the stream id of one of this tick's speakers of room r
 *      and no lower slot already holds that id; otherwise it becomes free;
 *   2. the speakers that hold no slot, in selection order, take the free slots in ascending j;
 *   3. slots j >= N are set to -1.
 * slot_of[b] is j for the speaker in slot j and -1 for everyone else, rows in no room included.
 *
 * Encoder rows.  Row e = r * (1 + N) hears clamp(S_r); row e = r * (1 + N) + 1 + j hears clamp(S_r - x_s), s being the
 * speaker in slot j; a free slot hears clamp(S_r) -- its encoder stays on the room's audio, so that a new speaker's encoder
 * starts from the history the room's listeners have been hearing.
 *
 * Fan-out.  Participant b of room r receives all 23 bytes and the size of encoder row r * (1 + N) + 1 + slot_of[b] if it is a
 * speaker, those of row r * (1 + N) otherwise; a row in no room gets 23 zero bytes and size 0.  An empty (DTX) encoder packet
 * fans out as size 0.
 *
 * The index is not trusted, as in both other bridges: d_order entries are range-checked, bad ones skipped and counted once per
 * call in the bridge's error word (lyra_hip_bridge_errors); d_room_start values are clamped; a d_room_keys value outside
 * [0, n_table_rooms) is counted once, the room's table row is left alone, its encoder rows hear zeros and its members get
 * empty packets (23 zero bytes, size 0) and slot_of -1.  Every row number and slot that went through memory is checked again
 * before it addresses anything.  Duplicate keys, rows named twice or two rows with one stream id give unspecified audio, slots
 * and packets; even then nothing is written outside the buffers of the call.
 *
 * lyra_hip_shared_mix_dev
 *   Levels, selection, slot update and the E mixes: a helper on the encode-side stream, stateless apart from the caller's
 *   table; it completes on lyra_hip_stream().  d_enc_mix [E][320] with E = n_rooms * (1 + max_speakers).  d_room_keys, d_muted,
 *   d_is_comfort_noise (applied where given), d_levels, d_is_speaker and d_slot_of may be NULL.  d_pcm16 and d_enc_mix must be
 *   16-byte aligned and distinct.  A null required pointer, B out of range, n_rooms or n_members outside [0, B],
 *   n_table_rooms < 1, a misaligned buffer or max_speakers outside [1, 8]: LYRA_HIP_EINVAL, nothing enqueued.
 *
 * lyra_hip_shared_tick_dev
 *   One tick.  The contract is a composition, bit for bit, outputs and every byte of per-stream state:
 *     decode leg  lyra_hip_decode_lossy_mixed_dev(sample_rate_hz = 16000) on d_packets / d_packet_bytes (0 / 8 / 15 / 23),
 *     the mix     as above over that hop and the flags of this tick, updating d_slots,
 *     encode leg  ONE lyra_hip_encode_streams_dev call on E rows: ids d_enc_stream_ids[E], every rate 16000, row e at sample
 *                 offset 320 * e of the encoder mixes, d_enc_num_bits[E], d_enc_dtx[E] or NULL,
 *     fan-out     as above into d_out_packets / d_out_packet_bytes.
 *   Only the encoder side of d_enc_stream_ids is used, so they may coincide with participants' ids (whose decoder side the
 *   decode leg uses).  E > max_streams: LYRA_HIP_EINVAL -- such a tick (rooms smaller than 1 + N throughout) belongs on the
 *   loudest-N call.  With n_rooms == 0 there is no encode leg: every row gets an empty packet.
 *   Optional outputs (NULL: library scratch, allocated on first use before anything is enqueued, alternated by call parity):
 *   d_pcm16, d_enc_mix (16-byte aligned where given), d_enc_packets [E][23], d_enc_packet_bytes [E], d_is_noise,
 *   d_is_comfort_noise, d_levels, d_is_speaker, d_slot_of.  The bytes of d_enc_packets behind a packet's size are what the
 *   caller left there (zeros in the library's scratch), as with lyra_hip_encode_streams_dev; they fan out with the packet.
 *   Ordering: as the loudest-N tick -- one decode-side call followed by one encode-side call; the encode-side stream waits for
 *   an event recorded on the noise stream behind the lossy mix.  The fan-out runs on the quantizer stream behind the
 *   quantizer: outgoing packets (and the encoder packets) complete on the quantizer stream, d_pcm16 and the noise flags on the
 *   noise stream, d_enc_mix, d_slots, d_levels, d_is_speaker and d_slot_of on the encode-side stream (with n_rooms == 0 the
 *   outgoing packets too); lyra_hip_stream_wait and lyra_hip_synchronize cover all three, and so does every later call of the
 *   library.  LYRA_HIP_SUBBATCHES > 1 accepted (not split); lyra_hip_set_serial supported.
 *   Refusals as the loudest-N tick's, and the above: LYRA_HIP_EINVAL, nothing enqueued.
 *
 * lyra_hip_shared_begin / _end
 *   The two-deep host-buffer form: one validation, one upload, one download per tick; slot_of, the levels and the speaker
 *   flags ride in the download.  rooms[B] as in lyra_hip_bridge_begin.  room_labels[n_rooms]: strictly ascending and exactly
 *   the set of labels >= 0 present in rooms, each below max_streams.  enc_ids, enc_bits, enc_dtx: [n_rooms][1 + max_speakers],
 *   room i of room_labels first its common row, then its slots; enc_dtx may be NULL.  The slot table is the context's: one row
 *   per label, allocated on first use, initially all -1, key = label.  begin() validates on the host: participant ids, encoder
 *   ids (range, duplicates among themselves), packet sizes, bit counts, room sizes, max_speakers in [1, 8], the labels,
 *   E <= max_streams; a refusal is LYRA_HIP_EINVAL, enqueues nothing and changes nothing.
 *   It shares the two slots and in-flight counters of lyra_hip_bridge_begin and lyra_hip_speakers_begin: at most two ticks of
 *   any kind are in flight together, every other pipelined host-buffer form excludes it (in both directions), an end() of
 *   another kind on the oldest tick is refused and consumes nothing, lyra_hip_export_streams / lyra_hip_import_streams refuse
 *   while a tick is outstanding and lyra_hip_reset_streams drains the context first (it leaves the slot table alone).
 *
 * lyra_hip_shared_reset_rooms
 *   Drains the context and sets the table rows of the given labels back to -1 (labels that have no row yet are skipped; a label
 *   outside [0, max_streams) is LYRA_HIP_EINVAL and nothing changes).  The encoder streams of those rooms are the caller's to
 *   reset (lyra_hip_reset_streams). */
#ifndef LYRA_HIP_SHARED_BRIDGE_H_
#define LYRA_HIP_SHARED_BRIDGE_H_

#include "lyra_hip_speakers.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LYRA_HIP_SHARED_SLOTS 8   /* width of a row of the slot table: LYRA_HIP_SPEAKERS_MAX */

typedef struct lyra_hip_shared_tick {
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
  uint8_t* d_out_packets;            /* [B][23] */
  int32_t* d_out_packet_bytes;       /* [B] */
  int16_t* d_pcm16;                  /* [B][320], or NULL: what every participant said */
  int32_t* d_is_noise;               /* [B], or NULL */
  int32_t* d_is_comfort_noise;       /* [B], or NULL */
  int max_speakers;                  /* N: 1 .. LYRA_HIP_SPEAKERS_MAX */
  int64_t* d_levels;                 /* [B], or NULL */
  int32_t* d_is_speaker;             /* [B], or NULL */
  const int32_t* d_room_keys;        /* [n_rooms] table row of every room, or NULL: room r uses row r */
  int32_t* d_slots;                  /* [n_table_rooms][8] stream ids, -1: free; in and out */
  int n_table_rooms;
  const int32_t* d_enc_stream_ids;   /* [E], E = n_rooms * (1 + N): the encoder streams */
  const int32_t* d_enc_num_bits;     /* [E] */
  const int32_t* d_enc_dtx;          /* [E], or NULL: no encoder row uses DTX */
  int16_t* d_enc_mix;                /* [E][320], or NULL: what every encoder row hears */
  uint8_t* d_enc_packets;            /* [E][23], or NULL */
  int32_t* d_enc_packet_bytes;       /* [E], or NULL */
  int32_t* d_slot_of;                /* [B], or NULL: the slot of a speaker, -1 for everyone else */
} lyra_hip_shared_tick;

int lyra_hip_shared_mix_dev(lyra_hip_ctx* ctx, const int16_t* d_pcm16 /* [B][320] */, const int32_t* d_stream_ids /* [B] */,
                            int B, const int32_t* d_order, const int32_t* d_room_start, int n_rooms, int n_members,
                            const int32_t* d_muted /* or NULL */, const int32_t* d_is_comfort_noise /* or NULL */,
                            int max_speakers, const int32_t* d_room_keys /* [n_rooms], or NULL */, int32_t* d_slots,
                            int n_table_rooms, int16_t* d_enc_mix /* [E][320] */, int64_t* d_levels /* [B], or NULL */,
                            int32_t* d_is_speaker /* [B], or NULL */, int32_t* d_slot_of /* [B], or NULL */);
int lyra_hip_shared_tick_dev(lyra_hip_ctx* ctx, const lyra_hip_shared_tick* tick);
int lyra_hip_shared_begin(lyra_hip_ctx* ctx, const int32_t* stream_ids, int B, const uint8_t* packets /* [B][23] */,
                          const int32_t* packet_bytes /* [B] */, const int32_t* rooms /* [B] */,
                          const int32_t* muted /* [B], or NULL */, unsigned flags, int max_speakers,
                          const int32_t* room_labels /* [n_rooms] */, int n_rooms,
                          const int32_t* enc_ids /* [n_rooms][1 + N] */, const int32_t* enc_bits /* [n_rooms][1 + N] */,
                          const int32_t* enc_dtx /* [n_rooms][1 + N], or NULL */);
int lyra_hip_shared_end(lyra_hip_ctx* ctx, uint8_t* out_packets /* [B][23] */, int32_t* out_packet_bytes /* [B] */,
                        int32_t* is_noise /* [B], or NULL */, int32_t* is_comfort_noise /* [B], or NULL */,
                        int64_t* levels /* [B], or NULL */, int32_t* is_speaker /* [B], or NULL */,
                        int32_t* slot_of /* [B], or NULL */);
int lyra_hip_shared_reset_rooms(lyra_hip_ctx* ctx, const int32_t* room_labels, int n);

#ifdef __cplusplus
}
#endif
#endif  /* LYRA_HIP_SHARED_BRIDGE_H_ */
