/* lyra_hip_spans_meeting.h -- a recorded MEETING WITH A SCHEDULE through the conference bridge, time-parallel: participants
 * who join late, leave early, drop and come back, and move between rooms, decoded, mixed and encoded in one call.
 *
 * The recording call of the span family (the header beside this one, "a meeting recording through the bridge") assumes that
 * every participant is present for the same T ticks and stays in one room, and tells the caller to cut a meeting at every
 * change.  Nothing in the codec forces the cut: both legs take spans of different lengths, a stream's state advances only on
 * the ticks on which it is a row, and the pass between the legs keeps no state from tick to tick.  So a meeting with any
 * schedule is ONE decode leg over each participant's present ticks, ONE pass that knows who is where on every tick, and ONE
 * encode leg.  This header adds the schedule, the pass driven by it, and the call around both.
 *
 * Names.  The calls are lyra_hip_spans_meeting_*.  This header includes lyra_hip_speakers.h (whose
 * LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE is the flag bit used here; LYRA_HIP_SPEAKERS_MAX bounds max_speakers) and
 * lyra_hip_spans_mixed.h (lyra_hip_span), and none of the other conference headers.
 *
 * Data model.  A call covers P participants.
 *   spans[p]     participant p: its stream id and its frames in the frame-major buffers of the span calls.  n_frames is the
 *                number of ticks on which p is PRESENT; it may differ per participant and may be 0.  Ids distinct and
 *                non-negative, first_frame >= 0, the ranges of participants with frames disjoint; at most 2^30 - 1 span frames
 *                in all.
 *   stays        a HOST array [n_stays] of lyra_hip_meeting_stay, sorted by (participant, first_tick): participant p is
 *                present, in `room`, on meeting ticks first_tick .. first_tick + n_ticks - 1.  room is a label as in the tick
 *                calls' planner; < 0: present but in no room (hears zeros, heard by nobody).  n_ticks >= 1, first_tick >= 0
 *                (and at most 2^40), participant in 0 .. P-1; stays of one participant do not overlap (they may touch: a room
 *                move is two stays back to back); their n_ticks sum to spans[p].n_frames.  A participant with no stay has
 *                n_frames == 0 and is ignored by both legs and the pass.  Anything else is LYRA_HIP_EINVAL.
 *   meaning      Participant p's k-th present tick is buffer frame spans[p].first_frame + k: present ticks are contiguous in
 *                the buffers, whatever gaps the meeting timeline has.  On a tick covered by no stay the participant is
 *                ABSENT: it is no row of that tick -- not decoded, not encoded, not heard; its state does not advance and
 *                nothing is written for it.  The meeting length is T = max(first_tick + n_ticks), 0 without stays.
 *   epochs       An epoch is a maximal run of ticks between two consecutive values of {first_tick, first_tick + n_ticks} over
 *                all stays: membership is constant inside it.  (Ticks in front of the earliest first_tick belong to no epoch;
 *                an epoch in which nobody is present has no entries.)  Within an epoch rooms come in ascending label order
 *                and participants in ascending participant number inside a room: the row order of the tick call with the
 *                present participants as rows, so the loudest-N "ties to the earlier row" rule carries over.
 *   per frame    d_packets [frames][23] on the device; packet_bytes HOST [frames], 0 / 8 / 15 / 23; num_bits HOST [frames];
 *                d_muted on the device, [frames] or NULL; every output: frame-indexed exactly as in the recording call.
 *   per part.    dtx HOST [P] or NULL.
 *   flags        LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE.   max_speakers  0: the full mix; 1 .. 8: the loudest-N selection.
 *   Frames outside every span are untouched in every buffer; the mix frames of a present participant in no room are written
 *   as zeros by the pass itself.
 *
 * LYRA_HIP_MEETING_MAX_ENTRIES.  An entry is one participant present in one epoch.  A schedule of more entries is refused
 * (LYRA_HIP_EINVAL): the caller cuts such a meeting into two calls -- spans continue live streams, so the cut is exact.  At
 * the bound the index of a call is 2^22 * 12 bytes of entries (an int64 frame base and an int32 room each, 48 MB) plus at most
 * 2^22 * 8 bytes of room offsets (32 MB) plus 80 bytes per epoch piece, once in pinned host memory and once on the device,
 * grow-only; a meeting of 32 participants and an event every 25 ticks over 9,000 ticks takes about 150 KB.
 *
 * lyra_hip_spans_meeting_plan (no context, no GPU)
 *   Runs every check above, plus: a room of more than 32767 members (the tick calls' bound on a room) in any epoch is
 *   LYRA_HIP_EINVAL.  Returns n_epochs, n_entries and n_ticks (all three required), and where the caller passes buffers (each
 *   may be NULL): epoch_tick [n_epochs + 1] (the epochs' first ticks and the meeting's end), epoch_entry [n_epochs + 1]
 *   (offsets into the entry arrays), entry_participant [n_entries] and entry_room [n_entries]: the dense room number inside
 *   the epoch, 0 .. rooms of the epoch - 1 in ascending label order.  The entries of rooms come first and are
 *   room-contiguous, participants ascending; they are followed by the epoch's present participants in no room, ascending,
 *   marked -1.  A caller sizes the arrays with a first call that passes none.  P >= 1; stays may be NULL when n_stays == 0.
 *
 * lyra_hip_spans_meeting_mix_dev
 *   The pass alone, stateless, on the encode-side stream; it completes on lyra_hip_stream().  d_muted, d_is_comfort_noise
 *   (applied where given), d_levels and d_is_speaker may be NULL.  Per present (participant, tick) it is bit for bit
 *   lyra_hip_bridge_mix_dev (max_speakers == 0) or lyra_hip_speakers_mix_dev (1 .. 8) on that tick's present rows, in
 *   ascending participant number.  The pass is table-driven: the host uploads one row per epoch piece and one launch per
 *   stage covers every (epoch, unit, tick) of a slab of epochs -- a churny meeting of thousands of short epochs costs the
 *   launches of a constant one.  Every launch covers at most 2^25 wavefronts; the selection scratch of a slab (levels,
 *   speaker lists, parked keys of rooms above 64) is grow-only and stays under 256 MB whatever the schedule; an epoch too long
 *   for a slab is split into pieces.
 *
 * lyra_hip_spans_meeting_dev
 *   The whole bridge.  The contract is a composition: per span frame and per span stream, outgoing packets and sizes, pcm16,
 *   mix, is_noise, is_comfort_noise, levels and speaker flags are BIT FOR BIT what lyra_hip_bridge_tick_dev (max_speakers
 *   == 0) or lyra_hip_speakers_tick_dev (1 .. 8) give over ticks 0 .. T-1 in order, where the rows of tick t are the
 *   participants present on t in ascending participant number, with that tick's packets, sizes, bit counts, mutes and the
 *   index of those rows' rooms; a tick with nobody present is no call.  Afterwards lyra_hip_export_streams returns the same
 *   bytes, for participants and lanes.  Everything else is the recording call's: a call continues live streams, mid-burst
 *   included, and tick calls or further calls may follow; the decode leg (lyra_hip_decode_spans_lossy_mixed_dev at 16 kHz)
 *   blocks the host once at its start, the encode leg (lyra_hip_encode_spans_mixed_dev at 16000 straight from d_mix) runs as
 *   the DTX participants' pass and then the others', and a DTX pass blocks the host once more; where any dtx[p] != 0 (of a
 *   participant with frames) the context's encoder rate must be 16000; d_pcm16, d_is_noise and d_is_comfort_noise complete
 *   on lyra_hip_stream_decode(), everything else on lyra_hip_stream(); the ordering rules count one decode-side call and two
 *   or three encode-side calls; the library uses scratch of its own for the comfort-noise flags when d_is_comfort_noise is
 *   NULL and SKIP_COMFORT_NOISE is set; lyra_hip_set_serial is supported and LYRA_HIP_SUBBATCHES > 1 accepted (not split);
 *   bytes past a packet's size and the rows of empty DTX packets are not written.  A call in which no participant has a
 *   frame is accepted and enqueues nothing.
 *   Refusals, each LYRA_HIP_EINVAL with nothing enqueued and no state or error counter changed: everything the planner
 *   refuses; a null call or required pointer; P outside 1 .. max_streams; span or lane ids out of range, or a lane that is
 *   a participant with frames, or named twice; a packet size or bit count off the lists on a span frame; d_pcm16 / d_mix
 *   misaligned or equal; d_levels not 8-byte aligned; unknown flags; max_speakers outside 0 .. 8; DTX with an encoder rate
 *   other than 16000.  All scratch is allocated before the decode leg is enqueued.
 *
 * lyra_hip_spans_meeting
 *   The host-buffer form: stages frames 0 .. the last span's end, runs lyra_hip_spans_meeting_dev, synchronises and writes
 *   the spans' frames of the outputs only; the caller's arrays outside the spans are untouched.  out_packets rows read back
 *   zero behind each packet's bytes.  pcm16, mix, is_noise, is_comfort_noise, levels and is_speaker may be NULL.
 *
 * Measured on an MI355X (tools/bridge_bench.py --recording --churn TICKS, profiles/bridge.jsonl): 3 minutes of 32
 * participants in 4 rooms on 4,096 lanes, median of 5 (min..max).  One event in 150 ticks: one call 73.0 ms (71.0..74.0), the 61
 * recording calls cut at the events 0.628 s (0.612..0.666), the ticks with the present rows 4.65 s (4.56..4.76).  One event in 25
 * ticks: 70.8 ms (69.1..73.1), 1.816 s (1.780..1.931) in 361 calls, 5.61 s (5.58..5.63).  The pass alone: 0.15 and 0.45 ms.
 *
 * Out of scope: shared encoders, request sizes other than one hop, external sample rates, pipelined begin / end forms. */
#ifndef LYRA_HIP_SPANS_MEETING_H_
#define LYRA_HIP_SPANS_MEETING_H_

#include "lyra_hip_speakers.h"
#include "lyra_hip_spans_mixed.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LYRA_HIP_MEETING_MAX_ENTRIES (1 << 22)

typedef struct lyra_hip_meeting_stay {
  int32_t participant;   /* index into spans */
  int32_t room;          /* label; < 0: present, in no room (hears zeros, heard by nobody) */
  int64_t first_tick;    /* meeting tick */
  int64_t n_ticks;       /* >= 1 */
} lyra_hip_meeting_stay;

typedef struct lyra_hip_spans_meeting_call {
  const lyra_hip_span* spans;        /* HOST [P]: participant p, n_frames = its present ticks */
  int P;
  const int32_t* lane_ids;           /* HOST [n_lanes]: streams lent to both legs */
  int n_lanes;
  const lyra_hip_meeting_stay* stays;   /* HOST [n_stays], sorted by (participant, first_tick) */
  int n_stays;
  const uint8_t* d_packets;          /* [frames][23] incoming */
  const int32_t* packet_bytes;       /* HOST [frames] 0 / 8 / 15 / 23 */
  const int32_t* d_muted;            /* [frames], or NULL */
  unsigned flags;                    /* LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE */
  const int32_t* num_bits;           /* HOST [frames] outgoing bit counts */
  const int32_t* dtx;                /* HOST [P], or NULL: no outgoing stream uses DTX */
  uint8_t* d_out_packets;            /* [frames][23] */
  int32_t* d_out_packet_bytes;       /* [frames] */
  int16_t* d_pcm16;                  /* [frames][320] workspace: what every participant said */
  int16_t* d_mix;                    /* [frames][320] workspace: what every participant heard */
  int32_t* d_is_noise;               /* [frames], or NULL */
  int32_t* d_is_comfort_noise;       /* [frames], or NULL */
  int max_speakers;                  /* 0: full mix; 1 .. LYRA_HIP_SPEAKERS_MAX */
  int64_t* d_levels;                 /* [frames], or NULL (max_speakers >= 1 only) */
  int32_t* d_is_speaker;             /* [frames], or NULL (max_speakers >= 1 only) */
} lyra_hip_spans_meeting_call;

int lyra_hip_spans_meeting_plan(const lyra_hip_span* spans, int P, const lyra_hip_meeting_stay* stays, int n_stays,
                                int64_t* n_epochs, int64_t* n_entries, int64_t* n_ticks,
                                int64_t* epoch_tick /* [n_epochs + 1], or NULL */, int64_t* epoch_entry /* [n_epochs + 1], or NULL */,
                                int32_t* entry_participant /* [n_entries], or NULL */, int32_t* entry_room /* [n_entries], or NULL */);
int lyra_hip_spans_meeting_mix_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int P, const lyra_hip_meeting_stay* stays,
                                   int n_stays, const int16_t* d_pcm16 /* [frames][320] */,
                                   const int32_t* d_muted /* [frames], or NULL */,
                                   const int32_t* d_is_comfort_noise /* [frames], or NULL */, int max_speakers,
                                   int16_t* d_mix /* [frames][320] */, int64_t* d_levels /* [frames], or NULL */,
                                   int32_t* d_is_speaker /* [frames], or NULL */);
int lyra_hip_spans_meeting_dev(lyra_hip_ctx* ctx, const lyra_hip_spans_meeting_call* call);
int lyra_hip_spans_meeting(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int P, const int32_t* lane_ids, int n_lanes,
                           const lyra_hip_meeting_stay* stays, int n_stays, const uint8_t* packets /* [frames][23] */,
                           const int32_t* packet_bytes, const int32_t* muted /* [frames], or NULL */, unsigned flags,
                           const int32_t* num_bits, const int32_t* dtx /* [P], or NULL */, int max_speakers,
                           uint8_t* out_packets /* [frames][23] */, int32_t* out_packet_bytes /* [frames] */,
                           int16_t* pcm16 /* [frames][320], or NULL */, int16_t* mix /* [frames][320], or NULL */,
                           int32_t* is_noise, int32_t* is_comfort_noise, int64_t* levels, int32_t* is_speaker);

#ifdef __cplusplus
}
#endif
#endif  /* LYRA_HIP_SPANS_MEETING_H_ */
