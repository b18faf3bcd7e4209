/* lyra_hip_bridge_spans.h -- a meeting RECORDING through the conference bridge, time-parallel: decode, mix and encode all ticks
 * of P participants in one call.
 *
 * The ticks of lyra_hip_bridge.h / lyra_hip_speakers.h are one serial chain each (decode leg, mix, encode leg), and a recorded
 * meeting is hundreds of thousands of them with a handful of rows.  Both legs have time-parallel forms already: the codec
 * state is convolution history only, and the span calls of lyra_hip_spans_mixed.h run a long recording on lent lanes, bit for
 * bit.  What sits between the legs keeps no state from tick to tick at all: the mix and the loudest-N selection are exact
 * integer functions of one tick's hop, mutes and comfort-noise flags.  So the mix of a recording is ONE pass over all ticks,
 * and this header composes the three: what a service needs to render what each participant heard, to re-mix an archive under
 * other mutes or bitrates, or to replay captured bridge traffic.
 *
 * Names.  The calls belong to the span family and are named like it, lyra_hip_spans_bridge_*: the tick calls' header is the only
 * one that declares names starting with lyra_hip_bridge (tests/test_bridge_cpu.py keeps it so).  This header includes
 * lyra_hip_speakers.h, whose LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE is the same bit as LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE.
 *
 * Data model.  A call covers P participants over the same T ticks.
 *   spans[p]     participant p: its stream id and its frames in the frame-major buffers of the span calls.  Tick t of
 *                participant p is buffer frame spans[p].first_frame + t.  Every span has the same n_frames (= T >= 0);
 *                anything else is LYRA_HIP_EINVAL.  Ids distinct, frame ranges non-negative and disjoint, as the span calls.
 *   rooms        a HOST array [P] of labels as in lyra_hip_bridge_plan (< 0: in no room).  Membership is constant within a
 *                call: a meeting whose membership changes is cut into consecutive calls at the change points.  Spans continue
 *                live streams (a later call's spans start where the earlier call's ended), so the cut is exact.
 *                The library builds the inverted index itself and checks it; no device-side index arrives from the caller.
 *   per frame    d_packets [frames][23] on the device; packet_bytes HOST [frames], 0 / 8 / 15 / 23, as
 *                lyra_hip_decode_spans_lossy_mixed_dev; num_bits HOST [frames], as lyra_hip_encode_spans_mixed_dev;
 *                d_muted on the device, [frames] or NULL: a mute that comes and goes is a property of the tick.
 *   per part.    dtx HOST [P] or NULL, as the tick's d_dtx.
 *   flags        LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE.   max_speakers  0: the full mix; 1 .. 8: the loudest-N selection.
 *   outputs      frame-indexed.  d_out_packets [frames][23], d_out_packet_bytes [frames], d_pcm16 [frames][320] (what was said)
 *                and d_mix [frames][320] (what was heard) are required; the last two are the caller's workspace as in the span
 *                calls, 16-byte aligned and distinct.  d_is_noise, d_is_comfort_noise [frames] are optional (the library uses
 *                scratch of its own for the latter when it is NULL and SKIP_COMFORT_NOISE is set); d_levels [frames] int64
 *                and d_is_speaker [frames] int32 are optional and written by the loudest-N selection only.
 *   Frames outside every span are untouched in every buffer; the mix frames of a participant in no room are written as zeros
 *   by the pass itself (there is no memset of d_mix).
 *
 * lyra_hip_spans_bridge_plan (no context, no GPU; like lyra_hip_bridge_plan)
 *   The checks above -- non-null pointers, P >= 1, equal n_frames, ids >= 0 and distinct, first_frame >= 0, disjoint ranges --
 *   plus those of lyra_hip_bridge_plan, and the index over participant numbers 0 .. P-1: order holds P entries, room_start
 *   P + 1.  T = 0 is accepted (an empty recording; the index is still built).  Returns 0 or LYRA_HIP_EINVAL.
 *
 * lyra_hip_spans_bridge_mix_dev
 *   The pass alone, stateless, on the encode-side stream; it completes on lyra_hip_stream().  d_muted, d_is_comfort_noise
 *   (applied where given: there is no flag here), d_levels and d_is_speaker may be NULL.  Per span frame it is bit for bit
 *   lyra_hip_bridge_mix_dev (max_speakers == 0) or lyra_hip_speakers_mix_dev (1 .. 8) on that tick's P rows.  With
 *   max_speakers >= 1 the pass runs over slabs of ticks, so that its selection scratch (speaker lists, levels, parked keys of
 *   rooms above 64) is grow-only and stays under 256 MB whatever T is.  Every launch, full mix included, covers at most 2^25
 *   (unit, tick) pairs -- 2^31 threads -- and a longer recording runs as more launches: no tick count wraps that arithmetic.
 *
 * lyra_hip_spans_bridge_dev
 *   The whole bridge.  The contract is a composition: per span frame and per span stream, outgoing packets and sizes, pcm16,
 *   mix, is_noise, is_comfort_noise, levels and speaker flags are BIT FOR BIT what P-row calls of lyra_hip_bridge_tick_dev
 *   (max_speakers == 0) or lyra_hip_speakers_tick_dev (1 .. 8) give over ticks 0 .. T-1 in order, with rows of ids in span
 *   order, that tick's packets, sizes, bit counts and mutes, and the index of `rooms`.  Bytes past a packet's size, and the row
 *   of a DTX noise frame (size 0), are not written.  Afterwards lyra_hip_export_streams returns the same bytes; a call
 *   continues live streams, mid-burst included; tick calls, or another of these calls with other rooms, may follow.  The same
 *   lanes lend decoder-side state to the decode leg and encoder-side state to the encode leg; they come back reset on both
 *   sides, and their other slots are untouched.
 *     decode leg  lyra_hip_decode_spans_lossy_mixed_dev at 16 kHz; it blocks the host once at its start, as its twin does.
 *     the pass    as lyra_hip_spans_bridge_mix_dev.
 *     encode leg  lyra_hip_encode_spans_mixed_dev at 16000 straight from d_mix (no copy).  It takes one DTX flag per call:
 *                 where dtx[] mixes both kinds the leg runs as two passes on the same lanes, the DTX participants' and then
 *                 the others'.  A DTX pass blocks the host once more.
 *   Encoder rate: the tick's encode leg gives every row the 16 kHz noise estimator whatever lyra_hip_set_encoder_sample_rate
 *   says; the span DTX encode uses the context's.  So where any dtx[p] != 0 the context's encoder rate must be 16000 (the
 *   default) -- anything else is LYRA_HIP_EINVAL; without DTX the rate is not read.
 *   Ordering: for rules (1) to (3) of "Streams" (lyra_hip.h) the call is one decode-side call followed by encode-side calls
 *   on the one encode-side stream, in order: the pass, then the encode leg's one or two passes (two or three in all; only
 *   decode-side calls count for the two-buffer rule, and there is one).  The encode-side stream waits for an event behind the
 *   decode leg.  d_pcm16, d_is_noise and d_is_comfort_noise complete
 *   on lyra_hip_stream_decode(); everything else, packets included, on lyra_hip_stream() (the quantizer stream is not used).
 *   lyra_hip_set_serial is supported; LYRA_HIP_SUBBATCHES > 1 is accepted (not split).
 *   Refusals, each LYRA_HIP_EINVAL with nothing enqueued and no state or error counter changed: a null call or required pointer;
 *   P outside 1 .. max_streams; span or lane ids out of range or named twice; negative or overlapping ranges; unequal n_frames;
 *   more than 2^30 - 1 span frames in all; a packet size or bit count off the lists on a span frame; a room of more than
 *   LYRA_HIP_BRIDGE_MAX_ROOM members; d_pcm16 / d_mix misaligned or equal; d_levels not 8-byte aligned; unknown flags;
 *   max_speakers outside 0 .. 8; DTX with an encoder rate other than 16000.  The pipelined host-buffer forms in flight
 *   interact with it as with the span calls it composes.
 *
 * lyra_hip_spans_bridge
 *   The host-buffer form: stages frames 0 .. the last span's end, runs lyra_hip_spans_bridge_dev, synchronises and writes the
 *   spans' frames of the outputs only; the caller's arrays outside the spans are untouched.  out_packets rows read back zero
 *   behind each packet's bytes.  pcm16, mix, is_noise, is_comfort_noise, levels and is_speaker may be NULL.
 *
 * Out of scope: shared encoders over spans, request sizes other than one hop, external sample rates (the bridge is 16 kHz by
 * construction), pipelined begin / end forms.  Participants who join, leave or move rooms inside one call: lyra_hip_spans_meeting.h. */
#ifndef LYRA_HIP_BRIDGE_SPANS_H_
#define LYRA_HIP_BRIDGE_SPANS_H_

#include "lyra_hip_speakers.h"
#include "lyra_hip_spans_mixed.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lyra_hip_spans_bridge_call {
  const lyra_hip_span* spans;        /* HOST [P]: participant p, every n_frames = T */
  int P;
  const int32_t* lane_ids;           /* HOST [n_lanes]: streams lent to both legs */
  int n_lanes;
  const int32_t* rooms;              /* HOST [P] labels, < 0: in no room */
  const uint8_t* d_packets;          /* [frames][23] incoming */
  const int32_t* packet_bytes;       /* HOST [frames] 0 / 8 / 15 / 23 */
  const int32_t* d_muted;            /* [frames], or NULL */
  unsigned flags;                    /* LYRA_HIP_BRIDGE_* */
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
} lyra_hip_spans_bridge_call;

int lyra_hip_spans_bridge_plan(const lyra_hip_span* spans, int P, const int32_t* rooms /* [P] */, int32_t* order /* [P] */,
                               int32_t* room_start /* [P + 1] */, int* n_rooms, int* n_members, int64_t* n_ticks);
int lyra_hip_spans_bridge_mix_dev(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int P, const int32_t* rooms,
                                  const int16_t* d_pcm16 /* [frames][320] */, const int32_t* d_muted /* [frames], or NULL */,
                                  const int32_t* d_is_comfort_noise /* [frames], or NULL */, int max_speakers,
                                  int16_t* d_mix /* [frames][320] */, int64_t* d_levels /* [frames], or NULL */,
                                  int32_t* d_is_speaker /* [frames], or NULL */);
int lyra_hip_spans_bridge_dev(lyra_hip_ctx* ctx, const lyra_hip_spans_bridge_call* call);
int lyra_hip_spans_bridge(lyra_hip_ctx* ctx, const lyra_hip_span* spans, int P, const int32_t* lane_ids, int n_lanes,
                          const int32_t* rooms, const uint8_t* packets /* [frames][23] */, const int32_t* packet_bytes,
                          const int32_t* muted /* [frames], or NULL */, unsigned flags, const int32_t* num_bits,
                          const int32_t* dtx /* [P], or NULL */, int max_speakers, uint8_t* out_packets /* [frames][23] */,
                          int32_t* out_packet_bytes /* [frames] */, int16_t* pcm16 /* [frames][320], or NULL */,
                          int16_t* mix /* [frames][320], or NULL */, int32_t* is_noise, int32_t* is_comfort_noise,
                          int64_t* levels, int32_t* is_speaker);

#ifdef __cplusplus
}
#endif
#endif  /* LYRA_HIP_BRIDGE_SPANS_H_ */
