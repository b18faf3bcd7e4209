// bridge_api.inc -- part of api.hip, behind speakers_api.inc and shared_bridge_api.inc (the mixes it dispatches to): the
// conference bridge (include/lyra_hip_bridge.h) and the entry points of its three kinds of tick -- the full mix, the loudest-N
// selection (include/lyra_hip_speakers.h) and the shared encoders (include/lyra_hip_shared_bridge.h).  Each of the mix call,
// the tick, begin() and end() is one body for all three; where the arrays of a tick lie in the staging is bridge_staging.h,
// the staging itself the context's slots of PL_BRIDGE (HostSlot, api.hip), with room for the largest tick of any kind.
//   lyra_hip_bridge_mix_dev: bridge_mix_kernel alone (bridge_kernels.hip), a stateless encode-side call on se[0].
//   lyra_hip_bridge_tick_dev: lossy_tick_launch (the decode leg, as lyra_hip_decode_lossy_mixed_dev at 16 kHz) -> the mix on
//     se[0] -> lyra_hip_encode_streams_dev on the mix (every rate 16000, row b at 320 * b).  The one edge the composition adds:
//     se[0] waits for an event that lossy_tick_launch records on the noise stream right behind lossy_mix_kernel
//     (lyra_hip_ctx::lossy_mix_hook), so the mix does not wait for the estimator behind it.  No per-stream state of its own.
//   lyra_hip_bridge_begin / _end: its two-deep host-buffer form, as decode_streams_api.inc: one upload from pinned staging on
//     the decode-side stream, no synchronisation; one download behind both legs on the quantizer stream, end() waits for its
//     event only.
#include "../../include/lyra_hip_bridge.h"
#include "bridge_plan.h"
#include "bridge_staging.h"

static_assert(bridge::MAX_ROOM == LYRA_HIP_BRIDGE_MAX_ROOM, "the planner's bound is the header's");
static_assert(bridge_staging::PACKET_BYTES == LYRA_HIP_MAX_PACKET_BYTES, "the staging's packet rows are the library's");

namespace {

using BrgKind = bridge_staging::Kind;

void brg_free(lyra_hip_ctx* c) {
  dfree(c->d_brg_mix[0], c->d_brg_mix[1], c->d_brg_flags[0], c->d_brg_flags[1], c->d_brg_const, c->d_bridge_err);
  c->brg_cap = 0;
  if (c->ev_brg_mix) (void)hipEventDestroy(c->ev_brg_mix);
  c->ev_brg_mix = nullptr;
}

// The error word of bridge_mix_kernel: all lyra_hip_bridge_mix_dev needs.
int brg_ensure_mix(lyra_hip_ctx* c) { return err_word_ensure(c, &c->d_bridge_err); }

// The edge's event, the constants of the encode leg (every rate 16000, row b at sample 320 * b) and the tick's scratch: the mix and the comfort-noise flags of a call that was given none.  Two sets, picked by lossy-call parity
// as d_dstr16 is (and like it not what keeps call n + 1 off call n's set today: tick n + 1's noise-stream half waits for tick
// n's quantizer, which runs behind tick n's mix).
int brg_ensure(lyra_hip_ctx* c, int B) {
  int rc = brg_ensure_mix(c);
  if (rc) return rc;
  if (!c->ev_brg_mix) HIPCHK(c, hipEventCreateWithFlags(&c->ev_brg_mix, hipEventDisableTiming));
  if ((rc = err_word_ensure(c, &c->d_mixed_err))) return rc;   // (encode16 would allocate it on the way: everything up front)
  if (!c->d_brg_const) {
    const size_t n = (size_t)c->max_streams;
    std::vector<int32_t> h(2 * n);
    for (size_t b = 0; b < n; ++b) {
      h[b] = 16000;
      h[n + b] = (int32_t)(320 * b);   // (at most max_streams * 960 < 2^31: lyra_hip_create's bound on max_streams)
    }
    HIPCHK(c, dalloc(&c->d_brg_const, 2 * n));
    HIPCHK(c, hipMemcpy(c->d_brg_const, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  }
  if (B <= c->brg_cap) return 0;
  if ((rc = sync_all(c))) return rc;   // (the buffers of the calls in flight)
  dfree(c->d_brg_mix[0], c->d_brg_mix[1], c->d_brg_flags[0], c->d_brg_flags[1]);
  c->brg_cap = 0;
  for (auto& p : c->d_brg_mix) HIPCHK(c, dalloc(&p, (size_t)B * 320));
  for (auto& p : c->d_brg_flags) HIPCHK(c, dalloc(&p, (size_t)B));
  c->brg_cap = B;
  return 0;
}

bool brg_misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; }

// the buffer checks of every mix call, the pass over spans (bridge_spans_api.inc) included; `mix_name`: d_mix or d_enc_mix
int brg_check_buffers(lyra_hip_ctx* c, const char* what, const int16_t* d_pcm16, const int16_t* d_mix, const char* mix_name,
                      const int64_t* d_levels) {
  if (brg_misaligned(d_pcm16) || brg_misaligned(d_mix) || d_pcm16 == d_mix)
    return fail(c, LYRA_HIP_EINVAL, "%s: d_pcm16 and %s must be 16-byte aligned and distinct", what, mix_name);
  if ((reinterpret_cast<uintptr_t>(d_levels) & 7u) != 0) return fail(c, LYRA_HIP_EINVAL, "%s: d_levels must be 8-byte aligned", what);
  return 0;
}

int brg_check_index(lyra_hip_ctx* c, const char* what, int B, const int32_t* d_order, const int32_t* d_room_start, int n_rooms,
                    int n_members) {
  if (n_rooms < 0 || n_rooms > B || n_members < 0 || n_members > B)
    return fail(c, LYRA_HIP_EINVAL, "%s: n_rooms %d or n_members %d outside 0..B (%d)", what, n_rooms, n_members, B);
  if ((n_rooms > 0 && !d_room_start) || (n_members > 0 && !d_order)) return fail(c, LYRA_HIP_EINVAL, "%s: null index", what);
  return 0;
}

// zero the mix (rows no room names), then one wavefront per room; on se[0]
int brg_mix_launch(lyra_hip_ctx* c, const int16_t* d_pcm16, int B, const int32_t* d_order, const int32_t* d_room_start,
                   int n_rooms, int n_members, const int32_t* d_muted, const int32_t* d_is_cn, int16_t* d_mix) {
  HIPCHK(c, hipMemsetAsync(d_mix, 0, (size_t)B * 640, c->se[0]));
  if (n_rooms > 0 && n_members > 0) {
    hipLaunchKernelGGL(bridge_mix_kernel, dim3(cdiv(n_rooms, 4)), dim3(256), 0, c->se[0], d_pcm16, B, d_order, d_room_start,
                       n_rooms, n_members, d_muted, d_is_cn, d_mix, c->d_bridge_err);
    HIPCHK(c, hipGetLastError());
  }
  return 0;
}

// A mix of any kind, as the three mix calls and the tick hand it over.  max_speakers 0: the full mix; 1 .. 8: the selection
// (speakers_api.inc) with d_levels and d_is_speaker; with `sh`, the shared encoders' (shared_bridge_api.inc), whose d_mix is
// the encoder rows' and which reads d_stream_ids and writes d_slot_of.
struct BrgMix {
  const int16_t* d_pcm16;
  const int32_t* d_stream_ids;
  int B;
  const int32_t *d_order, *d_room_start;
  int n_rooms, n_members;
  const int32_t *d_muted, *d_is_cn;
  int max_speakers;
  const ShrTick* sh;
  int16_t* d_mix;
  int64_t* d_levels;
  int32_t *d_is_speaker, *d_slot_of;
};

// the kernels of the mix on se[0]; the scratch of its kind has been ensured
int brg_mix_any(lyra_hip_ctx* c, const BrgMix& M, int set) {
  if (M.sh)
    return shr_mix_launch(c, M.d_pcm16, M.d_stream_ids, M.B, M.d_order, M.d_room_start, M.n_rooms, M.n_members, M.d_muted, M.d_is_cn,
                          M.max_speakers, *M.sh, M.d_mix, M.d_levels, M.d_is_speaker,
                          M.d_slot_of ? M.d_slot_of : c->d_shr_slot_of[set], set);
  if (M.max_speakers)
    return spk_mix_launch(c, M.d_pcm16, M.B, M.d_order, M.d_room_start, M.n_rooms, M.n_members, M.d_muted, M.d_is_cn,
                          M.max_speakers, M.d_mix, M.d_levels, M.d_is_speaker, set);
  return brg_mix_launch(c, M.d_pcm16, M.B, M.d_order, M.d_room_start, M.n_rooms, M.n_members, M.d_muted, M.d_is_cn, M.d_mix);
}

// The mix alone, a stateless encode-side call on se[0]: lyra_hip_bridge_mix_dev (`select` false), lyra_hip_speakers_mix_dev
// and, with M.sh, lyra_hip_shared_mix_dev.
int brg_mix_call(lyra_hip_ctx* c, const char* what, const BrgMix& M, bool select) {
  int rc = check_batch(c, M.B);
  if (rc) return rc;
  if (!M.d_pcm16 || !M.d_mix || (M.sh && (!M.d_stream_ids || !M.sh->d_slots))) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  if ((rc = brg_check_index(c, what, M.B, M.d_order, M.d_room_start, M.n_rooms, M.n_members))) return rc;
  if ((rc = brg_check_buffers(c, what, M.d_pcm16, M.d_mix, M.sh ? "d_enc_mix" : "d_mix", M.d_levels))) return rc;
  if (select && (rc = spk_check_n(c, what, M.max_speakers))) return rc;
  if (M.sh && M.sh->n_table_rooms < 1) return fail(c, LYRA_HIP_EINVAL, "%s: n_table_rooms %d", what, M.sh->n_table_rooms);
  DEVSCOPE(c);
  if ((rc = brg_ensure_mix(c))) return rc;
  if (select && (rc = spk_ensure(c, M.B))) return rc;
  if (M.sh && (rc = shr_ensure(c, M.B))) return rc;   // (the encoder mixes are the caller's: the scratch is sized by B alone)
  if ((rc = enc_side_begin(c, 0))) return rc;
  rc = brg_mix_any(c, M, (int)(c->n_lossy_calls & 1));
  if (!rc) rc = enc_side_done(c, 0);
  return rc;
}

// begin() of every kind of tick: two ticks deep, no pipelined request of any other kind in flight (the tick runs on both sides'
// streams), no decoder-twin request being assembled.  (pl_admit with the wording the three kinds of tick have always had.)
int brg_admit(lyra_hip_ctx* c, const char* what) {
  if (pl_in_flight(c, PL_BRIDGE) >= PL_DEPTH)
    return fail(c, LYRA_HIP_EINVAL, "%s: two ticks are already in flight (call _end first)", what);
  if (pl_blocker(c, PL_BRIDGE) >= 0 || c->twin_out_n != 0)
    return fail(c, LYRA_HIP_EINVAL, "%s: another pipelined request is in flight (call its _end first)", what);
  return 0;
}

// One tick, for every kind of mix.  max_speakers 0: the full mix of lyra_hip_bridge_tick_dev; 1 .. 8: the selection mix of
// lyra_hip_speakers_tick_dev (speakers_api.inc) with its two further outputs; with `sh`, the shared-encoder tick of
// lyra_hip_shared_tick_dev (shared_bridge_api.inc): the selection, then E = n_rooms * (1 + max_speakers) encoder rows in place of
// B and the fan-out behind the quantizer (T->d_num_bits, d_dtx and d_mix are not read).  `what` names the call in messages.
int brg_tick_impl(lyra_hip_ctx* c, const char* what, const lyra_hip_bridge_tick* T, int max_speakers, int64_t* d_levels,
                  int32_t* d_is_speaker, const ShrTick* sh = nullptr) {
  const int B = T->B;
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (!T->d_stream_ids || !T->d_packets || !T->d_packet_bytes || (!sh && !T->d_num_bits) || !T->d_out_packets ||
      !T->d_out_packet_bytes)
    return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  if ((rc = brg_check_index(c, what, B, T->d_order, T->d_room_start, T->n_rooms, T->n_members))) return rc;
  const int E = sh ? T->n_rooms * (1 + max_speakers) : 0;   // (n_rooms <= B: at most 9 * max_streams)
  if (sh) {
    if (!sh->d_slots || (E > 0 && (!sh->d_enc_stream_ids || !sh->d_enc_num_bits)))
      return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
    if (sh->n_table_rooms < 1) return fail(c, LYRA_HIP_EINVAL, "%s: n_table_rooms %d", what, sh->n_table_rooms);
    if (E > c->max_streams)
      return fail(c, LYRA_HIP_EINVAL, "%s: %d rooms x (1 + %d) encoder rows exceed max_streams (%d): use the loudest-N tick", what,
                  T->n_rooms, max_speakers, c->max_streams);
    if (brg_misaligned(sh->d_enc_mix) || (sh->d_enc_mix && T->d_pcm16 == sh->d_enc_mix))
      return fail(c, LYRA_HIP_EINVAL, "%s: d_pcm16 and d_enc_mix must be 16-byte aligned and distinct", what);
  }
  if (T->flags & ~LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE) return fail(c, LYRA_HIP_EINVAL, "%s: unknown flags 0x%x", what, T->flags);
  if (brg_misaligned(T->d_pcm16) || brg_misaligned(T->d_mix) || (T->d_mix && T->d_pcm16 == T->d_mix))
    return fail(c, LYRA_HIP_EINVAL, "%s: d_pcm16 and d_mix must be 16-byte aligned and distinct", what);
  DEVSCOPE(c);
  // everything the tick allocates or builds on first use, BEFORE anything is enqueued
  if ((rc = ensure_scratch(c, std::max(B, E)))) return rc;   // (E: the encode leg of a shared-encoder tick, else 0)
  if ((rc = rates_ensure(c))) return rc;
  if ((rc = lossy_ensure(c, B))) return rc;
  if (!T->d_pcm16 && (rc = dstr16_ensure(c, B))) return rc;
  if ((rc = brg_ensure(c, B))) return rc;
  if (max_speakers && (rc = spk_ensure(c, B))) return rc;
  if (sh && (rc = shr_ensure(c, std::max(B, E)))) return rc;
  const int set = (int)(c->n_lossy_calls & 1);
  const bool skip_cn = (T->flags & LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE) != 0;
  int16_t* pcm16 = T->d_pcm16 ? T->d_pcm16 : c->d_dstr16[set];
  int16_t* mix = sh ? (sh->d_enc_mix ? sh->d_enc_mix : c->d_shr_mix[set]) : T->d_mix ? T->d_mix : c->d_brg_mix[set];
  int32_t* is_cn = T->d_is_comfort_noise ? T->d_is_comfort_noise : skip_cn ? c->d_brg_flags[set] : nullptr;
  // ---- decode leg: lyra_hip_decode_lossy_mixed_dev at 16 kHz, with the event behind its mix ----
  c->lossy_mix_hook = c->ev_brg_mix;
  rc = lossy_tick_launch(c, T->d_stream_ids, B, T->d_packets, T->d_packet_bytes, nullptr, 0, 16000, pcm16, nullptr, T->d_is_noise,
                         is_cn, LOSSY_MIXED_BYTES);
  c->lossy_mix_hook = nullptr;
  if (rc) return rc;
  // ---- the edge and the mix: se[0] behind this tick's hop and flags ----
  if ((rc = enc_cross_begin(c, 0, 1))) return rc;
  HIPCHK(c, hipStreamWaitEvent(c->se[0], c->ev_brg_mix, 0));
  int32_t* slot_of = sh ? (sh->d_slot_of ? sh->d_slot_of : c->d_shr_slot_of[set]) : nullptr;
  const BrgMix M = {pcm16, T->d_stream_ids, B, T->d_order, T->d_room_start, T->n_rooms, T->n_members, T->d_muted,
                    skip_cn ? is_cn : nullptr, max_speakers, sh, mix, d_levels, d_is_speaker, slot_of};
  if ((rc = brg_mix_any(c, M, set))) return rc;
  // ---- encode leg ----
  const int32_t* rates16 = c->d_brg_const;
  if (sh) return shr_encode_fanout(c, T, max_speakers, E, *sh, mix, slot_of, set);
  return lyra_hip_encode_streams_dev(c, T->d_stream_ids, B, mix, 320L * B, rates16 + c->max_streams, rates16, T->d_num_bits,
                                     T->d_dtx, T->d_out_packets, T->d_out_packet_bytes);
}

// what lyra_hip_shared_begin has in place of num_bits and dtx: the labels of the rooms present and their encoder rows
struct ShrBegin {
  const int32_t* room_labels;
  int n_rooms;
  const int32_t *enc_ids, *enc_bits, *enc_dtx;
};

// begin() of every kind of tick (max_speakers as in brg_tick_impl; `sb`: a shared-encoder tick): one validation, one staging,
// one upload, one download
int brg_begin_impl(lyra_hip_ctx* c, const char* what, const int32_t* ids, int B, const uint8_t* packets,
                   const int32_t* packet_bytes, const int32_t* rooms, const int32_t* muted, unsigned flags,
                   const int32_t* num_bits, const int32_t* dtx, int max_speakers, const ShrBegin* sb = nullptr) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (!packets || !packet_bytes || !rooms ||
      (sb ? sb->n_rooms > 0 && (!sb->room_labels || !sb->enc_ids || !sb->enc_bits) : !num_bits))
    return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  if (flags & ~LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE) return fail(c, LYRA_HIP_EINVAL, "%s: unknown flags 0x%x", what, flags);
  int E = 0;
  if (sb) {   // the encoder rows: their count, and their ids in front of the participants'
    if (sb->n_rooms < 0 || sb->n_rooms > B) return fail(c, LYRA_HIP_EINVAL, "%s: n_rooms %d outside 0..B (%d)", what, sb->n_rooms, B);
    E = sb->n_rooms * (1 + max_speakers);
    if (E > c->max_streams)
      return fail(c, LYRA_HIP_EINVAL, "%s: %d rooms x (1 + %d) encoder rows exceed max_streams (%d): use the loudest-N tick", what,
                  sb->n_rooms, max_speakers, c->max_streams);
    if (E > 0 && (rc = check_ids_host(c, sb->enc_ids, E))) return rc;
  }
  if ((rc = check_ids_host(c, ids, B))) return rc;
  for (int e = 0; e < E; ++e)
    if ((rc = check_bits(c, sb->enc_bits[e]))) return rc;
  for (int b = 0; b < B; ++b) {
    if (!sb && (rc = check_bits(c, num_bits[b]))) return rc;
    const int pb = packet_bytes[b];   // PacketSizeToNumQuantizedBits (lyra_config.h:99-106), 0: no packet on this tick
    if (pb != 0 && pb != 8 && pb != 15 && pb != LYRA_HIP_MAX_PACKET_BYTES)
      return fail(c, LYRA_HIP_EINVAL, "%s: packet of %d bytes at position %d (0, 8, 15 or 23)", what, pb, b);
  }
  if ((rc = brg_admit(c, what))) return rc;
  DEVSCOPE(c);
  HostSlot& S = host_slot_begin(c, PL_BRIDGE);
  if ((rc = host_slot_ensure(c, S, host_staging::bridge((size_t)c->max_streams)))) return rc;
  const BrgKind kind = sb ? bridge_staging::SHARED : max_speakers ? bridge_staging::SPEAKERS : bridge_staging::FULL;
  const bridge_staging::Layout L = bridge_staging::layout(kind, (size_t)B, (size_t)E);
  int32_t* h = reinterpret_cast<int32_t*>(S.h_in);
  int n_rooms = 0, n_members = 0;
  if (bridge::plan(rooms, B, h + L.order, h + L.room_start, &n_rooms, &n_members))
    return fail(c, LYRA_HIP_EINVAL, "%s: a room of more than %d members", what, LYRA_HIP_BRIDGE_MAX_ROOM);
  int at = -1;
  if (const int bad = sb ? shared_bridge::check_labels(rooms, h + L.order, h + L.room_start, n_rooms, sb->room_labels, sb->n_rooms,
                                                       c->max_streams, &at)
                         : 0)
    return fail(c, LYRA_HIP_EINVAL, "%s: room_labels (%d given, %d rooms present; position %d, code %d) must be the labels "
                "present in rooms, strictly ascending and below max_streams (%d)", what, sb->n_rooms, n_rooms, at, bad, c->max_streams);
  // everything the tick allocates or builds on first use, BEFORE anything is enqueued: a failure here leaves the streams idle
  if ((rc = ensure_scratch(c, std::max(B, E)))) return rc;
  if ((rc = rates_ensure(c))) return rc;
  if ((rc = lossy_ensure(c, B))) return rc;
  if ((rc = dstr16_ensure(c, B))) return rc;
  if ((rc = brg_ensure(c, B))) return rc;
  if (max_speakers && (rc = spk_ensure(c, B))) return rc;
  if (sb) {
    if ((rc = shr_ensure(c, std::max(B, E)))) return rc;
    if (!c->d_shr_table) {   // one row per label below max_streams, all free
      HIPCHK(c, dalloc(&c->d_shr_table, (size_t)c->max_streams * LYRA_HIP_SHARED_SLOTS));
      HIPCHK(c, hipMemset(c->d_shr_table, 0xFF, (size_t)c->max_streams * LYRA_HIP_SHARED_SLOTS * 4));
    }
  }
  for (int b = 0; b < B; ++b) {
    h[L.ids + b] = ids[b];
    h[L.packet_bytes + b] = packet_bytes[b];
    h[L.muted + b] = muted ? (muted[b] != 0) : 0;
    if (sb) continue;
    h[L.num_bits + b] = num_bits[b];
    h[L.dtx + b] = dtx ? (dtx[b] != 0) : 0;
  }
  for (int r = 0; sb && r < n_rooms; ++r) h[L.room_keys + r] = sb->room_labels[r];
  for (int e = 0; e < E; ++e) {
    h[L.enc_ids + e] = sb->enc_ids[e];
    h[L.enc_bits + e] = sb->enc_bits[e];
    h[L.enc_dtx + e] = sb->enc_dtx ? (sb->enc_dtx[e] != 0) : 0;
  }
  std::memcpy(S.h_in + L.in_packets * 4, packets, (size_t)B * LYRA_HIP_MAX_PACKET_BYTES);
  // one upload from pinned staging on the decode-side stream, in front of the tick's first kernel.  The encode leg reads ids,
  // bits and DTX flags on se[0] / sq[0]: both are behind the tick's edge, which is behind the decode-side half and so the copy.
  HIPCHK(c, hipMemcpyAsync(S.d_in, S.h_in, L.in_bytes, hipMemcpyHostToDevice, c->sd[0]));
  const int32_t* m = reinterpret_cast<const int32_t*>(S.d_in);
  int32_t* o = reinterpret_cast<int32_t*>(S.d_out);
  uint8_t* out_pk = S.d_out + L.out_packets * 4;
  // empty packets, and the bytes behind a shorter one, read back as zeros; the extractor's stream is ahead of the quantizer's
  // (a shared-encoder tick's fan-out writes every byte of them)
  if (!sb) HIPCHK(c, hipMemsetAsync(out_pk, 0, (size_t)B * LYRA_HIP_MAX_PACKET_BYTES, c->se[0]));
  lyra_hip_bridge_tick T = {};
  T.d_stream_ids = m + L.ids;
  T.B = B;
  T.d_packets = S.d_in + L.in_packets * 4;
  T.d_packet_bytes = m + L.packet_bytes;
  T.d_order = m + L.order;
  T.d_room_start = m + L.room_start;
  T.n_rooms = n_rooms;
  T.n_members = n_members;
  T.d_muted = muted ? m + L.muted : nullptr;
  T.flags = flags;
  T.d_num_bits = sb ? nullptr : m + L.num_bits;
  T.d_dtx = dtx ? m + L.dtx : nullptr;
  T.d_out_packets = out_pk;
  T.d_out_packet_bytes = o + L.out_packet_bytes;
  T.d_is_noise = o + L.is_noise;
  T.d_is_comfort_noise = o + L.is_comfort_noise;
  ShrTick sh = {};
  if (sb) {
    sh.d_room_keys = m + L.room_keys;
    sh.d_slots = c->d_shr_table;
    sh.n_table_rooms = c->max_streams;
    sh.d_enc_stream_ids = m + L.enc_ids;
    sh.d_enc_num_bits = m + L.enc_bits;
    sh.d_enc_dtx = sb->enc_dtx ? m + L.enc_dtx : nullptr;
    sh.d_slot_of = o + L.slot_of;
  }
  if ((rc = brg_tick_impl(c, what, &T, max_speakers, max_speakers ? reinterpret_cast<int64_t*>(o + L.levels) : nullptr,
                          max_speakers ? o + L.is_speaker : nullptr, sb ? &sh : nullptr)))
    return rc;
  // packets and sizes are written by the quantizer on sq[0] (a shared-encoder tick: by the fan-out behind it), the flags by the
  // noise-stream half: the one download rides on sq[0] behind the end of that half (the quantizer itself is already enqueued and
  // does not wait for it).  The levels, speaker flags and slot_of of a selection tick are written on se[0] by the mix's kernels:
  // the quantizer on sq[0] waits for the extractor's event on se[0] (encq_handoff, api.hip), which is enqueued behind them, so
  // sq[0] is behind them as well.  A shared-encoder tick without rooms has no quantizer and ends on se[0] instead.
  HIPCHK(c, hipStreamWaitEvent(c->sq[0], c->ev_noise[(c->n_noise_calls - 1) & 1], 0));
  if (sb && E == 0) HIPCHK(c, hipStreamWaitEvent(c->sq[0], c->ev_encs[2][0], 0));
  HIPCHK(c, hipMemcpyAsync(S.h_out, S.d_out, L.out_bytes, hipMemcpyDeviceToHost, c->sq[0]));
  S.kind = kind;
  return host_slot_begun(c, PL_BRIDGE, S, B, c->sq[0]);
}

// end() of every kind of tick: `kind` is the caller's, and the optional outputs are those its kind of tick has
int brg_end_impl(lyra_hip_ctx* c, const char* what, BrgKind kind, uint8_t* out_packets, int32_t* out_packet_bytes, int32_t* is_noise,
                 int32_t* is_comfort_noise, int64_t* levels = nullptr, int32_t* is_speaker = nullptr, int32_t* slot_of = nullptr) {
  HostSlot* oldest = host_slot_oldest(c, PL_BRIDGE, what);
  if (!oldest) return LYRA_HIP_EINVAL;
  HostSlot& S = *oldest;
  static const char* const begun_by[] = {"the full-mix begin()", "lyra_hip_speakers_begin", "lyra_hip_shared_begin"};
  if (S.kind != kind) return fail(c, LYRA_HIP_EINVAL, "%s: the oldest tick was begun by %s", what, begun_by[S.kind]);
  if (!out_packets || !out_packet_bytes) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  DEVSCOPE(c);
  if (const int rc = host_slot_ended(c, PL_BRIDGE, S, true)) return rc;
  const size_t n = (size_t)S.B;
  const bridge_staging::Layout L = bridge_staging::layout(kind, n, 0);   // (what comes down does not depend on E)
  const int32_t* o = reinterpret_cast<const int32_t*>(S.h_out);
  std::memcpy(out_packet_bytes, o + L.out_packet_bytes, n * 4);
  if (is_noise) std::memcpy(is_noise, o + L.is_noise, n * 4);
  if (is_comfort_noise) std::memcpy(is_comfort_noise, o + L.is_comfort_noise, n * 4);
  if (is_speaker) std::memcpy(is_speaker, o + L.is_speaker, n * 4);
  if (levels) std::memcpy(levels, o + L.levels, n * 8);
  if (slot_of) std::memcpy(slot_of, o + L.slot_of, n * 4);
  std::memcpy(out_packets, o + L.out_packets, n * LYRA_HIP_MAX_PACKET_BYTES);
  return 0;
}

// the fields the three public tick structs have in common (they are separate types, with the same names)
template <class Tick>
lyra_hip_bridge_tick brg_common_fields(const Tick& S) {
  lyra_hip_bridge_tick T = {};
  T.d_stream_ids = S.d_stream_ids;
  T.B = S.B;
  T.d_packets = S.d_packets;
  T.d_packet_bytes = S.d_packet_bytes;
  T.d_order = S.d_order;
  T.d_room_start = S.d_room_start;
  T.n_rooms = S.n_rooms;
  T.n_members = S.n_members;
  T.d_muted = S.d_muted;
  T.flags = S.flags;
  T.d_out_packets = S.d_out_packets;
  T.d_out_packet_bytes = S.d_out_packet_bytes;
  T.d_pcm16 = S.d_pcm16;
  T.d_is_noise = S.d_is_noise;
  T.d_is_comfort_noise = S.d_is_comfort_noise;
  return T;
}

// the refusals of a selection tick's struct, in front of brg_tick_impl's
template <class Tick>
int brg_check_selection(lyra_hip_ctx* c, const char* what, const Tick* S) {
  if (!S) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  const int rc = spk_check_n(c, what, S->max_speakers);
  if (rc) return rc;
  if ((reinterpret_cast<uintptr_t>(S->d_levels) & 7u) != 0) return fail(c, LYRA_HIP_EINVAL, "%s: d_levels must be 8-byte aligned", what);
  return 0;
}

}  // namespace

extern "C" {

int lyra_hip_bridge_plan(const int32_t* rooms, int B, int32_t* order, int32_t* room_start, int* n_rooms, int* n_members) {
  return bridge::plan(rooms, B, order, room_start, n_rooms, n_members) ? LYRA_HIP_EINVAL : 0;
}

// ---- the mix alone ----

int lyra_hip_bridge_mix_dev(lyra_hip_ctx* c, const int16_t* d_pcm16, int B, const int32_t* d_order, const int32_t* d_room_start,
                            int n_rooms, int n_members, const int32_t* d_muted, const int32_t* d_is_comfort_noise,
                            int16_t* d_mix) {
  const BrgMix M = {d_pcm16, nullptr, B, d_order, d_room_start, n_rooms, n_members, d_muted, d_is_comfort_noise, 0, nullptr, d_mix,
                    nullptr, nullptr, nullptr};
  return brg_mix_call(c, "bridge_mix", M, false);
}

int lyra_hip_speakers_mix_dev(lyra_hip_ctx* c, const int16_t* d_pcm16, int B, const int32_t* d_order, const int32_t* d_room_start,
                              int n_rooms, int n_members, const int32_t* d_muted, const int32_t* d_is_comfort_noise,
                              int max_speakers, int16_t* d_mix, int64_t* d_levels, int32_t* d_is_speaker) {
  const BrgMix M = {d_pcm16, nullptr, B, d_order, d_room_start, n_rooms, n_members, d_muted, d_is_comfort_noise, max_speakers,
                    nullptr, d_mix, d_levels, d_is_speaker, nullptr};
  return brg_mix_call(c, "speakers_mix", M, true);
}

int lyra_hip_shared_mix_dev(lyra_hip_ctx* c, const int16_t* d_pcm16, const int32_t* d_stream_ids, int B, const int32_t* d_order,
                            const int32_t* d_room_start, int n_rooms, int n_members, const int32_t* d_muted,
                            const int32_t* d_is_comfort_noise, int max_speakers, const int32_t* d_room_keys, int32_t* d_slots,
                            int n_table_rooms, int16_t* d_enc_mix, int64_t* d_levels, int32_t* d_is_speaker, int32_t* d_slot_of) {
  ShrTick sh = {};
  sh.d_room_keys = d_room_keys;
  sh.d_slots = d_slots;
  sh.n_table_rooms = n_table_rooms;
  const BrgMix M = {d_pcm16, d_stream_ids, B, d_order, d_room_start, n_rooms, n_members, d_muted, d_is_comfort_noise, max_speakers,
                    &sh, d_enc_mix, d_levels, d_is_speaker, d_slot_of};
  return brg_mix_call(c, "shared_mix", M, true);
}

// ---- one tick on device buffers ----

int lyra_hip_bridge_tick_dev(lyra_hip_ctx* c, const lyra_hip_bridge_tick* T) {
  if (!c) return LYRA_HIP_EINVAL;
  if (!T) return fail(c, LYRA_HIP_EINVAL, "bridge_tick: null pointer");
  return brg_tick_impl(c, "bridge_tick", T, 0, nullptr, nullptr);
}

int lyra_hip_speakers_tick_dev(lyra_hip_ctx* c, const lyra_hip_speakers_tick* S) {
  if (!c) return LYRA_HIP_EINVAL;
  const int rc = brg_check_selection(c, "speakers_tick", S);
  if (rc) return rc;
  lyra_hip_bridge_tick T = brg_common_fields(*S);
  T.d_num_bits = S->d_num_bits;
  T.d_dtx = S->d_dtx;
  T.d_mix = S->d_mix;
  return brg_tick_impl(c, "speakers_tick", &T, S->max_speakers, S->d_levels, S->d_is_speaker);
}

int lyra_hip_shared_tick_dev(lyra_hip_ctx* c, const lyra_hip_shared_tick* S) {
  if (!c) return LYRA_HIP_EINVAL;
  const int rc = brg_check_selection(c, "shared_tick", S);
  if (rc) return rc;
  const lyra_hip_bridge_tick T = brg_common_fields(*S);
  const ShrTick sh = {S->d_room_keys, S->d_slots, S->n_table_rooms, S->d_enc_stream_ids, S->d_enc_num_bits, S->d_enc_dtx,
                      S->d_enc_mix, S->d_enc_packets, S->d_enc_packet_bytes, S->d_slot_of};
  return brg_tick_impl(c, "shared_tick", &T, S->max_speakers, S->d_levels, S->d_is_speaker, &sh);
}

// ---- the two-deep host-buffer form ----

int lyra_hip_bridge_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets, const int32_t* packet_bytes,
                          const int32_t* rooms, const int32_t* muted, unsigned flags, const int32_t* num_bits,
                          const int32_t* dtx) {
  if (!c) return LYRA_HIP_EINVAL;
  return brg_begin_impl(c, "bridge_begin", ids, B, packets, packet_bytes, rooms, muted, flags, num_bits, dtx, 0);
}

int lyra_hip_speakers_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets, const int32_t* packet_bytes,
                            const int32_t* rooms, const int32_t* muted, unsigned flags, const int32_t* num_bits,
                            const int32_t* dtx, int max_speakers) {
  if (!c) return LYRA_HIP_EINVAL;
  int rc = spk_check_n(c, "speakers_begin", max_speakers);
  if (rc) return rc;
  return brg_begin_impl(c, "speakers_begin", ids, B, packets, packet_bytes, rooms, muted, flags, num_bits, dtx, max_speakers);
}

int lyra_hip_shared_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets, const int32_t* packet_bytes,
                          const int32_t* rooms, const int32_t* muted, unsigned flags, int max_speakers, const int32_t* room_labels,
                          int n_rooms, const int32_t* enc_ids, const int32_t* enc_bits, const int32_t* enc_dtx) {
  if (!c) return LYRA_HIP_EINVAL;
  int rc = spk_check_n(c, "shared_begin", max_speakers);
  if (rc) return rc;
  const ShrBegin sb = {room_labels, n_rooms, enc_ids, enc_bits, enc_dtx};
  return brg_begin_impl(c, "shared_begin", ids, B, packets, packet_bytes, rooms, muted, flags, nullptr, nullptr, max_speakers, &sb);
}

int lyra_hip_bridge_end(lyra_hip_ctx* c, uint8_t* out_packets, int32_t* out_packet_bytes, int32_t* is_noise,
                        int32_t* is_comfort_noise) {
  if (!c) return LYRA_HIP_EINVAL;
  return brg_end_impl(c, "bridge_end", bridge_staging::FULL, out_packets, out_packet_bytes, is_noise, is_comfort_noise);
}

int lyra_hip_speakers_end(lyra_hip_ctx* c, uint8_t* out_packets, int32_t* out_packet_bytes, int32_t* is_noise,
                          int32_t* is_comfort_noise, int64_t* levels, int32_t* is_speaker) {
  if (!c) return LYRA_HIP_EINVAL;
  return brg_end_impl(c, "speakers_end", bridge_staging::SPEAKERS, out_packets, out_packet_bytes, is_noise, is_comfort_noise, levels,
                      is_speaker);
}

int lyra_hip_shared_end(lyra_hip_ctx* c, uint8_t* out_packets, int32_t* out_packet_bytes, int32_t* is_noise,
                        int32_t* is_comfort_noise, int64_t* levels, int32_t* is_speaker, int32_t* slot_of) {
  if (!c) return LYRA_HIP_EINVAL;
  return brg_end_impl(c, "shared_end", bridge_staging::SHARED, out_packets, out_packet_bytes, is_noise, is_comfort_noise, levels,
                      is_speaker, slot_of);
}

long lyra_hip_bridge_errors(lyra_hip_ctx* c, int clear) {
  return read_error_counter(c, &lyra_hip_ctx::d_bridge_err, clear);
}

}  // extern "C"
