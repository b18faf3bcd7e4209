// bridge_api.inc -- part of api.hip: the conference bridge (include/lyra_hip_bridge.h).
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

static_assert(bridge::MAX_ROOM == LYRA_HIP_BRIDGE_MAX_ROOM, "the planner's bound is the header's");

namespace {

struct BrgSlot {
  uint8_t* h_in = nullptr;     // pinned: the int32 arrays going up (kBrgInArrays, below), then packets [B][23]
  uint8_t* h_out = nullptr;    // pinned: [out_packet_bytes | is_noise | is_comfort_noise] int32, B each, then out packets [B][23]
  uint8_t* d_in = nullptr;     // the same on the device (room for max_streams rows each)
  uint8_t* d_out = nullptr;
  hipEvent_t ev_done = nullptr;
  int B = 0;
  int max_speakers = 0;        // 0: a full-mix tick (lyra_hip_bridge_begin); else a tick of lyra_hip_speakers_begin ...
  bool shared = false;         // ... or, with this set, of lyra_hip_shared_begin (shared_bridge_api.inc)
};
struct BrgHost { BrgSlot slot[2]; };

// going up, int32 [n] each (room_start: n + 1): ids | packet_bytes | order | muted | num_bits | dtx | room_start
constexpr size_t kBrgInArrays = 7;
size_t brg_in_bytes(size_t n) { return (kBrgInArrays * n + 1) * 4 + n * LYRA_HIP_MAX_PACKET_BYTES; }
size_t brg_out_bytes(size_t n) { return 3 * n * 4 + n * LYRA_HIP_MAX_PACKET_BYTES; }
// a tick of lyra_hip_speakers_begin (speakers_api.inc) comes down through the same slots as
// [out_packet_bytes | is_noise | is_comfort_noise | is_speaker] int32, levels int64, out packets: the slots have room for it
constexpr size_t kSpkOutWords = 6;
size_t spk_out_bytes(size_t n) { return kSpkOutWords * n * 4 + n * LYRA_HIP_MAX_PACKET_BYTES; }
// speakers_api.inc: the scratch of the selection mix, and its three kernels on se[0]
int spk_ensure(lyra_hip_ctx* c, int B);
int spk_mix_launch(lyra_hip_ctx* c, const int16_t* d_pcm16, int B, const int32_t* d_order, const int32_t* d_room_start,
                   int n_rooms, int n_members, const int32_t* d_muted, const int32_t* d_is_cn, int max_speakers, int16_t* d_mix,
                   int64_t* d_levels, int32_t* d_is_speaker, int set);
// shared_bridge_api.inc: what a shared-encoder tick has in place of the per-listener bit counts, DTX flags and mix; its
// scratch; its mix on se[0] (levels, selection, slot update, the E encoder mixes); and its staging, which is the largest:
// going up [ids | packet_bytes | order | muted | room_start | room_keys | enc_ids | enc_bits | enc_dtx], coming down
// [out_packet_bytes | is_noise | is_comfort_noise | is_speaker] int32, levels int64, slot_of int32, out packets
struct ShrTick {
  const int32_t* d_room_keys;
  int32_t* d_slots;
  int n_table_rooms;
  const int32_t *d_enc_stream_ids, *d_enc_num_bits, *d_enc_dtx;
  int16_t* d_enc_mix;
  uint8_t* d_enc_packets;
  int32_t *d_enc_packet_bytes, *d_slot_of;
};
constexpr size_t kShrInArrays = 9, kShrOutWords = 7;
size_t shr_in_bytes(size_t n) { return (kShrInArrays * n + 1) * 4 + n * LYRA_HIP_MAX_PACKET_BYTES; }
size_t shr_out_bytes(size_t n) { return kShrOutWords * n * 4 + n * LYRA_HIP_MAX_PACKET_BYTES; }
int shr_ensure(lyra_hip_ctx* c, int rows);
int shr_mix_launch(lyra_hip_ctx* c, const int16_t* d_pcm16, const int32_t* d_stream_ids, int B, const int32_t* d_order,
                   const int32_t* d_room_start, int n_rooms, int n_members, const int32_t* d_muted, const int32_t* d_is_cn,
                   int max_speakers, const ShrTick& sh, int16_t* d_enc_mix, int64_t* d_levels, int32_t* d_is_speaker,
                   int32_t* d_slot_of, int set);

void brg_free(lyra_hip_ctx* c) {
  dfree(c->d_brg_mix[0], c->d_brg_mix[1], c->d_brg_flags[0], c->d_brg_flags[1], c->d_brg_const, c->d_bridge_err);
  c->brg_cap = 0;
  if (c->ev_brg_mix) (void)hipEventDestroy(c->ev_brg_mix);
  c->ev_brg_mix = nullptr;
  BrgHost* H = static_cast<BrgHost*>(c->brg_host);
  if (!H) return;
  for (BrgSlot& S : H->slot) {
    if (S.h_in) (void)hipHostFree(S.h_in);
    if (S.h_out) (void)hipHostFree(S.h_out);
    dfree(S.d_in, S.d_out);
    if (S.ev_done) (void)hipEventDestroy(S.ev_done);
  }
  delete H;
  c->brg_host = nullptr;
}

int brg_slot_ensure(lyra_hip_ctx* c, BrgSlot* S) {
  const size_t n = (size_t)c->max_streams;
  if (!S->h_in) HIPCHK(c, hipHostMalloc((void**)&S->h_in, shr_in_bytes(n), hipHostMallocDefault));
  if (!S->h_out) HIPCHK(c, hipHostMalloc((void**)&S->h_out, shr_out_bytes(n), hipHostMallocDefault));
  if (!S->d_in) HIPCHK(c, dalloc(&S->d_in, shr_in_bytes(n)));
  if (!S->d_out) HIPCHK(c, dalloc(&S->d_out, shr_out_bytes(n)));
  if (!S->ev_done) HIPCHK(c, hipEventCreateWithFlags(&S->ev_done, hipEventDisableTiming));
  return 0;
}

// The error word of bridge_mix_kernel: all lyra_hip_bridge_mix_dev needs.
int brg_ensure_mix(lyra_hip_ctx* c) {
  if (!c->d_bridge_err) {
    HIPCHK(c, dalloc(&c->d_bridge_err, 1));
    HIPCHK(c, hipMemset(c->d_bridge_err, 0, 4));
  }
  return 0;
}

// The edge's event, the constants of the encode leg (every rate 16000, row b at sample 320 * b) and the tick's scratch: the mix and the comfort-noise flags of a call that was given none.  Two sets, picked by lossy-call parity
// as d_dstr16 is (and like it not what keeps call n + 1 off call n's set today: tick n + 1's noise-stream half waits for tick
// n's quantizer, which runs behind tick n's mix).
int brg_ensure(lyra_hip_ctx* c, int B) {
  int rc = brg_ensure_mix(c);
  if (rc) return rc;
  if (!c->ev_brg_mix) HIPCHK(c, hipEventCreateWithFlags(&c->ev_brg_mix, hipEventDisableTiming));
  if (!c->d_mixed_err) {   // (encode16 would allocate it on the way: everything up front)
    HIPCHK(c, dalloc(&c->d_mixed_err, 1));
    HIPCHK(c, hipMemset(c->d_mixed_err, 0, 4));
  }
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

int shr_encode_fanout(lyra_hip_ctx* c, const lyra_hip_bridge_tick* T, int max_speakers, int E, const ShrTick& sh,
                      const int16_t* enc_mix, const int32_t* slot_of, int set);

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
  rc = sh ? shr_mix_launch(c, pcm16, T->d_stream_ids, B, T->d_order, T->d_room_start, T->n_rooms, T->n_members, T->d_muted,
                           skip_cn ? is_cn : nullptr, max_speakers, *sh, mix, d_levels, d_is_speaker, slot_of, set)
       : max_speakers ? spk_mix_launch(c, pcm16, B, T->d_order, T->d_room_start, T->n_rooms, T->n_members, T->d_muted,
                                     skip_cn ? is_cn : nullptr, max_speakers, mix, d_levels, d_is_speaker, set)
                    : brg_mix_launch(c, pcm16, B, T->d_order, T->d_room_start, T->n_rooms, T->n_members, T->d_muted,
                                     skip_cn ? is_cn : nullptr, mix);
  if (rc) return rc;
  // ---- encode leg ----
  const int32_t* rates16 = c->d_brg_const;
  if (sh) return shr_encode_fanout(c, T, max_speakers, E, *sh, mix, slot_of, set);
  return lyra_hip_encode_streams_dev(c, T->d_stream_ids, B, mix, 320L * B, rates16 + c->max_streams, rates16, T->d_num_bits,
                                     T->d_dtx, T->d_out_packets, T->d_out_packet_bytes);
}

// begin() of both kinds of tick (max_speakers as in brg_tick_impl): one validation, one staging, one upload, one download
int brg_begin_impl(lyra_hip_ctx* c, const char* what, const int32_t* ids, int B, const uint8_t* packets,
                   const int32_t* packet_bytes, const int32_t* rooms, const int32_t* muted, unsigned flags,
                   const int32_t* num_bits, const int32_t* dtx, int max_speakers) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (!packets || !packet_bytes || !rooms || !num_bits) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  if (flags & ~LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE) return fail(c, LYRA_HIP_EINVAL, "%s: unknown flags 0x%x", what, flags);
  if ((rc = check_ids_host(c, ids, B))) return rc;
  for (int b = 0; b < B; ++b) {
    if ((rc = check_bits(c, num_bits[b]))) return rc;
    const int pb = packet_bytes[b];   // PacketSizeToNumQuantizedBits (lyra_config.h:99-106), 0: no packet on this tick
    if (pb != 0 && pb != 8 && pb != 15 && pb != LYRA_HIP_MAX_PACKET_BYTES)
      return fail(c, LYRA_HIP_EINVAL, "%s: packet of %d bytes at position %d (0, 8, 15 or 23)", what, pb, b);
  }
  if ((rc = brg_admit(c, what))) return rc;
  DEVSCOPE(c);
  if (!c->brg_host) c->brg_host = new BrgHost();
  BrgSlot& S = static_cast<BrgHost*>(c->brg_host)->slot[c->pl_begun[PL_BRIDGE] & 1];
  if ((rc = brg_slot_ensure(c, &S))) return rc;
  // (the slot's previous user, two ticks back, has ended: its kernels on every stream have read d_in, its download has left
  // d_out and h_out)
  const size_t n = (size_t)B;
  int32_t* h = reinterpret_cast<int32_t*>(S.h_in);
  int n_rooms = 0, n_members = 0;
  if (bridge::plan(rooms, B, h + 2 * n, h + 6 * n, &n_rooms, &n_members))
    return fail(c, LYRA_HIP_EINVAL, "%s: a room of more than %d members", what, LYRA_HIP_BRIDGE_MAX_ROOM);
  // everything the tick allocates or builds on first use, BEFORE anything is enqueued: a failure here leaves the streams idle
  if ((rc = ensure_scratch(c, B))) return rc;
  if ((rc = rates_ensure(c))) return rc;
  if ((rc = lossy_ensure(c, B))) return rc;
  if ((rc = dstr16_ensure(c, B))) return rc;
  if ((rc = brg_ensure(c, B))) return rc;
  if (max_speakers && (rc = spk_ensure(c, B))) return rc;
  for (int b = 0; b < B; ++b) {
    h[b] = ids[b];
    h[n + b] = packet_bytes[b];
    h[3 * n + b] = muted ? (muted[b] != 0) : 0;
    h[4 * n + b] = num_bits[b];
    h[5 * n + b] = dtx ? (dtx[b] != 0) : 0;
  }
  std::memcpy(S.h_in + (kBrgInArrays * n + 1) * 4, packets, n * LYRA_HIP_MAX_PACKET_BYTES);
  // one upload from pinned staging on the decode-side stream, in front of the tick's first kernel.  The encode leg reads ids,
  // bits and DTX flags on se[0] / sq[0]: both are behind the tick's edge, which is behind the decode-side half and so the copy.
  HIPCHK(c, hipMemcpyAsync(S.d_in, S.h_in, brg_in_bytes(n), hipMemcpyHostToDevice, c->sd[0]));
  const int32_t* m = reinterpret_cast<const int32_t*>(S.d_in);
  int32_t* o = reinterpret_cast<int32_t*>(S.d_out);
  const size_t out_words = max_speakers ? kSpkOutWords : 3;
  uint8_t* out_pk = S.d_out + out_words * n * 4;
  // empty packets, and the bytes behind a shorter one, read back as zeros; the extractor's stream is ahead of the quantizer's
  HIPCHK(c, hipMemsetAsync(out_pk, 0, n * LYRA_HIP_MAX_PACKET_BYTES, c->se[0]));
  lyra_hip_bridge_tick T = {};
  T.d_stream_ids = m;
  T.B = B;
  T.d_packets = S.d_in + (kBrgInArrays * n + 1) * 4;
  T.d_packet_bytes = m + n;
  T.d_order = m + 2 * n;
  T.d_room_start = m + 6 * n;
  T.n_rooms = n_rooms;
  T.n_members = n_members;
  T.d_muted = muted ? m + 3 * n : nullptr;
  T.flags = flags;
  T.d_num_bits = m + 4 * n;
  T.d_dtx = dtx ? m + 5 * n : nullptr;
  T.d_out_packets = out_pk;
  T.d_out_packet_bytes = o;
  T.d_is_noise = o + n;
  T.d_is_comfort_noise = o + 2 * n;
  // (a selection tick: is_speaker behind the three int32 arrays, then the levels, 8-byte aligned at 16 * n bytes)
  if ((rc = brg_tick_impl(c, what, &T, max_speakers, max_speakers ? reinterpret_cast<int64_t*>(o + 4 * n) : nullptr,
                          max_speakers ? o + 3 * n : nullptr)))
    return rc;
  // packets and sizes are written by the quantizer on sq[0], the flags by the noise-stream half: the one download rides on
  // sq[0] behind the end of that half (the quantizer itself is already enqueued and does not wait for it).  The levels and
  // speaker flags of a selection tick are written on se[0] by the mix's kernels: the quantizer on sq[0] waits for the
  // extractor's event on se[0] (encq_handoff, api.hip), which is enqueued behind them, so sq[0] is behind them as well.
  HIPCHK(c, hipStreamWaitEvent(c->sq[0], c->ev_noise[(c->n_noise_calls - 1) & 1], 0));
  HIPCHK(c, hipMemcpyAsync(S.h_out, S.d_out, out_words * n * 4 + n * LYRA_HIP_MAX_PACKET_BYTES, hipMemcpyDeviceToHost, c->sq[0]));
  HIPCHK(c, hipEventRecord(S.ev_done, c->sq[0]));
  S.B = B;
  S.max_speakers = max_speakers;
  S.shared = false;
  c->pl_begun[PL_BRIDGE]++;
  return 0;
}

}  // namespace

extern "C" {

int lyra_hip_bridge_plan(const int32_t* rooms, int B, int32_t* order, int32_t* room_start, int* n_rooms, int* n_members) {
  return bridge::plan(rooms, B, order, room_start, n_rooms, n_members) ? LYRA_HIP_EINVAL : 0;
}

int lyra_hip_bridge_mix_dev(lyra_hip_ctx* c, const int16_t* d_pcm16, int B, const int32_t* d_order, const int32_t* d_room_start,
                            int n_rooms, int n_members, const int32_t* d_muted, const int32_t* d_is_comfort_noise,
                            int16_t* d_mix) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (!d_pcm16 || !d_mix) return fail(c, LYRA_HIP_EINVAL, "bridge_mix: null pointer");
  if ((rc = brg_check_index(c, "bridge_mix", B, d_order, d_room_start, n_rooms, n_members))) return rc;
  if (brg_misaligned(d_pcm16) || brg_misaligned(d_mix) || d_pcm16 == d_mix)
    return fail(c, LYRA_HIP_EINVAL, "bridge_mix: d_pcm16 and d_mix must be 16-byte aligned and distinct");
  DEVSCOPE(c);
  if ((rc = brg_ensure_mix(c))) return rc;
  if ((rc = enc_side_begin(c, 0))) return rc;
  rc = brg_mix_launch(c, d_pcm16, B, d_order, d_room_start, n_rooms, n_members, d_muted, d_is_comfort_noise, d_mix);
  if (!rc) rc = enc_side_done(c, 0);
  return rc;
}

int lyra_hip_bridge_tick_dev(lyra_hip_ctx* c, const lyra_hip_bridge_tick* T) {
  if (!c) return LYRA_HIP_EINVAL;
  if (!T) return fail(c, LYRA_HIP_EINVAL, "bridge_tick: null pointer");
  return brg_tick_impl(c, "bridge_tick", T, 0, nullptr, nullptr);
}

int lyra_hip_bridge_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets, const int32_t* packet_bytes,
                          const int32_t* rooms, const int32_t* muted, unsigned flags, const int32_t* num_bits,
                          const int32_t* dtx) {
  if (!c) return LYRA_HIP_EINVAL;
  return brg_begin_impl(c, "bridge_begin", ids, B, packets, packet_bytes, rooms, muted, flags, num_bits, dtx, 0);
}

int lyra_hip_bridge_end(lyra_hip_ctx* c, uint8_t* out_packets, int32_t* out_packet_bytes, int32_t* is_noise,
                        int32_t* is_comfort_noise) {
  if (!c) return LYRA_HIP_EINVAL;
  if (!c->brg_host || c->pl_ended[PL_BRIDGE] == c->pl_begun[PL_BRIDGE]) return fail(c, LYRA_HIP_EINVAL, "bridge_end: no tick in flight");
  BrgSlot& S = static_cast<BrgHost*>(c->brg_host)->slot[c->pl_ended[PL_BRIDGE] & 1];
  if (S.max_speakers)
    return fail(c, LYRA_HIP_EINVAL, "bridge_end: the oldest tick was begun by lyra_hip_%s_begin", S.shared ? "shared" : "speakers");
  if (!out_packets || !out_packet_bytes) return fail(c, LYRA_HIP_EINVAL, "bridge_end: null pointer");
  DEVSCOPE(c);
  c->pl_ended[PL_BRIDGE]++;                  // whatever happens below, the slot is given back
  HIPCHK(c, hipEventSynchronize(S.ev_done));
  const size_t n = (size_t)S.B;
  std::memcpy(out_packet_bytes, S.h_out, n * 4);
  if (is_noise) std::memcpy(is_noise, S.h_out + n * 4, n * 4);
  if (is_comfort_noise) std::memcpy(is_comfort_noise, S.h_out + 2 * n * 4, n * 4);
  std::memcpy(out_packets, S.h_out + 3 * n * 4, n * LYRA_HIP_MAX_PACKET_BYTES);
  return 0;
}

long lyra_hip_bridge_errors(lyra_hip_ctx* c, int clear) {
  return read_error_counter(c, &lyra_hip_ctx::d_bridge_err, clear);
}

}  // extern "C"
