// shared_bridge_api.inc -- part of api.hip, behind speakers_api.inc: the loudest-N bridge with shared encoders
// (include/lyra_hip_shared_bridge.h).  The tick is brg_tick_impl (bridge_api.inc) with a ShrTick: the decode leg, the edge, the
// allocations and the refusals are the bridge's own; what is new here is the mix on se[0] -- speakers_level_kernel and
// speakers_select_kernel as they are, then shared_slots_kernel and shared_mix_kernel (shared_bridge_kernels.hip) -- the encode
// leg on E = n_rooms * (1 + max_speakers) rows instead of B, the fan-out on sq[0] behind the quantizer, the scratch of all
// that, and a begin() / end() of its own on the bridge's two slots and counters.
#include "../../include/lyra_hip_shared_bridge.h"
#include "shared_bridge_plan.h"

static_assert(LYRA_HIP_SHARED_SLOTS == LYRA_HIP_SPEAKERS_MAX, "a table row is as wide as a speaker list");

namespace {

void shr_free_bufs(lyra_hip_ctx* c) {
  for (int i = 0; i < 2; ++i)
    dfree(c->d_shr_slot_row[i], c->d_shr_row_room[i], c->d_shr_slot_of[i], c->d_shr_mix[i], c->d_shr_pk[i], c->d_shr_len[i]);
  c->shr_cap = 0;
}
void shr_free(lyra_hip_ctx* c) {
  shr_free_bufs(c);
  dfree(c->d_shr_table);
}

// rows = max(B, E) of the tick: slot_row [n_rooms][8] (n_rooms <= B), row_room and slot_of [B], the encoder mixes, packets
// and sizes [E].  Two sets by lossy-call parity, like d_brg_mix; called before anything is enqueued.
int shr_ensure(lyra_hip_ctx* c, int rows) {
  if (rows <= c->shr_cap) return 0;
  int rc = sync_all(c);   // (the buffers of the calls in flight)
  if (rc) return rc;
  shr_free_bufs(c);
  for (int i = 0; i < 2; ++i) {
    HIPCHK(c, dalloc(&c->d_shr_slot_row[i], (size_t)rows * LYRA_HIP_SHARED_SLOTS));
    HIPCHK(c, dalloc(&c->d_shr_row_room[i], (size_t)rows));
    HIPCHK(c, dalloc(&c->d_shr_slot_of[i], (size_t)rows));
    HIPCHK(c, dalloc(&c->d_shr_mix[i], (size_t)rows * 320));
    HIPCHK(c, dalloc(&c->d_shr_pk[i], (size_t)rows * LYRA_HIP_MAX_PACKET_BYTES));
    HIPCHK(c, dalloc(&c->d_shr_len[i], (size_t)rows));
  }
  c->shr_cap = rows;
  return 0;
}

// levels over all B rows (which also clears the flags, pos_room, slot_of and row_room; there is no per-listener mix to
// clear), one wavefront per room for the selection and again for the slots, then one per encoder row; on se[0].
// spk_ensure(c, B) and shr_ensure(c, max(B, E)) have run.  A tick without members still has its E rows: they hear zeros.
int shr_mix_launch(lyra_hip_ctx* c, const int16_t* d_pcm16, const int32_t* d_stream_ids, int B, const int32_t* d_order,
                   const int32_t* d_room_start, int n_rooms, int n_members, const int32_t* d_muted, const int32_t* d_is_cn,
                   int max_speakers, const ShrTick& sh, int16_t* d_enc_mix, int64_t* d_levels, int32_t* d_is_speaker,
                   int32_t* d_slot_of, int set) {
  long long* levels = reinterpret_cast<long long*>(d_levels ? d_levels : c->d_spk_levels[set]);
  int32_t* flags = d_is_speaker ? d_is_speaker : c->d_spk_flags[set];
  int32_t* pos_room = c->d_spk_pos_room[set];
  hipLaunchKernelGGL(speakers_level_kernel, dim3(cdiv(B, 4)), dim3(256), 0, c->se[0], d_pcm16, B, levels, (int16_t*)nullptr, flags,
                     pos_room, n_members, d_slot_of, c->d_shr_row_room[set]);
  HIPCHK(c, hipGetLastError());
  if (n_rooms <= 0) return 0;
  hipLaunchKernelGGL(speakers_select_kernel, dim3(cdiv(n_rooms, 4)), dim3(256), 0, c->se[0], levels, B, d_order, d_room_start,
                     n_rooms, n_members, d_muted, d_is_cn, max_speakers, c->d_spk_keys[set], c->d_spk_list[set], pos_room, flags,
                     c->d_bridge_err);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(shared_slots_kernel, dim3(cdiv(n_rooms, 4)), dim3(256), 0, c->se[0], c->d_spk_list[set], d_stream_ids, B,
                     d_order, d_room_start, n_rooms, n_members, max_speakers, sh.d_room_keys, sh.n_table_rooms, sh.d_slots,
                     c->d_shr_slot_row[set], d_slot_of, c->d_shr_row_room[set], c->d_bridge_err);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(shared_mix_kernel, dim3(cdiv(n_rooms * (1 + max_speakers), 4)), dim3(256), 0, c->se[0], d_pcm16, B, n_rooms,
                     max_speakers, c->d_spk_list[set], c->d_shr_slot_row[set], sh.d_room_keys, sh.n_table_rooms, d_enc_mix);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int shr_fanout_launch(lyra_hip_ctx* c, hipStream_t st, const lyra_hip_bridge_tick* T, int max_speakers, const int32_t* slot_of,
                      const uint8_t* pk, const int32_t* len, int set) {
  hipLaunchKernelGGL(shared_fanout_kernel, dim3(cdiv(T->B * (LYRA_HIP_MAX_PACKET_BYTES + 1), 256)), dim3(256), 0, st, T->B,
                     T->n_rooms, max_speakers, c->d_shr_row_room[set], slot_of, pk, len, T->d_out_packets, T->d_out_packet_bytes);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// The encode leg and the fan-out of a shared-encoder tick, behind shr_mix_launch (brg_tick_impl).
int shr_encode_fanout(lyra_hip_ctx* c, const lyra_hip_bridge_tick* T, int max_speakers, int E, const ShrTick& sh,
                      const int16_t* enc_mix, const int32_t* slot_of, int set) {
  uint8_t* pk = sh.d_enc_packets ? sh.d_enc_packets : c->d_shr_pk[set];
  int32_t* len = sh.d_enc_packet_bytes ? sh.d_enc_packet_bytes : c->d_shr_len[set];
  if (E == 0) {   // no room, no encoder row: an empty packet for everybody, on se[0] behind the level kernel; an encode-side call
    int rc = shr_fanout_launch(c, c->se[0], T, max_speakers, slot_of, pk, len, set);
    return rc ? rc : enc_side_done(c, 0);
  }
  // the library's own packet rows read as zeros behind a packet's bytes; the extractor's stream is ahead of the quantizer's
  if (!sh.d_enc_packets) HIPCHK(c, hipMemsetAsync(pk, 0, (size_t)E * LYRA_HIP_MAX_PACKET_BYTES, c->se[0]));
  const int32_t* rates16 = c->d_brg_const;
  int rc = lyra_hip_encode_streams_dev(c, sh.d_enc_stream_ids, E, enc_mix, 320L * E, rates16 + c->max_streams, rates16,
                                       sh.d_enc_num_bits, sh.d_enc_dtx, pk, len);
  if (rc) return rc;
  // sq[0], behind the quantizer that wrote pk / len; slot_of and row_room were written on se[0] in front of the extractor, whose
  // event the quantizer waited for.  The quantizer's event is recorded again behind the fan-out: whoever waits for "the latest
  // quantizer" from here on (wait_encode_side) waits for the outgoing packets and for the last reader of this set's scratch.
  if ((rc = shr_fanout_launch(c, c->sq[0], T, max_speakers, slot_of, pk, len, set))) return rc;
  HIPCHK(c, hipEventRecord(c->ev_encs[c->sq_slot[0]][0], c->sq[0]));
  return 0;
}

}  // namespace

extern "C" {

int lyra_hip_shared_mix_dev(lyra_hip_ctx* c, const int16_t* d_pcm16, const int32_t* d_stream_ids, int B, const int32_t* d_order,
                            const int32_t* d_room_start, int n_rooms, int n_members, const int32_t* d_muted,
                            const int32_t* d_is_comfort_noise, int max_speakers, const int32_t* d_room_keys, int32_t* d_slots,
                            int n_table_rooms, int16_t* d_enc_mix, int64_t* d_levels, int32_t* d_is_speaker, int32_t* d_slot_of) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (!d_pcm16 || !d_stream_ids || !d_slots || !d_enc_mix) return fail(c, LYRA_HIP_EINVAL, "shared_mix: null pointer");
  if ((rc = brg_check_index(c, "shared_mix", B, d_order, d_room_start, n_rooms, n_members))) return rc;
  if (brg_misaligned(d_pcm16) || brg_misaligned(d_enc_mix) || d_pcm16 == d_enc_mix)
    return fail(c, LYRA_HIP_EINVAL, "shared_mix: d_pcm16 and d_enc_mix must be 16-byte aligned and distinct");
  if ((reinterpret_cast<uintptr_t>(d_levels) & 7u) != 0) return fail(c, LYRA_HIP_EINVAL, "shared_mix: d_levels must be 8-byte aligned");
  if ((rc = spk_check_n(c, "shared_mix", max_speakers))) return rc;
  if (n_table_rooms < 1) return fail(c, LYRA_HIP_EINVAL, "shared_mix: n_table_rooms %d", n_table_rooms);
  DEVSCOPE(c);
  if ((rc = brg_ensure_mix(c))) return rc;
  if ((rc = spk_ensure(c, B))) return rc;
  if ((rc = shr_ensure(c, B))) return rc;   // (the encoder mixes are the caller's: the scratch is sized by B alone)
  if ((rc = enc_side_begin(c, 0))) return rc;
  const int set = (int)(c->n_lossy_calls & 1);
  ShrTick sh = {};
  sh.d_room_keys = d_room_keys;
  sh.d_slots = d_slots;
  sh.n_table_rooms = n_table_rooms;
  rc = shr_mix_launch(c, d_pcm16, d_stream_ids, B, d_order, d_room_start, n_rooms, n_members, d_muted, d_is_comfort_noise,
                      max_speakers, sh, d_enc_mix, d_levels, d_is_speaker, d_slot_of ? d_slot_of : c->d_shr_slot_of[set], set);
  if (!rc) rc = enc_side_done(c, 0);
  return rc;
}

int lyra_hip_shared_tick_dev(lyra_hip_ctx* c, const lyra_hip_shared_tick* S) {
  if (!c) return LYRA_HIP_EINVAL;
  if (!S) return fail(c, LYRA_HIP_EINVAL, "shared_tick: null pointer");
  int rc = spk_check_n(c, "shared_tick", S->max_speakers);
  if (rc) return rc;
  if ((reinterpret_cast<uintptr_t>(S->d_levels) & 7u) != 0)
    return fail(c, LYRA_HIP_EINVAL, "shared_tick: d_levels must be 8-byte aligned");
  lyra_hip_bridge_tick T = {};   // the fields the three kinds of tick have in common, one by one
  T.d_stream_ids = S->d_stream_ids;
  T.B = S->B;
  T.d_packets = S->d_packets;
  T.d_packet_bytes = S->d_packet_bytes;
  T.d_order = S->d_order;
  T.d_room_start = S->d_room_start;
  T.n_rooms = S->n_rooms;
  T.n_members = S->n_members;
  T.d_muted = S->d_muted;
  T.flags = S->flags;
  T.d_out_packets = S->d_out_packets;
  T.d_out_packet_bytes = S->d_out_packet_bytes;
  T.d_pcm16 = S->d_pcm16;
  T.d_is_noise = S->d_is_noise;
  T.d_is_comfort_noise = S->d_is_comfort_noise;
  const ShrTick sh = {S->d_room_keys, S->d_slots, S->n_table_rooms, S->d_enc_stream_ids, S->d_enc_num_bits, S->d_enc_dtx,
                      S->d_enc_mix, S->d_enc_packets, S->d_enc_packet_bytes, S->d_slot_of};
  return brg_tick_impl(c, "shared_tick", &T, S->max_speakers, S->d_levels, S->d_is_speaker, &sh);
}

int lyra_hip_shared_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets, const int32_t* packet_bytes,
                          const int32_t* rooms, const int32_t* muted, unsigned flags, int max_speakers, const int32_t* room_labels,
                          int n_rooms, const int32_t* enc_ids, const int32_t* enc_bits, const int32_t* enc_dtx) {
  const char* what = "shared_begin";
  if (!c) return LYRA_HIP_EINVAL;
  int rc = spk_check_n(c, what, max_speakers);
  if (rc) return rc;
  if ((rc = check_batch(c, B))) return rc;
  if (!packets || !packet_bytes || !rooms || (n_rooms > 0 && (!room_labels || !enc_ids || !enc_bits)))
    return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  if (flags & ~LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE) return fail(c, LYRA_HIP_EINVAL, "%s: unknown flags 0x%x", what, flags);
  if (n_rooms < 0 || n_rooms > B) return fail(c, LYRA_HIP_EINVAL, "%s: n_rooms %d outside 0..B (%d)", what, n_rooms, B);
  const int E = n_rooms * (1 + max_speakers);
  if (E > c->max_streams)
    return fail(c, LYRA_HIP_EINVAL, "%s: %d rooms x (1 + %d) encoder rows exceed max_streams (%d): use the loudest-N tick", what,
                n_rooms, max_speakers, c->max_streams);
  if (E > 0 && (rc = check_ids_host(c, enc_ids, E))) return rc;
  if ((rc = check_ids_host(c, ids, B))) return rc;
  for (int e = 0; e < E; ++e)
    if ((rc = check_bits(c, enc_bits[e]))) return rc;
  for (int b = 0; b < B; ++b) {
    const int pb = packet_bytes[b];
    if (pb != 0 && pb != 8 && pb != 15 && pb != LYRA_HIP_MAX_PACKET_BYTES)
      return fail(c, LYRA_HIP_EINVAL, "%s: packet of %d bytes at position %d (0, 8, 15 or 23)", what, pb, b);
  }
  if ((rc = brg_admit(c, what))) return rc;
  DEVSCOPE(c);
  if (!c->brg_host) c->brg_host = new BrgHost();
  BrgSlot& S = static_cast<BrgHost*>(c->brg_host)->slot[c->pl_begun[PL_BRIDGE] & 1];
  if ((rc = brg_slot_ensure(c, &S))) return rc;
  // (the slot's previous user, two ticks back, has ended)  going up, int32: ids | packet_bytes | order | muted [B] each,
  // room_start [B + 1], room keys [B], enc_ids | enc_bits | enc_dtx [E] each, then the packets
  const size_t n = (size_t)B, ne = (size_t)E, w_keys = 5 * n + 1, w_enc = 6 * n + 1, w_end = w_enc + 3 * ne;
  int32_t* h = reinterpret_cast<int32_t*>(S.h_in);
  int planned = 0, n_members = 0;
  if (bridge::plan(rooms, B, h + 2 * n, h + 4 * n, &planned, &n_members))
    return fail(c, LYRA_HIP_EINVAL, "%s: a room of more than %d members", what, LYRA_HIP_BRIDGE_MAX_ROOM);
  int at = -1;
  if (const int bad = shared_bridge::check_labels(rooms, h + 2 * n, h + 4 * n, planned, room_labels, n_rooms, c->max_streams, &at))
    return fail(c, LYRA_HIP_EINVAL, "%s: room_labels (%d given, %d rooms present; position %d, code %d) must be the labels "
                "present in rooms, strictly ascending and below max_streams (%d)", what, n_rooms, planned, at, bad, c->max_streams);
  // everything the tick allocates or builds on first use, BEFORE anything is enqueued: a failure here leaves the streams idle
  if ((rc = ensure_scratch(c, std::max(B, E)))) return rc;
  if ((rc = rates_ensure(c))) return rc;
  if ((rc = lossy_ensure(c, B))) return rc;
  if ((rc = dstr16_ensure(c, B))) return rc;
  if ((rc = brg_ensure(c, B))) return rc;
  if ((rc = spk_ensure(c, B))) return rc;
  if ((rc = shr_ensure(c, std::max(B, E)))) return rc;
  if (!c->d_shr_table) {   // one row per label below max_streams, all free
    HIPCHK(c, dalloc(&c->d_shr_table, (size_t)c->max_streams * LYRA_HIP_SHARED_SLOTS));
    HIPCHK(c, hipMemset(c->d_shr_table, 0xFF, (size_t)c->max_streams * LYRA_HIP_SHARED_SLOTS * 4));
  }
  for (int b = 0; b < B; ++b) {
    h[b] = ids[b];
    h[n + b] = packet_bytes[b];
    h[3 * n + b] = muted ? (muted[b] != 0) : 0;
  }
  for (int r = 0; r < n_rooms; ++r) h[w_keys + r] = room_labels[r];
  for (int e = 0; e < E; ++e) {
    h[w_enc + e] = enc_ids[e];
    h[w_enc + ne + e] = enc_bits[e];
    h[w_enc + 2 * ne + e] = enc_dtx ? (enc_dtx[e] != 0) : 0;
  }
  std::memcpy(S.h_in + w_end * 4, packets, n * LYRA_HIP_MAX_PACKET_BYTES);
  // one upload on the decode-side stream in front of the tick's first kernel; se[0] / sq[0] read theirs behind the tick's edge
  HIPCHK(c, hipMemcpyAsync(S.d_in, S.h_in, w_end * 4 + n * LYRA_HIP_MAX_PACKET_BYTES, hipMemcpyHostToDevice, c->sd[0]));
  const int32_t* m = reinterpret_cast<const int32_t*>(S.d_in);
  // coming down: [out_packet_bytes | is_noise | is_comfort_noise | is_speaker] int32, levels int64 (at 16 * n bytes), slot_of
  // int32, then the packets -- every byte of them is written by the fan-out
  int32_t* o = reinterpret_cast<int32_t*>(S.d_out);
  lyra_hip_bridge_tick T = {};
  T.d_stream_ids = m;
  T.B = B;
  T.d_packets = S.d_in + w_end * 4;
  T.d_packet_bytes = m + n;
  T.d_order = m + 2 * n;
  T.d_room_start = m + 4 * n;
  T.n_rooms = n_rooms;
  T.n_members = n_members;
  T.d_muted = muted ? m + 3 * n : nullptr;
  T.flags = flags;
  T.d_out_packets = S.d_out + kShrOutWords * n * 4;
  T.d_out_packet_bytes = o;
  T.d_is_noise = o + n;
  T.d_is_comfort_noise = o + 2 * n;
  ShrTick sh = {};
  sh.d_room_keys = m + w_keys;
  sh.d_slots = c->d_shr_table;
  sh.n_table_rooms = c->max_streams;
  sh.d_enc_stream_ids = m + w_enc;
  sh.d_enc_num_bits = m + w_enc + ne;
  sh.d_enc_dtx = enc_dtx ? m + w_enc + 2 * ne : nullptr;
  sh.d_slot_of = o + 6 * n;
  if ((rc = brg_tick_impl(c, what, &T, max_speakers, reinterpret_cast<int64_t*>(o + 4 * n), o + 3 * n, &sh))) return rc;
  // The one download rides on sq[0] behind the fan-out (packets, sizes) and behind the end of the noise-stream half (the noise
  // flags).  Levels, speaker flags and slot_of were written on se[0] in front of the extractor, which the quantizer waited for;
  // a tick without rooms has no quantizer and ends on se[0] instead.
  HIPCHK(c, hipStreamWaitEvent(c->sq[0], c->ev_noise[(c->n_noise_calls - 1) & 1], 0));
  if (E == 0) HIPCHK(c, hipStreamWaitEvent(c->sq[0], c->ev_encs[2][0], 0));
  HIPCHK(c, hipMemcpyAsync(S.h_out, S.d_out, shr_out_bytes(n), hipMemcpyDeviceToHost, c->sq[0]));
  HIPCHK(c, hipEventRecord(S.ev_done, c->sq[0]));
  S.B = B;
  S.max_speakers = max_speakers;
  S.shared = true;
  c->pl_begun[PL_BRIDGE]++;
  return 0;
}

int lyra_hip_shared_end(lyra_hip_ctx* c, uint8_t* out_packets, int32_t* out_packet_bytes, int32_t* is_noise,
                        int32_t* is_comfort_noise, int64_t* levels, int32_t* is_speaker, int32_t* slot_of) {
  if (!c) return LYRA_HIP_EINVAL;
  if (!c->brg_host || c->pl_ended[PL_BRIDGE] == c->pl_begun[PL_BRIDGE]) return fail(c, LYRA_HIP_EINVAL, "shared_end: no tick in flight");
  BrgSlot& S = static_cast<BrgHost*>(c->brg_host)->slot[c->pl_ended[PL_BRIDGE] & 1];
  if (!S.shared)
    return fail(c, LYRA_HIP_EINVAL, "shared_end: the oldest tick was begun by %s", S.max_speakers ? "lyra_hip_speakers_begin" : "the full-mix begin()");
  if (!out_packets || !out_packet_bytes) return fail(c, LYRA_HIP_EINVAL, "shared_end: null pointer");
  DEVSCOPE(c);
  c->pl_ended[PL_BRIDGE]++;                  // whatever happens below, the slot is given back
  HIPCHK(c, hipEventSynchronize(S.ev_done));
  const size_t n = (size_t)S.B;
  std::memcpy(out_packet_bytes, S.h_out, n * 4);
  if (is_noise) std::memcpy(is_noise, S.h_out + n * 4, n * 4);
  if (is_comfort_noise) std::memcpy(is_comfort_noise, S.h_out + 2 * n * 4, n * 4);
  if (is_speaker) std::memcpy(is_speaker, S.h_out + 3 * n * 4, n * 4);
  if (levels) std::memcpy(levels, S.h_out + 4 * n * 4, n * 8);
  if (slot_of) std::memcpy(slot_of, S.h_out + 6 * n * 4, n * 4);
  std::memcpy(out_packets, S.h_out + kShrOutWords * n * 4, n * LYRA_HIP_MAX_PACKET_BYTES);
  return 0;
}

int lyra_hip_shared_reset_rooms(lyra_hip_ctx* c, const int32_t* room_labels, int n) {
  if (!c) return LYRA_HIP_EINVAL;
  if (n < 0 || (n > 0 && !room_labels)) return fail(c, LYRA_HIP_EINVAL, "shared_reset_rooms: bad argument");
  for (int i = 0; i < n; ++i)
    if (room_labels[i] < 0 || room_labels[i] >= c->max_streams)
      return fail(c, LYRA_HIP_EINVAL, "shared_reset_rooms: label %d at position %d outside 0..%d", room_labels[i], i, c->max_streams - 1);
  DEVSCOPE(c);
  int rc = sync_all(c);   // the table is read and written by the ticks in flight
  if (rc) return rc;
  if (!c->d_shr_table) return 0;
  for (int i = 0; i < n; ++i)
    HIPCHK(c, hipMemset(c->d_shr_table + (size_t)room_labels[i] * LYRA_HIP_SHARED_SLOTS, 0xFF, LYRA_HIP_SHARED_SLOTS * 4));
  return 0;
}

}  // extern "C"
