// shared_bridge_api.inc -- part of api.hip, behind speakers_api.inc and in front of bridge_api.inc: the loudest-N bridge with
// shared encoders (include/lyra_hip_shared_bridge.h).  The tick is brg_tick_impl (bridge_api.inc) with a ShrTick: the decode leg,
// the edge, the allocations, the refusals, begin() / end() and the entry points are the bridge's own; what is here is the mix on
// se[0] -- speakers_level_kernel and speakers_select_kernel as they are, then shared_slots_kernel and shared_mix_kernel
// (shared_bridge_kernels.hip) -- the encode leg on E = n_rooms * (1 + max_speakers) rows instead of B, the fan-out on sq[0]
// behind the quantizer, the scratch of all that, and the slot table's reset.
#include "../../include/lyra_hip_bridge.h"
#include "../../include/lyra_hip_shared_bridge.h"
#include "shared_bridge_plan.h"

static_assert(LYRA_HIP_SHARED_SLOTS == LYRA_HIP_SPEAKERS_MAX, "a table row is as wide as a speaker list");

namespace {

// what a shared-encoder tick has in place of the per-listener bit counts, DTX flags and mix
struct ShrTick {
  const int32_t* d_room_keys;
  int32_t* d_slots;
  int n_table_rooms;
  const int32_t *d_enc_stream_ids, *d_enc_num_bits, *d_enc_dtx;
  int16_t* d_enc_mix;
  uint8_t* d_enc_packets;
  int32_t *d_enc_packet_bytes, *d_slot_of;
};

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
