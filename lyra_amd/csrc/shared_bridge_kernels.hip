// shared_bridge_kernels.hip -- shared encoders for the loudest-N bridge (include/lyra_hip_shared_bridge.h,
// shared_bridge_api.inc): a room with max_speakers = N has 1 + N distinct mixes, so the tick encodes E = n_rooms * (1 + N)
// rows -- the room's common mix and one mix-minus per speaker slot -- and copies the packets to the participants.  Behind
// speakers_level_kernel and speakers_select_kernel (speakers_kernels.hip), which stay as they are:
//   shared_slots_kernel   one wavefront per room: at most 8 x 8 id compares between the room's row of the slot table and the
//                         stream ids of its speaker list; the table row, the speaker row of every slot, slot_of of the
//                         speakers, and the room of every member row (so that the fan-out needs no search);
//   shared_mix_kernel     parallel over ENCODER ROWS, not rooms: one wavefront sums the <= 8 speaker rows (L2 hits) and takes
//                         at most one out, so a room of any size is 1 + N wavefronts of work;
//   shared_fanout_kernel  over the participants, one thread per outgoing byte; on the quantizer stream behind the quantizer.
// Integer arithmetic only; no LDS, no scratch, no atomics on audio.  The index, the keys and the table are the caller's and are
// not trusted: room_start is clamped, every order[] entry, key, row number and slot that went through memory is checked against
// its range where it is read, before it addresses anything.
#include "kernels.h"
#include "speakers_rows.h"   // SPK_MAX, SPK_LANES, SpkAcc, spk_add, spk_minus

namespace lyra {

namespace {

constexpr int PKT = 23;   // LYRA_HIP_MAX_PACKET_BYTES

}  // namespace

// One wavefront per room, four rooms per workgroup.  Lane k < N holds speaker k of the room (row and stream id, selection
// order), lane j < 8 the old content of slot j.  Rule 1: slot j < N is kept if its id is a speaker's and no lower slot holds
// the same id (shuffles, 8 + 8 compares per lane).  Rule 2: the speakers whose id no kept slot holds take the free slots below
// N, both in ascending order -- the q-th of one gets the q-th of the other, ranks by popcount over two ballots.  Rule 3: what
// is neither kept nor taken, every slot >= N included, becomes -1.  A stream id < 0 cannot be told from "free": such a
// speaker holds no slot.  A key outside the table: counted once, the table untouched, the members stay in "no room".
__global__ __launch_bounds__(256) void shared_slots_kernel(const int32_t* __restrict__ spk, const int32_t* __restrict__ stream_ids,
                                                            int B, const int32_t* __restrict__ order,
                                                            const int32_t* __restrict__ room_start, int n_rooms, int n_members,
                                                            int max_speakers, const int32_t* __restrict__ room_keys,
                                                            int n_table_rooms, int32_t* slots, int32_t* __restrict__ slot_row,
                                                            int32_t* __restrict__ slot_of, int32_t* __restrict__ row_room,
                                                            unsigned* __restrict__ err) {
  const int lane = threadIdx.x & 63, room = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (room >= n_rooms) return;
  const int key = room_keys ? room_keys[room] : room;
  if (key < 0 || key >= n_table_rooms) {
    if (lane < SPK_MAX) slot_row[(size_t)room * SPK_MAX + lane] = -1;
    if (lane == 0) atomicAdd(err, 1u);
    return;
  }
  int s_row = -1, s_id = -1, old = -1;
  if (lane < SPK_MAX) {
    old = slots[(size_t)key * SPK_MAX + lane];
    const int r = lane < max_speakers ? spk[(size_t)room * SPK_MAX + lane] : -1;
    if (r >= 0 && r < B) {
      s_id = stream_ids[r];
      s_row = s_id >= 0 ? r : -1;
    }
  }
  // rule 1
  bool kept = false;
  int row = -1;
#pragma unroll
  for (int k = 0; k < SPK_MAX; ++k) {
    const int id_k = __shfl(s_id, k), row_k = __shfl(s_row, k);
    if (!kept && old >= 0 && row_k >= 0 && id_k == old) {
      kept = true;
      row = row_k;
    }
  }
#pragma unroll
  for (int j = 0; j < SPK_MAX; ++j) {
    const int o = __shfl(old, j);
    if (j < lane && o == old) kept = false;
  }
  kept = kept && lane < max_speakers;
  const unsigned kept_mask = (unsigned)__ballot(kept) & 0xffu;
  // rule 2
  bool placed = false;
#pragma unroll
  for (int j = 0; j < SPK_MAX; ++j) {
    const int o = __shfl(old, j);
    if (((kept_mask >> j) & 1u) && o == s_id) placed = true;
  }
  const bool is_free = lane < max_speakers && !kept;
  const unsigned wants = (unsigned)__ballot(s_row >= 0 && !placed) & 0xffu, frees = (unsigned)__ballot(is_free) & 0xffu;
  const int my_rank = is_free ? __popc(frees & ((1u << lane) - 1u)) : -1;
  int id = kept ? old : -1;
  row = kept ? row : -1;
#pragma unroll
  for (int k = 0; k < SPK_MAX; ++k) {
    const int id_k = __shfl(s_id, k), row_k = __shfl(s_row, k);
    if (is_free && ((wants >> k) & 1u) && __popc(wants & ((1u << k) - 1u)) == my_rank) {
      id = id_k;
      row = row_k;
    }
  }
  if (lane < SPK_MAX) {
    slots[(size_t)key * SPK_MAX + lane] = id;              // (rule 3: -1 for every slot >= max_speakers)
    slot_row[(size_t)room * SPK_MAX + lane] = row;
    if (row >= 0) slot_of[row] = lane;                     // (row < B: checked where it was read from the list)
  }
  // the room of every member row, for the fan-out
  int lo = room_start[room], hi = room_start[room + 1];
  lo = lo < 0 ? 0 : lo > n_members ? n_members : lo;
  hi = hi < lo ? lo : hi > n_members ? n_members : hi;
  for (int p = lo + lane; p < hi; p += 64) {
    const int r = order[p];
    if (r >= 0 && r < B) row_room[r] = room;
  }
}

// One wavefront per encoder row, four per workgroup; lanes 0..39 own 16 bytes of the 640-byte row, as in speakers_mix_kernel:
// always a load from inside the buffer (row 0 in place of a missing row), masked afterwards, so the nine requests go out back
// to back.  Row e = room * (1 + N) + c: c = 0 hears clamp(S), c > 0 hears clamp(S - x of the row in slot c - 1), a free slot
// clamp(S).  A room whose key is outside the table hears zeros.
__global__ __launch_bounds__(256) void shared_mix_kernel(const int16_t* __restrict__ pcm, int B, int n_rooms, int max_speakers,
                                                          const int32_t* __restrict__ spk, const int32_t* __restrict__ slot_row,
                                                          const int32_t* __restrict__ room_keys, int n_table_rooms,
                                                          int16_t* __restrict__ enc_mix) {
  const int lane = threadIdx.x & 63, e = blockIdx.x * 4 + (threadIdx.x >> 6), per = 1 + max_speakers;
  if (e >= n_rooms * per) return;
  const int room = e / per, c = e - room * per;
  const bool owner = lane < SPK_LANES;
  const int slice = owner ? lane : SPK_LANES - 1;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  const int key = room_keys ? room_keys[room] : room;
  const bool live = key >= 0 && key < n_table_rooms;
  int my_spk = -1, minus = -1;
  if (live && lane < SPK_MAX) {
    const int s = spk[(size_t)room * SPK_MAX + lane];
    if (s >= 0 && s < B) my_spk = s;
  }
  if (live && c > 0) {
    const int m = slot_row[(size_t)room * SPK_MAX + c - 1];
    if (m >= 0 && m < B) minus = m;
  }
  uint4 y[SPK_MAX];
#pragma unroll
  for (int k = 0; k < SPK_MAX; ++k) {
    const int s = __shfl(my_spk, k);
    const uint4 v = reinterpret_cast<const uint4*>(pcm + (size_t)(s >= 0 ? s : 0) * 320)[slice];
    y[k] = (owner && s >= 0) ? v : zero4;
  }
  const uint4 x = reinterpret_cast<const uint4*>(pcm + (size_t)(minus >= 0 ? minus : 0) * 320)[slice];
  SpkAcc S;
#pragma unroll
  for (int i = 0; i < 8; ++i) S.v[i] = 0;
#pragma unroll
  for (int k = 0; k < SPK_MAX; ++k) spk_add(S, y[k]);
  if (owner) reinterpret_cast<uint4*>(enc_mix + (size_t)e * 320)[lane] = spk_minus(S, x, minus >= 0);
}

// One thread per byte: thread 24 * b + k copies byte k < 23 of the packet of row b, thread 24 * b + 23 its size.  Row b of room
// r takes encoder row r * (1 + N) + 1 + slot_of[b] if it holds a slot, r * (1 + N) otherwise; a row in no room (row_room < 0:
// never named by the index, or the room's key was bad) gets zeros and size 0.
__global__ __launch_bounds__(256) void shared_fanout_kernel(int B, int n_rooms, int max_speakers,
                                                             const int32_t* __restrict__ row_room,
                                                             const int32_t* __restrict__ slot_of,
                                                             const uint8_t* __restrict__ enc_packets,
                                                             const int32_t* __restrict__ enc_packet_bytes,
                                                             uint8_t* __restrict__ out_packets,
                                                             int32_t* __restrict__ out_packet_bytes) {
  const int t = blockIdx.x * 256 + threadIdx.x, b = t / (PKT + 1), k = t - b * (PKT + 1);
  if (b >= B) return;
  const int room = row_room[b];
  long e = -1;
  if (room >= 0 && room < n_rooms) {
    const int s = slot_of[b];
    e = (long)room * (1 + max_speakers) + (s >= 0 && s < max_speakers ? 1 + s : 0);
  }
  if (k == PKT) out_packet_bytes[b] = e >= 0 ? enc_packet_bytes[e] : 0;
  else out_packets[(size_t)b * PKT + k] = e >= 0 ? enc_packets[(size_t)e * PKT + k] : (uint8_t)0;
}

}  // namespace lyra
