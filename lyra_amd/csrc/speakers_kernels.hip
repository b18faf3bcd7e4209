// speakers_kernels.hip -- the loudest-N mix of a conference bridge (include/lyra_hip_speakers.h, speakers_api.inc): every
// participant hears the clamped sum of the max_speakers loudest sources of its room, itself left out.  Integer arithmetic only:
// level_b = sum of squares of row b in 64 bits; a room's speakers are its candidates (valid index entry, a source, level > 0)
// with the largest level, the earlier position winning a tie; S_r = the int32 sum of the speakers' rows;
// y_b = clamp(S_r - (speaker_b ? x_b : 0)).  Three kernels on one stream:
//   speakers_level_kernel   every row of the batch: its level, and the row's mix / is_speaker / pos_room entries cleared;
//   speakers_select_kernel  one wavefront per room over levels and the index only (no audio): the speaker list of the room,
//                           is_speaker, and the room number of every position, so that the mix needs no search;
//   speakers_mix_kernel     parallel over the POSITIONS of the index, not over rooms: a room of any size costs every listener
//                           the same <= 8 speaker rows, and no room is serial in its size here.
// The index is the caller's and is not trusted (as bridge_kernels.hip): room_start is clamped, every order[] entry is checked
// against [0, B), and every row number that went through memory (the speaker lists, pos_room) is checked again where it is read.
#include "kernels.h"
#include "speakers_rows.h"   // SPK_MAX, SPK_LANES, SpkAcc, spk_add, spk_clamp, spk_minus: shared with shared_bridge_kernels.hip

namespace lyra {

namespace {

constexpr int SPK_CHUNK = 8;    // positions per wavefront of the mix
constexpr int SPK_POS = 32767;  // LYRA_HIP_BRIDGE_MAX_ROOM: positions inside a room take 15 bits of a key

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_max(u64 v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 o = __shfl_xor(v, d);
    v = o > v ? o : v;
  }
  return v;
}

}  // namespace

// One wavefront per row, four rows per workgroup; lanes 0..39 own 16 bytes (8 samples) of the row.  A square is at most 2^30
// and a row's sum at most 320 * 2^30 < 2^39: 64-bit accumulation, a shuffle reduction, one 8-byte store.  The row's mix is
// zeroed (rows that no room names hear zeros; the mix kernel overwrites the others), is_speaker[row] too, and pos_room[row]
// is set to "no room" for row < n_members (n_members <= B, checked on the host), in place of three memsets.  The shared-encoder
// tick (shared_bridge_kernels.hip) has no per-listener mix: it passes mix = nullptr, which skips those stores, and two further
// words per row to set to -1, slot_of[row] and row_room[row]; the loudest-N calls pass nullptr for both.
__global__ __launch_bounds__(256) void speakers_level_kernel(const int16_t* __restrict__ pcm, int B, long long* __restrict__ levels,
                                                              int16_t* __restrict__ mix, int32_t* __restrict__ is_speaker,
                                                              int32_t* __restrict__ pos_room, int n_members,
                                                              int32_t* __restrict__ slot_of, int32_t* __restrict__ row_room) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  u64 acc = 0;
  if (lane < SPK_LANES) {
    const uint4 x = reinterpret_cast<const uint4*>(pcm + (size_t)row * 320)[lane];
    const unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int a = (int)(short)(w[i] & 0xffffu), b = (int)w[i] >> 16;
      acc += (u64)(unsigned)(a * a) + (u64)(unsigned)(b * b);   // (32768^2 = 2^30 fits an int)
    }
    if (mix) reinterpret_cast<uint4*>(mix + (size_t)row * 320)[lane] = make_uint4(0u, 0u, 0u, 0u);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  if (lane == 0) {
    levels[row] = (long long)acc;
    is_speaker[row] = 0;
    if (row < n_members) pos_room[row] = -1;
    if (slot_of) slot_of[row] = -1;
    if (row_room) row_room[row] = -1;
  }
}

// One wavefront per room, four rooms per workgroup.  Pass 0, lanes striding over the room's positions: the room number into
// pos_room, the entry checked (a bad one is counted -- here and in no other kernel), and the key of a candidate,
//   (level << 15) | (32767 - position in the room):  unique inside a room, larger = louder, earlier position first,
// zero for a member that is no candidate.  A room of up to 64 members keeps its keys in registers; a larger one parks them in
// keys[] (every lane re-reads only what it wrote).  Then max_speakers rounds of "the largest key below the previous winner" by
// wave max-reduction: what is serial in the room size M is M * max_speakers / 64 8-byte reads per lane, L2 hits.
// The winner's row is read back from order[] at the position its key names, and checked again: rooms that a wild room_start
// makes overlap may have written each other's keys.
__global__ __launch_bounds__(256) void speakers_select_kernel(const long long* __restrict__ levels, int B,
                                                               const int32_t* __restrict__ order,
                                                               const int32_t* __restrict__ room_start, int n_rooms, int n_members,
                                                               const int32_t* __restrict__ muted, const int32_t* __restrict__ is_cn,
                                                               int max_speakers, u64* keys, int32_t* __restrict__ spk,
                                                               int32_t* __restrict__ pos_room, int32_t* __restrict__ is_speaker,
                                                               unsigned* __restrict__ err) {
  const int lane = threadIdx.x & 63, room = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (room >= n_rooms) return;
  int lo = room_start[room], hi = room_start[room + 1];
  lo = lo < 0 ? 0 : lo > n_members ? n_members : lo;
  hi = hi < lo ? lo : hi > n_members ? n_members : hi;
  const bool in_regs = hi - lo <= 64;
  unsigned bad = 0;
  u64 mine = 0;
  // (the loads behind a bad entry are redirected to row 0 and masked, not skipped: without a branch around them the
  // unrolled loop keeps four members' index -> level chains in flight, which is what a room of thousands waits for)
#pragma unroll 4
  for (int p = lo + lane; p < hi; p += 64) {
    pos_room[p] = room;
    const int r = order[p];
    const bool ok = r >= 0 && r < B;
    const int rr = ok ? r : 0;
    const long long lv = levels[rr];
    const int m = muted ? muted[rr] : 0, cn = is_cn ? is_cn[rr] : 0;
    const int pos = p - lo;
    u64 key = 0;
    if (ok && m == 0 && cn == 0 && lv > 0) key = ((u64)lv << 15) | (u64)(SPK_POS - (pos > SPK_POS ? SPK_POS : pos));
    bad += ok ? 0u : 1u;
    if (in_regs) mine = key;
    else keys[p] = key;
  }
  u64 prev = ~0ull;
#pragma unroll 1
  for (int k = 0; k < SPK_MAX; ++k) {
    u64 best = 0;
    if (k < max_speakers && prev != 0) {
      if (in_regs) {
        best = mine < prev ? mine : 0;
      } else {
#pragma unroll 4
        for (int p = lo + lane; p < hi; p += 64) {
          const u64 v = keys[p];
          best = (v < prev && v > best) ? v : best;
        }
      }
      best = wave_max(best);
    }
    prev = best;
    int row = -1;
    if (best != 0) {
      const int p = lo + SPK_POS - (int)(best & (u64)SPK_POS);
      if (p < hi) row = order[p];
      if (row < 0 || row >= B) row = -1;
    }
    if (lane == 0) {
      spk[(size_t)room * SPK_MAX + k] = row;
      if (row >= 0) is_speaker[row] = 1;
    }
  }
  if (bad) atomicAdd(err, bad);
}

// One wavefront per chunk of SPK_CHUNK consecutive positions of the index, four chunks per workgroup; the 40 x 16-byte row
// layout and the back-to-back masked loads of bridge_mix_kernel.  Lane j < 8 reads position first + j: its room (pos_room,
// written by the select kernel; -1: no room covers the position) and its row (range-checked).  The chunk's listener rows are
// loaded first; then, position by position, the sum of the room's <= 8 speaker rows is formed when the room changes (rooms of
// 1, 2 and 3 change it inside a chunk), the listener's own row is taken out if it is on the speaker list, and the result is
// clamped and stored, 16 bytes per lane.  No atomics on audio, no sum buffer in memory.
__global__ __launch_bounds__(256) void speakers_mix_kernel(const int16_t* __restrict__ pcm, int B, const int32_t* __restrict__ order,
                                                            int n_members, const int32_t* __restrict__ pos_room, int n_rooms,
                                                            const int32_t* __restrict__ spk, int16_t* __restrict__ mix) {
  const int lane = threadIdx.x & 63, first = (blockIdx.x * 4 + (threadIdx.x >> 6)) * SPK_CHUNK;
  if (first >= n_members) return;
  const bool owner = lane < SPK_LANES;
  const int slice = owner ? lane : SPK_LANES - 1;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  int my_row = -1, my_room = -1;
  if (lane < SPK_CHUNK && first + lane < n_members) {
    const int room = pos_room[first + lane], r = order[first + lane];
    if (room >= 0 && room < n_rooms && r >= 0 && r < B) {
      my_row = r;
      my_room = room;
    }
  }
  uint4 x[SPK_CHUNK];
#pragma unroll
  for (int j = 0; j < SPK_CHUNK; ++j) {
    // (always a load from inside the buffer, masked afterwards: the eight requests go out back to back)
    const int r = __shfl(my_row, j);
    const uint4 v = reinterpret_cast<const uint4*>(pcm + (size_t)(r >= 0 ? r : 0) * 320)[slice];
    x[j] = (owner && r >= 0) ? v : zero4;
  }
  int cur = -1, my_spk = -1;   // lane k < 8: speaker k of room `cur` (-1: none)
  SpkAcc S;
#pragma unroll
  for (int i = 0; i < 8; ++i) S.v[i] = 0;
#pragma unroll
  for (int j = 0; j < SPK_CHUNK; ++j) {
    const int room = __builtin_amdgcn_readfirstlane(__shfl(my_room, j));
    const int r = __builtin_amdgcn_readfirstlane(__shfl(my_row, j));
    if (room < 0) continue;
    if (room != cur) {
      cur = room;
      my_spk = -1;
      if (lane < SPK_MAX) {
        const int s = spk[(size_t)room * SPK_MAX + lane];
        if (s >= 0 && s < B) my_spk = s;
      }
      uint4 y[SPK_MAX];
#pragma unroll
      for (int k = 0; k < SPK_MAX; ++k) {
        const int s = __shfl(my_spk, k);
        const uint4 v = reinterpret_cast<const uint4*>(pcm + (size_t)(s >= 0 ? s : 0) * 320)[slice];
        y[k] = (owner && s >= 0) ? v : zero4;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) S.v[i] = 0;
#pragma unroll
      for (int k = 0; k < SPK_MAX; ++k) spk_add(S, y[k]);
    }
    const bool own = __ballot(my_spk == r) != 0;   // (r >= 0 here, a lane without a speaker holds -1)
    if (owner) reinterpret_cast<uint4*>(mix + (size_t)r * 320)[lane] = spk_minus(S, x[j], own);
  }
}

}  // namespace lyra
