// meeting_kernels.hip -- the conference bridge's mix over a meeting whose membership changes, as ONE pass
// (include/lyra_hip_spans_meeting.h, meeting_api.inc).  The work per unit is bridge_spans_kernels.hip's: one wavefront per
// (room, tick) with members in register chunks of 8, zeros for present participants in no room, levels per (participant,
// tick), the selection per (room, tick) with keys in registers up to 64 members and parked above, the speakers' mix per 8
// positions; the row layout is the tick kernels' (lanes 0..39 own 16 bytes of a 640-byte row, loads masked and not branched
// around; speakers_rows.h).  What differs is where a wavefront's work comes from: per-epoch launches would be correct but a
// churny meeting has thousands of epochs of a few ticks, so a launch covers a slab of epoch pieces and every wavefront looks
// its piece up in the table (meeting_kernels.h).  The lookup is wave-uniform: scalar loads, plain C++.
#include "meeting_kernels.h"
#include "speakers_rows.h"   // SPK_MAX, SPK_LANES, SpkAcc, spk_add, spk_minus

namespace lyra {

namespace {

constexpr int MEET_CHUNK = 8;     // member rows in flight per wavefront
constexpr int MEET_POS = 32767;   // LYRA_HIP_BRIDGE_MAX_ROOM: positions inside a room take 15 bits of a key

typedef unsigned long long u64;

__device__ __forceinline__ u64 meet_wave_max(u64 v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 o = __shfl_xor(v, d);
    v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ int meet_units(const MeetEpoch& E, int kind) {
  return kind == MEET_ROOMS ? E.n_rooms
         : kind == MEET_LONE ? E.n_entries - E.n_members
         : kind == MEET_ENTRIES ? E.n_entries
                                : (E.n_members + MEET_CHUNK - 1) / MEET_CHUNK;
}

// wavefront w of a launch over the pieces [e_lo, e_hi) counted in `kind`: its piece, its unit and its tick inside the piece;
// false: past the slab.  The last piece whose first wavefront is not above w is the one (pieces without a unit of this kind
// share their first wavefront with the next piece).
template <int KIND>
__device__ __forceinline__ bool meet_find(const MeetEpoch* __restrict__ tab, int e_lo, int e_hi, long long n_waves,
                                          const MeetEpoch** piece, int* unit, int* tick) {
  const long long w = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= n_waves) return false;
  const long long at = tab[e_lo].wave0[KIND] + w;
  int lo = e_lo, hi = e_hi - 1;   // the answer is in [lo, hi]
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (tab[mid].wave0[KIND] <= at) lo = mid;
    else hi = mid - 1;
  }
  const MeetEpoch* E = tab + lo;
  const int units = meet_units(*E, KIND);
  if (units <= 0) return false;   // (the host counts n_waves from the same table: not reached)
  const long long local = at - E->wave0[KIND];
  const int t = (int)(local / units);
  if (t >= E->n_ticks) return false;
  *piece = E;
  *tick = t;
  *unit = (int)(local - (long long)t * units);
  return true;
}

}  // namespace

__global__ __launch_bounds__(256) void meeting_mix_kernel(const MeetEpoch* __restrict__ tab, int e_lo, int e_hi, long long n_waves,
                                                           const int16_t* __restrict__ pcm, const long long* __restrict__ base,
                                                           const int32_t* __restrict__ room_start,
                                                           const int32_t* __restrict__ muted, const int32_t* __restrict__ is_cn,
                                                           int16_t* __restrict__ mix) {
  const int lane = threadIdx.x & 63;
  const MeetEpoch* E;
  int room, tick;
  if (!meet_find<MEET_ROOMS>(tab, e_lo, e_hi, n_waves, &E, &room, &tick)) return;
  const long long t = E->tick0 + tick;
  const long long* first = base + E->entry0;
  const int lo = room_start[E->room0 + room], hi = room_start[E->room0 + room + 1];
  const bool owner = lane < SPK_LANES;
  const int slice = owner ? lane : SPK_LANES - 1;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  SpkAcc S;
#pragma unroll
  for (int i = 0; i < 8; ++i) S.v[i] = 0;
  uint4 x[MEET_CHUNK];
  long long my_frame = -1;   // lane j < MEET_CHUNK: the frame of member j of the chunk (-1: none)
  int my_src = 0;

  auto load_members = [&](int at) {
    my_frame = -1;
    my_src = 0;
    if (lane < MEET_CHUNK && at + lane < hi) {
      my_frame = first[at + lane] + t;
      my_src = !(muted && muted[my_frame] != 0) && !(is_cn && is_cn[my_frame] != 0);
    }
  };
  auto load_rows = [&]() {
#pragma unroll
    for (int j = 0; j < MEET_CHUNK; ++j) {
      // (always a load from inside the buffer -- the chunk's first member's frame -- masked afterwards: back to back)
      const long long f = __shfl(my_frame, j), f0 = __shfl(my_frame, 0);
      const uint4 v = reinterpret_cast<const uint4*>(pcm + (size_t)(f >= 0 ? f : f0) * 320)[slice];
      x[j] = (owner && f >= 0) ? v : zero4;
    }
  };
  auto add_rows = [&]() {
#pragma unroll
    for (int j = 0; j < MEET_CHUNK; ++j)
      if (__shfl(my_src, j)) spk_add(S, x[j]);
  };
  auto write_rows = [&]() {
#pragma unroll
    for (int j = 0; j < MEET_CHUNK; ++j) {
      const long long f = __shfl(my_frame, j);
      const bool src = __shfl(my_src, j) != 0;
      if (owner && f >= 0) reinterpret_cast<uint4*>(mix + (size_t)f * 320)[lane] = spk_minus(S, x[j], src);
    }
  };

  if (hi <= lo) return;   // (the planner makes no empty room; lane 0 of every chunk below holds a member)
  if (hi - lo <= MEET_CHUNK) {
    load_members(lo);
    load_rows();
    add_rows();
    write_rows();
  } else {
    for (int at = lo; at < hi; at += MEET_CHUNK) {
      load_members(at);
      load_rows();
      add_rows();
    }
    for (int at = lo; at < hi; at += MEET_CHUNK) {
      load_members(at);
      load_rows();
      write_rows();
    }
  }
}

__global__ __launch_bounds__(256) void meeting_zero_kernel(const MeetEpoch* __restrict__ tab, int e_lo, int e_hi, long long n_waves,
                                                            const long long* __restrict__ base, int16_t* __restrict__ mix) {
  const int lane = threadIdx.x & 63;
  const MeetEpoch* E;
  int i, tick;
  if (!meet_find<MEET_LONE>(tab, e_lo, e_hi, n_waves, &E, &i, &tick)) return;
  const long long f = base[E->entry0 + E->n_members + i] + E->tick0 + tick;
  if (lane < SPK_LANES) reinterpret_cast<uint4*>(mix + (size_t)f * 320)[lane] = make_uint4(0u, 0u, 0u, 0u);
}

// speakers_level_kernel's sum of squares (at most 320 * 2^30 < 2^39) of the frame
__global__ __launch_bounds__(256) void meeting_level_kernel(const MeetEpoch* __restrict__ tab, int e_lo, int e_hi, long long n_waves,
                                                             const int16_t* __restrict__ pcm, const long long* __restrict__ base,
                                                             const int32_t* __restrict__ room, unsigned char* __restrict__ sel,
                                                             long long* __restrict__ levels, int16_t* __restrict__ mix,
                                                             int32_t* __restrict__ is_speaker) {
  const int lane = threadIdx.x & 63;
  const MeetEpoch* E;
  int p, tick;
  if (!meet_find<MEET_ENTRIES>(tab, e_lo, e_hi, n_waves, &E, &p, &tick)) return;
  const long long f = base[E->entry0 + p] + E->tick0 + tick;
  long long* lv = reinterpret_cast<long long*>(sel + E->sel);
  u64 acc = 0;
  if (lane < SPK_LANES) {
    const uint4 x = reinterpret_cast<const uint4*>(pcm + (size_t)f * 320)[lane];
    const unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int a = (int)(short)(w[i] & 0xffffu), b = (int)w[i] >> 16;
      acc += (u64)(unsigned)(a * a) + (u64)(unsigned)(b * b);   // (32768^2 = 2^30 fits an int)
    }
    if (room[E->entry0 + p] < 0) reinterpret_cast<uint4*>(mix + (size_t)f * 320)[lane] = make_uint4(0u, 0u, 0u, 0u);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  if (lane == 0) {
    lv[(size_t)tick * E->n_entries + p] = (long long)acc;
    if (levels) levels[f] = (long long)acc;
    if (is_speaker) is_speaker[f] = 0;
  }
}

// speakers_select_kernel's keys, (level << 15) | (32767 - position in the room), zero for a member that is no candidate, and
// its max_speakers rounds of "the largest key below the previous winner"
__global__ __launch_bounds__(256) void meeting_select_kernel(const MeetEpoch* __restrict__ tab, int e_lo, int e_hi, long long n_waves,
                                                              const long long* __restrict__ base,
                                                              const int32_t* __restrict__ room_start,
                                                              const int32_t* __restrict__ muted, const int32_t* __restrict__ is_cn,
                                                              int max_speakers, unsigned char* sel,
                                                              int32_t* __restrict__ is_speaker) {
  const int lane = threadIdx.x & 63;
  const MeetEpoch* E;
  int room, tick;
  if (!meet_find<MEET_ROOMS>(tab, e_lo, e_hi, n_waves, &E, &room, &tick)) return;
  const long long t = E->tick0 + tick;
  const long long* first = base + E->entry0;
  const int n_entries = E->n_entries, n_rooms = E->n_rooms, n_members = E->n_members;
  const long long* lv = reinterpret_cast<const long long*>(sel + E->sel) + (size_t)tick * n_entries;
  int32_t* spk = reinterpret_cast<int32_t*>(sel + E->sel + (size_t)E->n_ticks * n_entries * 8) + ((size_t)tick * n_rooms + room) * SPK_MAX;
  u64* park = reinterpret_cast<u64*>(sel + E->sel + (size_t)E->n_ticks * ((size_t)n_entries * 8 + (size_t)n_rooms * SPK_MAX * 4)) +
              (size_t)tick * n_members;   // (there only in a big piece; not touched by a room that fits the registers)
  const int lo = room_start[E->room0 + room], hi = room_start[E->room0 + room + 1];
  const bool in_regs = hi - lo <= 64;
  u64 mine = 0;
#pragma unroll 4
  for (int p = lo + lane; p < hi; p += 64) {
    const long long f = first[p] + t;
    const long long level = lv[p];
    const int m = muted ? muted[f] : 0, cn = is_cn ? is_cn[f] : 0;
    const int pos = p - lo;
    u64 key = 0;
    if (m == 0 && cn == 0 && level > 0) key = ((u64)level << 15) | (u64)(MEET_POS - (pos > MEET_POS ? MEET_POS : pos));
    if (in_regs) mine = key;
    else park[p] = key;
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
          const u64 v = park[p];
          best = (v < prev && v > best) ? v : best;
        }
      }
      best = meet_wave_max(best);
    }
    prev = best;
    int part = -1;
    if (best != 0) {
      const int p = lo + MEET_POS - (int)(best & (u64)MEET_POS);
      if (p < hi) part = p;
    }
    if (lane == 0) {
      spk[k] = part;
      if (part >= 0 && is_speaker) is_speaker[first[part] + t] = 1;
    }
  }
}

// speakers_mix_kernel with the rows at their frames: the chunk's listener rows are loaded first; then, position by position,
// the sum of the room's <= 8 speaker rows is formed when the room changes, the listener's own row is taken out if it is on
// the list, and the result is clamped and stored
__global__ __launch_bounds__(256) void meeting_speakers_mix_kernel(const MeetEpoch* __restrict__ tab, int e_lo, int e_hi,
                                                                    long long n_waves, const int16_t* __restrict__ pcm,
                                                                    const long long* __restrict__ base,
                                                                    const int32_t* __restrict__ room,
                                                                    const unsigned char* __restrict__ sel, int16_t* __restrict__ mix) {
  const int lane = threadIdx.x & 63;
  const MeetEpoch* E;
  int chunk, tick;
  if (!meet_find<MEET_CHUNKS>(tab, e_lo, e_hi, n_waves, &E, &chunk, &tick)) return;
  const long long t = E->tick0 + tick;
  const long long* first = base + E->entry0;
  const int n_members = E->n_members, n_rooms = E->n_rooms;
  const int32_t* spk = reinterpret_cast<const int32_t*>(sel + E->sel + (size_t)E->n_ticks * E->n_entries * 8) +
                       (size_t)tick * n_rooms * SPK_MAX;
  const int at = chunk * MEET_CHUNK;
  const bool owner = lane < SPK_LANES;
  const int slice = owner ? lane : SPK_LANES - 1;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  int my_part = -1, my_room = -1;
  long long my_frame = -1;
  if (lane < MEET_CHUNK && at + lane < n_members) {
    my_part = at + lane;
    my_room = room[E->entry0 + at + lane];
    my_frame = first[my_part] + t;
  }
  const long long f0 = __shfl(my_frame, 0);   // (at < n_members: lane 0 holds a member)
  uint4 x[MEET_CHUNK];
#pragma unroll
  for (int j = 0; j < MEET_CHUNK; ++j) {
    const long long f = __shfl(my_frame, j);
    const uint4 v = reinterpret_cast<const uint4*>(pcm + (size_t)(f >= 0 ? f : f0) * 320)[slice];
    x[j] = (owner && f >= 0) ? v : zero4;
  }
  int cur = -1, my_spk = -1;   // lane k < 8: speaker k of room `cur`, a position inside the epoch (-1: none)
  long long my_spk_frame = -1;
  SpkAcc S;
#pragma unroll
  for (int i = 0; i < 8; ++i) S.v[i] = 0;
#pragma unroll
  for (int j = 0; j < MEET_CHUNK; ++j) {
    const int r = __builtin_amdgcn_readfirstlane(__shfl(my_room, j));
    const int part = __builtin_amdgcn_readfirstlane(__shfl(my_part, j));
    const long long f = __shfl(my_frame, j);
    if (r < 0 || r >= n_rooms || part < 0) continue;
    if (r != cur) {
      cur = r;
      my_spk = -1;
      my_spk_frame = -1;
      if (lane < SPK_MAX) {
        const int s = spk[(size_t)r * SPK_MAX + lane];
        if (s >= 0 && s < n_members) {
          my_spk = s;
          my_spk_frame = first[s] + t;
        }
      }
      uint4 y[SPK_MAX];
#pragma unroll
      for (int k = 0; k < SPK_MAX; ++k) {
        const long long fs = __shfl(my_spk_frame, k);
        const uint4 v = reinterpret_cast<const uint4*>(pcm + (size_t)(fs >= 0 ? fs : f0) * 320)[slice];
        y[k] = (owner && fs >= 0) ? v : zero4;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) S.v[i] = 0;
#pragma unroll
      for (int k = 0; k < SPK_MAX; ++k) spk_add(S, y[k]);
    }
    const bool own = __ballot(my_spk == part) != 0;   // (part >= 0 here, a lane without a speaker holds -1)
    if (owner) reinterpret_cast<uint4*>(mix + (size_t)f * 320)[lane] = spk_minus(S, x[j], own);
  }
}

}  // namespace lyra
