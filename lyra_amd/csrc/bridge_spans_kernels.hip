// bridge_spans_kernels.hip -- the conference bridge's mix as ONE pass over all ticks of a recording
// (include/lyra_hip_bridge_spans.h, bridge_spans_api.inc).  The mix of a tick reads that tick's hop, mutes and comfort-noise
// flags and nothing of any other tick: exact integer arithmetic without cross-tick state, in the full mix
// (bridge_kernels.hip) and in the loudest-N selection (speakers_kernels.hip) alike.  So the kernels here are those two files'
// with a tick dimension: participant p's tick t is buffer frame first[p] + t of the span calls' frame-major buffers, and
// every row address is (first[p] + t) * 320 in 64 bits.  The row layout is the tick kernels': lanes 0..39 own 16 bytes of a
// 640-byte row, loads are masked and not branched around.  The index (order, room_start, pos_room, part_room, lone) is over
// participant numbers 0..P-1 and is the library's own, built and checked on the host: nothing here counts bad entries, and the
// speaker lists hold numbers copied from it (every list of a slab is written, -1 padded, before the slab's mix reads it).
// A launch covers one slab of ticks [t0, t0 + n_ticks); the host keeps (units per tick) * n_ticks below 2^31.
#include "bridge_spans_kernels.h"
#include "speakers_rows.h"   // SPK_MAX, SPK_LANES, SpkAcc, spk_add, spk_clamp, spk_minus

namespace lyra {

namespace {

constexpr int BSP_CHUNK = 8;     // member rows in flight per wavefront
constexpr int BSP_POS = 32767;   // LYRA_HIP_BRIDGE_MAX_ROOM: positions inside a room take 15 bits of a key

typedef unsigned long long u64;

__device__ __forceinline__ u64 bsp_wave_max(u64 v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 o = __shfl_xor(v, d);
    v = o > v ? o : v;
  }
  return v;
}

// wavefront w of a launch over `units` units per tick: its unit and its tick inside the slab; false: past the slab
__device__ __forceinline__ bool bsp_unit(int units, int n_ticks, int* unit, int* tick) {
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (long long)units * n_ticks) return false;
  *tick = (int)(w / units);
  *unit = (int)(w - (long long)*tick * units);
  return true;
}

}  // namespace

// One wavefront per (room, tick), four per workgroup; members in register chunks of BSP_CHUNK as in bridge_mix_kernel: a room
// of up to 8 reads every row once and writes once, a larger one takes a sum pass and a write pass.  muted and is_cn are read
// at the member's frame.
__global__ __launch_bounds__(256) void bridge_spans_mix_kernel(const int16_t* __restrict__ pcm, const long long* __restrict__ first,
                                                                const int32_t* __restrict__ order,
                                                                const int32_t* __restrict__ room_start, int n_rooms, long long t0,
                                                                int n_ticks, const int32_t* __restrict__ muted,
                                                                const int32_t* __restrict__ is_cn, int16_t* __restrict__ mix) {
  const int lane = threadIdx.x & 63;
  int room, tick;
  if (!bsp_unit(n_rooms, n_ticks, &room, &tick)) return;
  const long long t = t0 + tick;
  const int lo = room_start[room], hi = room_start[room + 1];
  const bool owner = lane < SPK_LANES;
  const int slice = owner ? lane : SPK_LANES - 1;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  SpkAcc S;
#pragma unroll
  for (int i = 0; i < 8; ++i) S.v[i] = 0;
  uint4 x[BSP_CHUNK];
  long long my_frame = -1;   // lane j < BSP_CHUNK: the frame of member j of the chunk (-1: none)
  int my_src = 0;

  auto load_members = [&](int at) {
    my_frame = -1;
    my_src = 0;
    if (lane < BSP_CHUNK && at + lane < hi) {
      my_frame = first[order[at + lane]] + t;
      my_src = !(muted && muted[my_frame] != 0) && !(is_cn && is_cn[my_frame] != 0);
    }
  };
  auto load_rows = [&]() {
#pragma unroll
    for (int j = 0; j < BSP_CHUNK; ++j) {
      // (always a load from inside the buffer -- the room's first member's frame -- masked afterwards: back to back)
      const long long f = __shfl(my_frame, j), f0 = __shfl(my_frame, 0);
      const uint4 v = reinterpret_cast<const uint4*>(pcm + (size_t)(f >= 0 ? f : f0) * 320)[slice];
      x[j] = (owner && f >= 0) ? v : zero4;
    }
  };
  auto add_rows = [&]() {
#pragma unroll
    for (int j = 0; j < BSP_CHUNK; ++j)
      if (__shfl(my_src, j)) spk_add(S, x[j]);
  };
  auto write_rows = [&]() {
#pragma unroll
    for (int j = 0; j < BSP_CHUNK; ++j) {
      const long long f = __shfl(my_frame, j);
      const bool src = __shfl(my_src, j) != 0;
      if (owner && f >= 0) reinterpret_cast<uint4*>(mix + (size_t)f * 320)[lane] = spk_minus(S, x[j], src);
    }
  };

  if (hi <= lo) return;   // (the planner makes no empty room; lane 0 of every chunk below holds a member)
  if (hi - lo <= BSP_CHUNK) {
    load_members(lo);
    load_rows();
    add_rows();
    write_rows();
  } else {
    for (int at = lo; at < hi; at += BSP_CHUNK) {
      load_members(at);
      load_rows();
      add_rows();
    }
    for (int at = lo; at < hi; at += BSP_CHUNK) {
      load_members(at);
      load_rows();
      write_rows();
    }
  }
}

// One wavefront per (participant in no room, tick): nobody hears it and it hears zeros.
__global__ __launch_bounds__(256) void bridge_spans_zero_kernel(const long long* __restrict__ first, const int32_t* __restrict__ lone,
                                                                 int n_lone, long long t0, int n_ticks, int16_t* __restrict__ mix) {
  const int lane = threadIdx.x & 63;
  int i, tick;
  if (!bsp_unit(n_lone, n_ticks, &i, &tick)) return;
  const long long f = first[lone[i]] + t0 + tick;
  if (lane < SPK_LANES) reinterpret_cast<uint4*>(mix + (size_t)f * 320)[lane] = make_uint4(0u, 0u, 0u, 0u);
}

// One wavefront per (participant, tick): speakers_level_kernel's sum of squares (at most 320 * 2^30 < 2^39) of the frame.
__global__ __launch_bounds__(256) void bridge_spans_level_kernel(const int16_t* __restrict__ pcm, const long long* __restrict__ first,
                                                                  const int32_t* __restrict__ part_room, int P, long long t0,
                                                                  int n_ticks, long long* __restrict__ lv,
                                                                  long long* __restrict__ levels, int16_t* __restrict__ mix,
                                                                  int32_t* __restrict__ is_speaker) {
  const int lane = threadIdx.x & 63;
  int p, tick;
  if (!bsp_unit(P, n_ticks, &p, &tick)) return;
  const long long f = first[p] + t0 + tick;
  u64 acc = 0;
  if (lane < SPK_LANES) {
    const uint4 x = reinterpret_cast<const uint4*>(pcm + (size_t)f * 320)[lane];
    const unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int a = (int)(short)(w[i] & 0xffffu), b = (int)w[i] >> 16;
      acc += (u64)(unsigned)(a * a) + (u64)(unsigned)(b * b);   // (32768^2 = 2^30 fits an int)
    }
    if (part_room[p] < 0) reinterpret_cast<uint4*>(mix + (size_t)f * 320)[lane] = make_uint4(0u, 0u, 0u, 0u);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
  if (lane == 0) {
    lv[(size_t)tick * P + p] = (long long)acc;
    if (levels) levels[f] = (long long)acc;
    if (is_speaker) is_speaker[f] = 0;
  }
}

// One wavefront per (room, tick): speakers_select_kernel's keys, (level << 15) | (32767 - position in the room), zero for a
// member that is no candidate, and its max_speakers rounds of "the largest key below the previous winner".  A room of up to
// 64 members keeps its keys in registers, a larger one parks them in keys[tick in slab][position].
__global__ __launch_bounds__(256) void bridge_spans_select_kernel(const long long* __restrict__ lv, const long long* __restrict__ first,
                                                                   const int32_t* __restrict__ order,
                                                                   const int32_t* __restrict__ room_start, int n_rooms,
                                                                   int n_members, int P, long long t0, int n_ticks,
                                                                   const int32_t* __restrict__ muted,
                                                                   const int32_t* __restrict__ is_cn, int max_speakers, u64* keys,
                                                                   int32_t* __restrict__ spk, int32_t* __restrict__ is_speaker) {
  const int lane = threadIdx.x & 63;
  int room, tick;
  if (!bsp_unit(n_rooms, n_ticks, &room, &tick)) return;
  const long long t = t0 + tick;
  const int lo = room_start[room], hi = room_start[room + 1];
  const bool in_regs = hi - lo <= 64;
  u64* park = keys + (size_t)tick * n_members;   // (not touched by a room that fits the registers)
  u64 mine = 0;
#pragma unroll 4
  for (int p = lo + lane; p < hi; p += 64) {
    const int part = order[p];
    const long long f = first[part] + t;
    const long long level = lv[(size_t)tick * P + part];
    const int m = muted ? muted[f] : 0, cn = is_cn ? is_cn[f] : 0;
    const int pos = p - lo;
    u64 key = 0;
    if (m == 0 && cn == 0 && level > 0) key = ((u64)level << 15) | (u64)(BSP_POS - (pos > BSP_POS ? BSP_POS : pos));
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
      best = bsp_wave_max(best);
    }
    prev = best;
    int part = -1;
    if (best != 0) {
      const int p = lo + BSP_POS - (int)(best & (u64)BSP_POS);
      if (p < hi) part = order[p];
    }
    if (lane == 0) {
      spk[((size_t)tick * n_rooms + room) * SPK_MAX + k] = part;
      if (part >= 0 && is_speaker) is_speaker[first[part] + t] = 1;
    }
  }
}

// One wavefront per (chunk of BSP_CHUNK consecutive positions of the index, tick): speakers_mix_kernel with the rows at their
// frames.  The chunk's listener rows are loaded first; then, position by position, the sum of the room's <= 8 speaker rows is
// formed when the room changes, the listener's own row is taken out if it is on the list, and the result is clamped and stored.
__global__ __launch_bounds__(256) void bridge_spans_speakers_mix_kernel(const int16_t* __restrict__ pcm,
                                                                         const long long* __restrict__ first,
                                                                         const int32_t* __restrict__ order, int n_members,
                                                                         const int32_t* __restrict__ pos_room, int n_rooms,
                                                                         long long t0, int n_ticks, const int32_t* __restrict__ spk,
                                                                         int16_t* __restrict__ mix) {
  const int lane = threadIdx.x & 63;
  int chunk, tick;
  if (!bsp_unit((n_members + BSP_CHUNK - 1) / BSP_CHUNK, n_ticks, &chunk, &tick)) return;
  const long long t = t0 + tick;
  const int at = chunk * BSP_CHUNK;
  const bool owner = lane < SPK_LANES;
  const int slice = owner ? lane : SPK_LANES - 1;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  int my_part = -1, my_room = -1;
  long long my_frame = -1;
  if (lane < BSP_CHUNK && at + lane < n_members) {
    my_part = order[at + lane];
    my_room = pos_room[at + lane];
    my_frame = first[my_part] + t;
  }
  const long long f0 = __shfl(my_frame, 0);   // (at < n_members: lane 0 holds a member)
  uint4 x[BSP_CHUNK];
#pragma unroll
  for (int j = 0; j < BSP_CHUNK; ++j) {
    const long long f = __shfl(my_frame, j);
    const uint4 v = reinterpret_cast<const uint4*>(pcm + (size_t)(f >= 0 ? f : f0) * 320)[slice];
    x[j] = (owner && f >= 0) ? v : zero4;
  }
  int cur = -1, my_spk = -1;   // lane k < 8: speaker k of room `cur`, a participant number (-1: none)
  long long my_spk_frame = -1;
  SpkAcc S;
#pragma unroll
  for (int i = 0; i < 8; ++i) S.v[i] = 0;
#pragma unroll
  for (int j = 0; j < BSP_CHUNK; ++j) {
    const int room = __builtin_amdgcn_readfirstlane(__shfl(my_room, j));
    const int part = __builtin_amdgcn_readfirstlane(__shfl(my_part, j));
    const long long f = __shfl(my_frame, j);
    if (room < 0 || room >= n_rooms || part < 0) continue;
    if (room != cur) {
      cur = room;
      my_spk = -1;
      my_spk_frame = -1;
      if (lane < SPK_MAX) {
        const int s = spk[((size_t)tick * n_rooms + room) * SPK_MAX + lane];
        if (s >= 0) {
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
