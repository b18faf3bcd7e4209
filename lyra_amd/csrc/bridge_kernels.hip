// bridge_kernels.hip -- the mix-minus of a conference bridge (include/lyra_hip_bridge.h, bridge_api.inc): every participant
// hears the sum of the other sources of its room.  Integer arithmetic only: S_r = the int32 sum of the room's source rows,
// y_b = clamp(S_r - (source_b ? x_b : 0)); exact and order-free.  Membership arrives as an inverted index (order[]: row
// numbers, a room's rows contiguous; room_start[]: the boundaries), so every row is stored once and summed per destination:
// no atomics on the audio and no zeroed sum buffer.  Rows that no room names are not touched here (the host zeroes the mix
// buffer in front of the launch).
#include "kernels.h"

namespace lyra {

namespace {

constexpr int BRIDGE_CHUNK = 8;    // member rows in flight per wavefront
constexpr int BRIDGE_LANES = 40;   // 40 lanes x 16 bytes = one 640-byte row

struct BridgeAcc { int v[8]; };

__device__ __forceinline__ void bridge_add(BridgeAcc& s, const uint4& x) {
  const unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    s.v[2 * i] += (int)(short)(w[i] & 0xffffu);
    s.v[2 * i + 1] += (int)w[i] >> 16;
  }
}

__device__ __forceinline__ int bridge_clamp(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

// clamp(S - (src ? x : 0)), eight samples
__device__ __forceinline__ uint4 bridge_minus(const BridgeAcc& s, const uint4& x, bool src) {
  const unsigned w[4] = {x.x, x.y, x.z, x.w};
  unsigned o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lo = src ? (int)(short)(w[i] & 0xffffu) : 0, hi = src ? (int)w[i] >> 16 : 0;
    o[i] = ((unsigned)bridge_clamp(s.v[2 * i] - lo) & 0xffffu) | ((unsigned)bridge_clamp(s.v[2 * i + 1] - hi) << 16);
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

}  // namespace

// One wavefront per room, four rooms per workgroup; lanes 0..39 own one 16-byte slice (8 samples) of the 640-byte row.
// Members are read in chunks of up to BRIDGE_CHUNK rows held in registers: a room of up to BRIDGE_CHUNK reads every row once
// and writes once; a larger room takes a sum pass and a write pass (the second read of a row is an L2 hit).
// The index is the caller's and is not trusted: room_start values are clamped to [0, n_members] (and a room that ends before
// it starts is empty), every order[] entry is checked against [0, B) -- a bad one is skipped and counted once in *err.
// pcm and mix must be 16-byte aligned (checked on the host).
__global__ __launch_bounds__(256) void bridge_mix_kernel(const int16_t* __restrict__ pcm, int B, const int32_t* __restrict__ order,
                                                          const int32_t* __restrict__ room_start, int n_rooms, int n_members,
                                                          const int32_t* __restrict__ muted, const int32_t* __restrict__ is_cn,
                                                          int16_t* __restrict__ mix, unsigned* __restrict__ err) {
  const int lane = threadIdx.x & 63, room = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (room >= n_rooms) return;
  int lo = room_start[room], hi = room_start[room + 1];
  lo = lo < 0 ? 0 : lo > n_members ? n_members : lo;
  hi = hi < lo ? lo : hi > n_members ? n_members : hi;
  const bool owner = lane < BRIDGE_LANES;
  const int slice = owner ? lane : BRIDGE_LANES - 1;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  BridgeAcc S;
#pragma unroll
  for (int i = 0; i < 8; ++i) S.v[i] = 0;
  uint4 x[BRIDGE_CHUNK];
  int my_row = -1, my_src = 0;   // lane j < BRIDGE_CHUNK: member j of the chunk (-1: none, or a bad entry)
  unsigned bad = 0;

  // lane j reads member `first + j`: its row number (range-checked) and whether it is a source
  auto load_members = [&](int first, bool count) {
    my_row = -1;
    my_src = 0;
    if (lane < BRIDGE_CHUNK && first + lane < hi) {
      const int r = order[first + lane];
      if (r >= 0 && r < B) {
        my_row = r;
        my_src = !(muted && muted[r] != 0) && !(is_cn && is_cn[r] != 0);
      } else if (count) {
        ++bad;
      }
    }
  };
  auto load_rows = [&]() {
#pragma unroll
    for (int j = 0; j < BRIDGE_CHUNK; ++j) {
      // (always a load from inside the buffer, masked afterwards: the eight requests go out back to back)
      const int r = __shfl(my_row, j);
      const uint4 v = reinterpret_cast<const uint4*>(pcm + (size_t)(r >= 0 ? r : 0) * 320)[slice];
      x[j] = (owner && r >= 0) ? v : zero4;
    }
  };
  auto add_rows = [&]() {
#pragma unroll
    for (int j = 0; j < BRIDGE_CHUNK; ++j)
      if (__shfl(my_src, j)) bridge_add(S, x[j]);
  };
  auto write_rows = [&]() {
#pragma unroll
    for (int j = 0; j < BRIDGE_CHUNK; ++j) {
      const int r = __shfl(my_row, j);
      const bool src = __shfl(my_src, j) != 0;
      if (owner && r >= 0) reinterpret_cast<uint4*>(mix + (size_t)r * 320)[lane] = bridge_minus(S, x[j], src);
    }
  };

  if (hi - lo <= BRIDGE_CHUNK) {
    load_members(lo, true);
    load_rows();
    add_rows();
    write_rows();
  } else {
    for (int first = lo; first < hi; first += BRIDGE_CHUNK) {
      load_members(first, true);
      load_rows();
      add_rows();
    }
    for (int first = lo; first < hi; first += BRIDGE_CHUNK) {
      load_members(first, false);
      load_rows();
      write_rows();
    }
  }
  if (bad) atomicAdd(err, bad);
}

}  // namespace lyra
