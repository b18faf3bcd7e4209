// speakers_rows.h -- the row arithmetic that speakers_kernels.hip and shared_bridge_kernels.hip share.  A 640-byte row of 320
// int16 samples is 40 lanes x 16 bytes; a lane sums its eight samples of up to SPK_MAX rows in int32 and takes at most one row
// out again before the clamp.
#pragma once
#include "kernels.h"

namespace lyra {

constexpr int SPK_MAX = 8;      // LYRA_HIP_SPEAKERS_MAX: speakers per room, and the width of a speaker list
constexpr int SPK_LANES = 40;   // 40 lanes x 16 bytes = one 640-byte row

struct SpkAcc { int v[8]; };

__device__ __forceinline__ void spk_add(SpkAcc& s, const uint4& x) {
  const unsigned w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    s.v[2 * i] += (int)(short)(w[i] & 0xffffu);
    s.v[2 * i + 1] += (int)w[i] >> 16;
  }
}

__device__ __forceinline__ int spk_clamp(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

// clamp(S - (own ? x : 0)), eight samples
__device__ __forceinline__ uint4 spk_minus(const SpkAcc& s, const uint4& x, bool own) {
  const unsigned w[4] = {x.x, x.y, x.z, x.w};
  unsigned o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int lo = own ? (int)(short)(w[i] & 0xffffu) : 0, hi = own ? (int)w[i] >> 16 : 0;
    o[i] = ((unsigned)spk_clamp(s.v[2 * i] - lo) & 0xffffu) | ((unsigned)spk_clamp(s.v[2 * i + 1] - hi) << 16);
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

}  // namespace lyra
