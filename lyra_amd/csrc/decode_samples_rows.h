// decode_samples_rows.h -- what the kernels of the three DecodeSamples calls share, as device-inline functions: a row's plan
// (ds_plan_kernel, ds_plan_any_kernel, ds_plan_streams_kernel: each keeps only its head -- where `rx`, the round's total and
// "may this row write its state" come from) and a row's splice at 8 / 32 / 48 kHz (ds_splice_kernel, ds_splice_streams_kernel).
// A fix to the ring move, the leftover hand-out or the resampler's use is made here, once.
#pragma once
#include "kernels.h"
#include "decode_samples_any_plan.h"
#include "resample_pass.h"

namespace lyra {

// what the plan's one-thread-per-row half leaves its 16-lanes-per-row half, per row of the workgroup
struct DsPlanLds { int id[256], push[256], src[256]; };

__device__ __forceinline__ void ds_plan_lds_clear(DsPlanLds& sh, int tid) {
  sh.push[tid] = -1;
  sh.src[tid] = DS_SRC_NONE;
}

// One thread, row b of stream `id`: applies the transition for a pass total of `total` samples (a packet arrived: rx), writes
// the state back unless the row is one whose plan must change nothing, and hands out the round's id lists (-1 = the row skips
// that leg) and the four info words.  Adds to nerr: packets that found the ring full, a plan that left its proven bounds.
__device__ __forceinline__ void ds_plan_row(DsPlanLds& sh, int tid, int b, int id, bool rx, int total, bool write_state, int& nerr,
                                            uint8_t* __restrict__ cng_state, int32_t* __restrict__ gen_ids,
                                            int32_t* __restrict__ cng1_ids, int32_t* __restrict__ cng2_ids,
                                            int32_t* __restrict__ est_ids, int32_t* __restrict__ info) {
  DsState* sp = reinterpret_cast<DsState*>(cng_state + (size_t)id * st::CNG_BYTES + DS_STATE);
  const DsPlan p = ds_plan(*sp, rx, total);
  if (write_state) *sp = p.s;
  nerr += p.dropped + p.bad;
  gen_ids[b] = p.gen_start >= 0 ? id : -1;
  cng1_ids[b] = p.cng_start == 0 ? id : -1;
  cng2_ids[b] = p.cng_start == 1 ? id : -1;
  est_ids[b] = p.est_seg >= 0 ? id : -1;
  int32_t w[4];
  ds_info(p, w);
  *reinterpret_cast<int4*>(info + (size_t)b * 4) = make_int4(w[0], w[1], w[2], w[3]);
  const bool direct = p.push_slot >= 0 && p.gen_src == p.push_slot;   // this call's packet starts its hop at once
  sh.id[tid] = id;
  sh.push[tid] = direct ? -1 : p.push_slot;
  sh.src[tid] = direct ? DS_SRC_NONE : p.gen_src;
}

// the sum of n (>= 0) over a wavefront's lanes, added to *counter: one atomic per wavefront at most
__device__ __forceinline__ void ds_wave_count(int n, unsigned* __restrict__ counter, int tid) {
  if (__ballot(n != 0)) {   // (wave-uniform)
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
    if ((tid & 63) == 0) atomicAdd(counter, (unsigned)n);
  }
}

// Behind every row's ds_plan_row: 16 lanes per row move feature vectors as float4 -- the packet's features into the stream's
// ring when their hop does not start in this call, and the features of the hop that starts (the ring's oldest, or
// ZeroFeatureEstimator's 64 x 0.0f) into the row the decoder chain reads.  A packet whose hop starts in this same call never
// goes through the ring.
__device__ __forceinline__ void ds_plan_move(const DsPlanLds& sh, int tid, int b0, int B, float* __restrict__ feats,
                                             float* __restrict__ ring) {
  __syncthreads();
  const int rows = min(256, B - b0), q = tid & 15;
  for (int r = tid >> 4; r < rows; r += 16) {
    const int push = sh.push[r], src = sh.src[r];
    float4* row = reinterpret_cast<float4*>(feats + (size_t)(b0 + r) * 64);
    float4* slots = reinterpret_cast<float4*>(ring + (size_t)sh.id[r] * DS_FIFO_DEPTH * 64);
    if (push >= 0) slots[push * 16 + q] = row[q];          // (push != src: the ring was not empty)
    if (src == DS_SRC_ZERO) row[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    else if (src >= 0) row[q] = slots[src * 16 + q];
  }
}

// rs_fir's destination (`dst[i] = v`, resample_pass.h) in ds_splice_row: the first n_new resampled samples to the caller's row behind
// the old leftover, the surplus (at most DSA_LEFT_MAX) to the slot's leftover; anything beyond is dropped.
struct SpliceDst {
  int16_t* row; int16_t* left; int n_new;
  struct Ref {
    int16_t* p;
    __device__ void operator=(int16_t v) const { if (p) *p = v; }
  };
  __device__ Ref operator[](int i) const {
    const int j = i - n_new;
    return Ref{j < 0 ? row + i : j < DSA_LEFT_MAX ? left + j : nullptr};
  }
};

// One wavefront, one row at 8 / 32 / 48 kHz: the row's n_int internal samples (cw.z, 0..1280, at src) run through the stream's
// resampler (slot `id` of the region `state`) as resample_kernel's do (rs_stream_pass, resample_pass.h: same taps, same separately rounded
// products, same history and phase write-back); row = the old leftover's first `used` samples (cw.y), then the new ones; the
// surplus becomes the stream's leftover.  Counts come from the call words cw alone (the slot's count may already be the next
// call's).  A row with n_int == 0 touches no resampler state: it serves from the leftover and moves what remains to the front.
// Rows are of any length and alignment, so samples move one int16 at a time.  rsb is the wavefront's own LDS row: no workgroup
// barrier, the order of its writes and reads is pinned by wavefront fences.
__device__ __forceinline__ void ds_splice_row(const ResampleP& P, float* rsb, int lane, int4 cw, uint8_t* state, int id,
                                              const int16_t* __restrict__ src, int16_t* __restrict__ row, int n_ext) {
  const int used = __builtin_amdgcn_readfirstlane(cw.y);
  const int n_in = min(__builtin_amdgcn_readfirstlane(cw.z), DSA_MAX_INTERNAL);
  int16_t* left = reinterpret_cast<int16_t*>(state + (size_t)id * st::RS_BYTES + DSA_LEFT_SAMPLES);
  int16_t keep = 0;
  if (lane < DSA_LEFT_MAX) keep = left[lane];
  if (lane < used) row[lane] = keep;
  if (n_in == 0) {   // (wave-uniform) n <= old count: what was not served moves to the front
    const int16_t next = (int16_t)__shfl_down((int)keep, used);
    if (used > 0 && lane < DSA_LEFT_MAX) left[lane] = lane + used < DSA_LEFT_MAX ? next : (int16_t)0;
    return;
  }
  const int n_out = n_in / P.down;   // (down-sampling: n_in is even and the phase 0, decode_samples_any_plan.h)
  rs_stream_pass<false, SpliceDst>(&P, rsb, lane, state, id, src, n_in, false, SpliceDst{row + used, left, n_ext - used}, n_out);
  if (lane < DSA_LEFT_MAX && lane >= cw.w) left[lane] = 0;   // (the FIR wrote the cw.w samples that stay)
}

// the wavefront's row of the splice kernels' LDS: [4][RS_TAPS - 1 + 1280, padded to 4] floats (ds_splice_lds_bytes)
__device__ __forceinline__ float* ds_splice_lds_row(float* rsb_all, int w) {
  return rsb_all + w * ((st::RS_TAPS - 1 + DSA_MAX_INTERNAL + 3) & ~3);
}

}  // namespace lyra
