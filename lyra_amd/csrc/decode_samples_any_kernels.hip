// decode_samples_any_kernels.hip -- what lyra_hip_decode_samples_any_dev (decode_samples_any_api.inc) adds to the kernels of
// lyra_hip_decode_samples_dev: the plan of one ROUND of a request of up to four hops, with the internal length per row
// (BufferedResampler's leftover differs from row to row, decode_samples_any_plan.h), and the kernel that ends the call at
// 8 / 32 / 48 kHz: resampler over a per-row length, old leftover + new samples to the caller's row, surplus to the slot.
#include "kernels.h"
#include "decode_samples_any_plan.h"

namespace lyra {

// ds_plan_kernel for round `round` of a call.  Round 0 reads the row's leftover count from its R_RS_D slot, derives the call's
// totals (ds_any_step), ADVANCES the count -- the next call plans on this stream before this call's samples exist -- and
// leaves {old count, used, n_int, new count} in call[b]: every later kernel of the call, the noise-stream ones above all,
// reads these words and never the slot.  Later rounds read n_int from call[b]; they carry no packet (pkt_bytes == nullptr).
// A row whose rounds are over plans a total of 0: no pass, no hop, state unchanged.
__global__ __launch_bounds__(256) void ds_plan_any_kernel(const int32_t* __restrict__ ids, int B,
                                                           const int32_t* __restrict__ pkt_bytes, int round, int n_ext,
                                                           int rate, uint8_t* __restrict__ rs_state, int32_t* call,
                                                           uint8_t* __restrict__ cng_state, int32_t* __restrict__ gen_ids,
                                                           int32_t* __restrict__ cng1_ids, int32_t* __restrict__ cng2_ids,
                                                           int32_t* __restrict__ est_ids, int32_t* __restrict__ info,
                                                           float* __restrict__ feats, float* __restrict__ ring,
                                                           unsigned* __restrict__ err) {
  __shared__ int sh_id[256], sh_push[256], sh_src[256];
  const int tid = threadIdx.x, b0 = blockIdx.x * 256, b = b0 + tid;
  int nerr = 0;
  sh_push[tid] = -1;
  sh_src[tid] = DS_SRC_NONE;
  if (b < B) {
    const int id = ids[b];
    const int pb = pkt_bytes ? pkt_bytes[b] : 0;
    const bool rx = mixed_received(pb);
    if (pb != 0 && !rx) nerr++;
    int n_int;
    if (round == 0) {
      int* cnt = reinterpret_cast<int*>(rs_state + (size_t)id * st::RS_BYTES + DSA_LEFT_COUNT);
      int left = *cnt;
      left = left < 0 ? 0 : left > DSA_LEFT_MAX ? DSA_LEFT_MAX : left;   // (sb::validate holds imported counts to the domain)
      const DsaStep s = ds_any_step(left, n_ext, rate);
      *cnt = s.left;
      n_int = s.n_int;
      *reinterpret_cast<int4*>(call + (size_t)b * 4) = make_int4(left, s.used, s.n_int, s.left);
    } else {
      n_int = call[(size_t)b * 4 + 2];
    }
    DsState* sp = reinterpret_cast<DsState*>(cng_state + (size_t)id * st::CNG_BYTES + DS_STATE);
    const DsPlan p = ds_plan(*sp, rx, ds_any_round_total(n_int, round));
    *sp = p.s;
    nerr += p.dropped + p.bad;
    gen_ids[b] = p.gen_start >= 0 ? id : -1;
    cng1_ids[b] = p.cng_start == 0 ? id : -1;
    cng2_ids[b] = p.cng_start == 1 ? id : -1;
    est_ids[b] = p.est_seg >= 0 ? id : -1;
    int32_t w[4];
    ds_info(p, w);
    *reinterpret_cast<int4*>(info + (size_t)b * 4) = make_int4(w[0], w[1], w[2], w[3]);
    const bool direct = p.push_slot >= 0 && p.gen_src == p.push_slot;   // this call's packet starts its hop at once
    sh_id[tid] = id;
    sh_push[tid] = direct ? -1 : p.push_slot;
    sh_src[tid] = direct ? DS_SRC_NONE : p.gen_src;
  }
  const unsigned long long bad = __ballot(nerr != 0);
  if (bad) {   // (wave-uniform)
    int n = nerr;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o);
    if ((tid & 63) == 0) atomicAdd(err, (unsigned)n);
  }
  __syncthreads();
  const int rows = min(256, B - b0), q = tid & 15;
  for (int r = tid >> 4; r < rows; r += 16) {
    const int push = sh_push[r], src = sh_src[r];
    float4* row = reinterpret_cast<float4*>(feats + (size_t)(b0 + r) * 64);
    float4* slots = reinterpret_cast<float4*>(ring + (size_t)sh_id[r] * DS_FIFO_DEPTH * 64);
    if (push >= 0) slots[push * 16 + q] = row[q];          // (push != src: the ring was not empty)
    if (src == DS_SRC_ZERO) row[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    else if (src >= 0) row[q] = slots[src * 16 + q];
  }
}

// Where resample_fir.inc's `dst[i] = v` goes in ds_splice_kernel: the first n_new resampled samples to the caller's row behind
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

size_t ds_splice_lds_bytes() { return (size_t)4 * ((st::RS_TAPS - 1 + DSA_MAX_INTERNAL + 3) & ~3) * 4; }

// The end of a call at 8 / 32 / 48 kHz: one wavefront per row, four rows per workgroup.  Row b's n_int internal samples
// (call[b][2], 0..1280, at in + b * in_stride) run through the stream's resampler with the text of resample_kernel
// (resample_fir.inc, resample_slot.inc: same taps, same separately rounded products, same history and phase write-back);
// out[b] = the old leftover's first `used` samples, then the new ones; the surplus becomes the stream's leftover.  Counts
// come from call[b] alone (the slot's count may already be the next call's).  A row with n_int == 0 touches no resampler
// state: it serves from the leftover and moves what remains to the front.  Rows are of any length, so the samples are read
// one int16 at a time.  No workgroup barrier: a wavefront reads only the LDS row it wrote.
__global__ __launch_bounds__(256) void ds_splice_kernel(ResampleP P, const int32_t* __restrict__ ids, int B,
                                                         const int32_t* __restrict__ call, uint8_t* __restrict__ state,
                                                         const int16_t* __restrict__ in, int in_stride,
                                                         int16_t* __restrict__ out, int n_ext) {
  extern __shared__ __attribute__((aligned(16))) float rsb_all[];   // [4][RS_TAPS - 1 + 1280, padded to 4]
  constexpr int H = st::RS_TAPS - 1;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x * 4 + w;
  if (b >= B) return;
  const int4 cw = *reinterpret_cast<const int4*>(call + (size_t)b * 4);
  const int used = __builtin_amdgcn_readfirstlane(cw.y);
  const int n_in = min(__builtin_amdgcn_readfirstlane(cw.z), DSA_MAX_INTERNAL);
  uint8_t* slot = state + (size_t)ids[b] * st::RS_BYTES;
  int16_t* left = reinterpret_cast<int16_t*>(slot + DSA_LEFT_SAMPLES);
  int16_t* row = out + (size_t)b * n_ext;
  int16_t keep = 0;
  if (lane < DSA_LEFT_MAX) keep = left[lane];
  if (lane < used) row[lane] = keep;
  if (n_in == 0) {   // (wave-uniform) n <= old count: what was not served moves to the front
    const int16_t next = (int16_t)__shfl_down((int)keep, used);
    if (used > 0 && lane < DSA_LEFT_MAX) left[lane] = lane + used < DSA_LEFT_MAX ? next : (int16_t)0;
    return;
  }
  float* rsb = rsb_all + w * ((H + DSA_MAX_INTERNAL + 3) & ~3);
  const int16_t* src = in + (size_t)b * in_stride;
  const bool vec = false;
#include "resample_load.inc"
  float* hist = reinterpret_cast<float*>(slot + st::RS_HIST);
  const int in_pos = *reinterpret_cast<const int*>(slot + st::RS_IN_POS);
  if (lane < H) rsb[lane] = hist[lane];
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int n_out = n_in / P.down;   // (down-sampling: n_in is even and the phase 0, decode_samples_any_plan.h)
  const SpliceDst dst{row + used, left, n_ext - used};
#include "resample_fir.inc"
#include "resample_slot.inc"
  if (lane < DSA_LEFT_MAX && lane >= cw.w) left[lane] = 0;   // (the FIR wrote the cw.w samples that stay)
}

}  // namespace lyra
