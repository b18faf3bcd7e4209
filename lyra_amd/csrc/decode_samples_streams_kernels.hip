// decode_samples_streams_kernels.hip -- the two kernels of lyra_hip_decode_samples_streams_dev
// (decode_samples_streams_api.inc) that read what lyra_hip_decode_samples_any_dev's take as launch constants: the request size,
// the sample rate and the place of the output, here one of each PER ROW (decode_samples_streams_plan.h).  They are
// ds_plan_any_kernel and ds_splice_kernel (decode_samples_any_kernels.hip) with those three read per row and with the row
// verdict in front; those kernels are not edited, so the uniform call cannot change.
#include "kernels.h"
#include "decode_samples_streams_plan.h"

namespace lyra {

// ds_plan_any_kernel with n_ext, rate and the offset check per row.  Round 0 validates the row (dss_row_verdict), derives
// its totals from its leftover count, advances the count, delivers the packet and leaves DSS_CALL_WORDS words in call[b];
// a row that fails is planned as one without a packet and with a request of 0 samples -- its leftover count is not even
// rewritten -- and is counted once in *rates_err.  Later rounds (pkt_bytes == nullptr) read call[b] only.
__global__ __launch_bounds__(256) void ds_plan_streams_kernel(const int32_t* __restrict__ ids, int B,
                                                               const int32_t* __restrict__ pkt_bytes, int round,
                                                               const int32_t* __restrict__ rates,
                                                               const int32_t* __restrict__ num_samples,
                                                               const int32_t* __restrict__ offsets, int max_hops,
                                                               long n_pcm_samples, uint8_t* __restrict__ rs_state, int32_t* call,
                                                               uint8_t* __restrict__ cng_state, int32_t* __restrict__ gen_ids,
                                                               int32_t* __restrict__ cng1_ids, int32_t* __restrict__ cng2_ids,
                                                               int32_t* __restrict__ est_ids, int32_t* __restrict__ info,
                                                               float* __restrict__ feats, float* __restrict__ ring,
                                                               unsigned* __restrict__ err, unsigned* __restrict__ rates_err) {
  __shared__ int sh_id[256], sh_push[256], sh_src[256];
  const int tid = threadIdx.x, b0 = blockIdx.x * 256, b = b0 + tid;
  int nerr = 0, ninvalid = 0;
  sh_push[tid] = -1;
  sh_src[tid] = DS_SRC_NONE;
  if (b < B) {
    const int id = ids[b];
    int pb = 0, n_int;
    int32_t* cw = call + (size_t)b * DSS_CALL_WORDS;
    if (round == 0) {
      const int rate = rates[b], n_ext = num_samples[b];
      const long off = offsets ? (long)offsets[b] : dss_default_offset(b);
      const int verdict = dss_row_verdict(rate, n_ext, max_hops, off, n_pcm_samples);
      int* cnt = reinterpret_cast<int*>(rs_state + (size_t)id * st::RS_BYTES + DSA_LEFT_COUNT);
      int left = *cnt;
      left = left < 0 ? 0 : left > DSA_LEFT_MAX ? DSA_LEFT_MAX : left;   // (sb::validate holds imported counts to the domain)
      DsaStep s = {0, 0, left};
      if (verdict == DSS_OK) {
        pb = pkt_bytes[b];
        s = ds_any_step(left, n_ext, rate);
        *cnt = s.left;
      } else {
        ninvalid = 1;
      }
      n_int = s.n_int;
      *reinterpret_cast<int4*>(cw) = make_int4(left, s.used, s.n_int, s.left);
      *reinterpret_cast<int4*>(cw + 4) = make_int4(verdict, verdict == DSS_OK ? n_ext : 0, rate, 0);
    } else {
      n_int = cw[2];
    }
    const bool rx = mixed_received(pb);
    if (pb != 0 && !rx) nerr++;
    DsState* sp = reinterpret_cast<DsState*>(cng_state + (size_t)id * st::CNG_BYTES + DS_STATE);
    const DsPlan p = ds_plan(*sp, rx, ds_any_round_total(n_int, round));
    if (!ninvalid) *sp = p.s;   // (an invalid row's plan changes nothing: no packet, no samples)
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
  const unsigned long long bad = __ballot((nerr | ninvalid) != 0);
  if (bad) {   // (wave-uniform)
    int n = nerr, m = ninvalid;
    for (int o = 32; o > 0; o >>= 1) {
      n += __shfl_down(n, o);
      m += __shfl_down(m, o);
    }
    if ((tid & 63) == 0) {
      if (n) atomicAdd(err, (unsigned)n);
      if (m) atomicAdd(rates_err, (unsigned)m);
    }
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

// resample_fir.inc's `dst[i] = v` in ds_splice_streams_kernel (SpliceDst of ds_splice_kernel): the first n_new resampled
// samples to the caller's row behind the old leftover, the surplus (at most DSA_LEFT_MAX) to the slot's leftover.
struct SpliceStreamsDst {
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

size_t ds_splice_streams_lds_bytes() { return (size_t)4 * ((st::RS_TAPS - 1 + DSA_MAX_INTERNAL + 3) & ~3) * 4; }

// The end of the call: one wavefront per row, four rows per workgroup, ds_splice_kernel's LDS.  The row's words come from
// call[b] (the plan kernel validated it: nothing of an invalid row is read or written here).  A row at 8 / 32 / 48 kHz takes
// its design from tab (rates_api.inc: [3 + {8000, 32000, 48000}] = 16 kHz -> rate, the floats the uniform call passes by
// value) and runs ds_splice_kernel's text over its n_int samples: old leftover + new samples to out + offset, surplus to the
// slot.  A 16 kHz row has no resampler and no leftover: its n samples are copied from the internal-rate row.  Offsets have
// no alignment, so samples are written one int16 at a time.  Every branch on the row's words is wave-uniform.
__global__ __launch_bounds__(256) void ds_splice_streams_kernel(const ResampleP* __restrict__ tab,
                                                                 const int32_t* __restrict__ ids, int B,
                                                                 const int32_t* __restrict__ call, uint8_t* __restrict__ state,
                                                                 const int16_t* __restrict__ in, int in_stride,
                                                                 int16_t* __restrict__ out, const int32_t* __restrict__ offsets) {
  extern __shared__ __attribute__((aligned(16))) float rsb_all[];   // [4][RS_TAPS - 1 + 1280, padded to 4]
  constexpr int H = st::RS_TAPS - 1;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x * 4 + w;
  if (b >= B) return;
  const int4 cw = *reinterpret_cast<const int4*>(call + (size_t)b * DSS_CALL_WORDS);
  const int4 rw = *reinterpret_cast<const int4*>(call + (size_t)b * DSS_CALL_WORDS + 4);
  const int n_ext = __builtin_amdgcn_readfirstlane(rw.y);
  const int rate = __builtin_amdgcn_readfirstlane(rw.z);
  if (__builtin_amdgcn_readfirstlane(rw.x) != DSS_OK || n_ext == 0) return;   // (an invalid row carries n == 0 as well)
  const long off = offsets ? (long)__builtin_amdgcn_readfirstlane(offsets[b]) : dss_default_offset(b);
  int16_t* row = out + off;
  const int16_t* src = in + (size_t)b * in_stride;
  const int di = rate == 8000 ? 0 : rate == 32000 ? 1 : rate == 48000 ? 2 : -1;
  if (di < 0) {   // 16 kHz: the samples themselves
    for (int i = lane; i < n_ext; i += 64) row[i] = src[i];
    return;
  }
  const int used = __builtin_amdgcn_readfirstlane(cw.y);
  const int n_in = min(__builtin_amdgcn_readfirstlane(cw.z), DSA_MAX_INTERNAL);
  uint8_t* slot = state + (size_t)ids[b] * st::RS_BYTES;
  int16_t* left = reinterpret_cast<int16_t*>(slot + DSA_LEFT_SAMPLES);
  int16_t keep = 0;
  if (lane < DSA_LEFT_MAX) keep = left[lane];
  if (lane < used) row[lane] = keep;
  if (n_in == 0) {   // n <= old count: what was not served moves to the front
    const int16_t next = (int16_t)__shfl_down((int)keep, used);
    if (used > 0 && lane < DSA_LEFT_MAX) left[lane] = lane + used < DSA_LEFT_MAX ? next : (int16_t)0;
    return;
  }
  const ResampleP& P = tab[3 + di];
  float* rsb = rsb_all + w * ((H + DSA_MAX_INTERNAL + 3) & ~3);
  const bool vec = false;
#include "resample_load.inc"
  float* hist = reinterpret_cast<float*>(slot + st::RS_HIST);
  const int in_pos = *reinterpret_cast<const int*>(slot + st::RS_IN_POS);
  if (lane < H) rsb[lane] = hist[lane];
  // (as in ds_splice_kernel: a wavefront reads only the LDS row it wrote; the order is pinned rather than assumed)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int n_out = n_in / P.down;   // (down-sampling: n_in is even and the phase 0, decode_samples_any_plan.h)
  const SpliceStreamsDst dst{row + used, left, n_ext - used};
#include "resample_fir.inc"
#include "resample_slot.inc"
  if (lane < DSA_LEFT_MAX && lane >= cw.w) left[lane] = 0;   // (the FIR wrote the cw.w samples that stay)
}

}  // namespace lyra
