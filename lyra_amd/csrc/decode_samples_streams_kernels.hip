// decode_samples_streams_kernels.hip -- the two kernels of lyra_hip_decode_samples_streams_dev
// (decode_samples_streams_api.inc) that read what lyra_hip_decode_samples_any_dev's take as launch constants: the request size,
// the sample rate and the place of the output, here one of each PER ROW (decode_samples_streams_plan.h).  They are
// ds_plan_any_kernel and ds_splice_kernel (decode_samples_any_kernels.hip) with those three read per row and with the row
// verdict in front; a row's plan and a row's splice are one text for both (decode_samples_rows.h), pinned bit for bit by
// tests/test_gpu_decode_samples_streams.py against the uniform call.
#include "kernels.h"
#include "decode_samples_streams_plan.h"
#include "decode_samples_rows.h"

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
  __shared__ DsPlanLds sh;
  const int tid = threadIdx.x, b0 = blockIdx.x * 256, b = b0 + tid;
  int nerr = 0, ninvalid = 0;
  ds_plan_lds_clear(sh, tid);
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
    // (an invalid row's plan changes nothing: no packet, no samples)
    ds_plan_row(sh, tid, b, id, rx, ds_any_round_total(n_int, round), !ninvalid, nerr, cng_state, gen_ids, cng1_ids, cng2_ids,
                est_ids, info);
  }
  ds_wave_count(nerr, err, tid);
  ds_wave_count(ninvalid, rates_err, tid);
  ds_plan_move(sh, tid, b0, B, feats, ring);
}

// The end of the call: one wavefront per row, four rows per workgroup, ds_splice_kernel's LDS.  The row's words come from
// call[b] (the plan kernel validated it: nothing of an invalid row is read or written here).  A row at 8 / 32 / 48 kHz takes
// its design from tab (rates_api.inc: [3 + {8000, 32000, 48000}] = 16 kHz -> rate, the floats the uniform call passes by
// value) and runs ds_splice_row over its n_int samples: old leftover + new samples to out + offset, surplus to the
// slot.  A 16 kHz row has no resampler and no leftover: its n samples are copied from the internal-rate row.  Offsets have
// no alignment, so samples are written one int16 at a time.  Every branch on the row's words is wave-uniform.
__global__ __launch_bounds__(256) void ds_splice_streams_kernel(const ResampleP* __restrict__ tab,
                                                                 const int32_t* __restrict__ ids, int B,
                                                                 const int32_t* __restrict__ call, uint8_t* __restrict__ state,
                                                                 const int16_t* __restrict__ in, int in_stride,
                                                                 int16_t* __restrict__ out, const int32_t* __restrict__ offsets) {
  extern __shared__ __attribute__((aligned(16))) float rsb_all[];   // [4][RS_TAPS - 1 + 1280, padded to 4]
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
  const int di = rs_design_index(rate);
  if (di < 0) {   // 16 kHz: the samples themselves
    for (int i = lane; i < n_ext; i += 64) row[i] = src[i];
    return;
  }
  ds_splice_row(tab[3 + di], ds_splice_lds_row(rsb_all, w), lane, cw, state, ids[b], src, row, n_ext);
}

}  // namespace lyra
