// decode_samples_any_kernels.hip -- what lyra_hip_decode_samples_any_dev (decode_samples_any_api.inc) adds to the kernels of
// lyra_hip_decode_samples_dev: the plan of one ROUND of a request of up to four hops, with the internal length per row
// (BufferedResampler's leftover differs from row to row, decode_samples_any_plan.h), and the kernel that ends the call at
// 8 / 32 / 48 kHz: resampler over a per-row length, old leftover + new samples to the caller's row, surplus to the slot.
// Both kernels are heads in front of the bodies the three calls share (decode_samples_rows.h).
#include "kernels.h"
#include "decode_samples_rows.h"

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
  __shared__ DsPlanLds sh;
  const int tid = threadIdx.x, b0 = blockIdx.x * 256, b = b0 + tid;
  int nerr = 0;
  ds_plan_lds_clear(sh, tid);
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
    ds_plan_row(sh, tid, b, id, rx, ds_any_round_total(n_int, round), true, nerr, cng_state, gen_ids, cng1_ids, cng2_ids, est_ids,
                info);
  }
  ds_wave_count(nerr, err, tid);
  ds_plan_move(sh, tid, b0, B, feats, ring);
}

// the dynamic LDS of ds_splice_kernel and ds_splice_streams_kernel (ds_splice_lds_row)
size_t ds_splice_lds_bytes() { return (size_t)4 * ((st::RS_TAPS - 1 + DSA_MAX_INTERNAL + 3) & ~3) * 4; }

// The end of a call at 8 / 32 / 48 kHz: one wavefront per row, four rows per workgroup.  Row b's n_int internal samples
// (call[b][2], at in + b * in_stride) go through ds_splice_row (decode_samples_rows.h) to out + b * n_ext.
__global__ __launch_bounds__(256) void ds_splice_kernel(ResampleP P, const int32_t* __restrict__ ids, int B,
                                                         const int32_t* __restrict__ call, uint8_t* __restrict__ state,
                                                         const int16_t* __restrict__ in, int in_stride,
                                                         int16_t* __restrict__ out, int n_ext) {
  extern __shared__ __attribute__((aligned(16))) float rsb_all[];   // [4][RS_TAPS - 1 + 1280, padded to 4]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x * 4 + w;
  if (b >= B) return;
  const int4 cw = *reinterpret_cast<const int4*>(call + (size_t)b * 4);
  ds_splice_row(P, ds_splice_lds_row(rsb_all, w), lane, cw, state, ids[b], in + (size_t)b * in_stride,
                out + (size_t)b * n_ext, n_ext);
}

}  // namespace lyra
