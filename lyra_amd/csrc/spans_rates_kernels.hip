// spans_rates_kernels.hip -- the span calls with a sample rate per span (include/lyra_hip_spans_rates.h; api.hip,
// spans_rates_api.inc).  The steps of a span call run at 16 kHz and never see the external rate, so what a rate per span changes is
// the passes that go once over every frame in front of the steps or behind them: the resampler, and under DTX the encoder-side
// NoiseEstimator.  Each is its uniform kernel with the design, the filterbank or the constants looked up per ROW (= per span with
// frames) instead of passed per call.  A workgroup never holds frames of two spans, so the rate is workgroup-uniform, the lookup is
// scalar work and the coefficients stay scalar operands.  The row's rate rides in SpanRsRow::pad[0]; the estimator's kernels read it
// from the resampler's row of the same index (both lists hold one row per span with frames, in the order of the call's spans).
//   span_resample_rates_kernel    span_resample_kernel; rows of the external-rate buffer are padded to a stride
//   span_logmel_rates_kernel      span_logmel_kernel (both call span_logmel_row, logmel_stages.h)
//   span_noise_scan_rates_kernel  span_noise_scan_kernel (both call span_dtx_scan, span_noise_scan.h)
#include "kernels.h"
#include "logmel_stages.h"
#include "resample_pass.h"
#include "span_noise_scan.h"

namespace lyra {

namespace {
__device__ __forceinline__ i32x4 ld16(const void* p) { return *reinterpret_cast<const i32x4*>(p); }
__device__ __forceinline__ void st16(void* p, i32x4 v) { *reinterpret_cast<i32x4*>(p) = v; }
}  // namespace

// dir 0: in = the external-rate buffer (rows in_stride samples apart, rate / 50 valid samples at the front of each), out = the
// 16 kHz buffer (out_stride = 320); dir 1 the reverse.  One wavefront per frame, four frames of ONE span per workgroup, as
// span_resample_kernel; LDS rows are sized for the 48 kHz hop (resample_rates_lds_bytes()).
//   padded rows        the FIR's history of frame f > 0 is the last 34 VALID samples of the row in front, at
//                      (f - 1) * in_stride + n_in - 34: with a stride wider than n_in they are not the 34 int16 in front of
//                      the row pointer.  The span's last 34 samples, which become the slot's history, move the same way.
//                      (in_stride == n_in on the 16 kHz side: there both rules name the same samples.)
//   frame 0 of a span  history from the span stream's slot -- never from the buffer, the row in front may be another span's,
//                      at another rate -- and the only wavefront that writes the slot.
//   the phase          later frames read the slot's phase word, which the frame-0 wavefront may be replacing meanwhile.  Old
//                      and new value differ by a multiple of n_in, and `first` (rs_fir, resample_pass.h) depends on in_pos % down
//                      alone.  Per design: 8000 -> 16000 and 16000 -> 32000 / 48000 interpolate (down = 1, the word is not
//                      read); 32000 -> 16000: n_in = 640, down = 2; 48000 -> 16000: n_in = 960, down = 3; 16000 -> 8000:
//                      n_in = 320, down = 2.  In each n_in is a multiple of down, and down divides 6, the modulus the word
//                      is kept in -- so `first` is the same from either value.
//   16 kHz             the row is copied (320 samples), no slot is read or written.
__global__ __launch_bounds__(256) void span_resample_rates_kernel(const ResampleP* __restrict__ tab, int dir,
                                                                   const SpanRsRow* __restrict__ rows, int n_rows,
                                                                   uint8_t* __restrict__ state, const int16_t* __restrict__ in,
                                                                   int in_stride, int16_t* __restrict__ out, int out_stride) {
  extern __shared__ __attribute__((aligned(16))) float rsb_all[];   // [4][RS_TAPS - 1 + 960, padded to 4]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const SpanRsRow row = rows[span_row_of_workgroup(rows, n_rows, &SpanRsRow::wg0, (int)blockIdx.x)];
  const long long f = ((long long)blockIdx.x - row.wg0) * 4 + w;   // frame of the span
  if (f >= row.n_frames) return;   // (wave-uniform)
  const int rate = row.pad[0];
  const int di = rs_design_index(rate);
  const int16_t* src = in + (size_t)(row.frame0 + f) * in_stride;
  int16_t* dst = out + (size_t)(row.frame0 + f) * out_stride;
  if (di < 0) {   // (workgroup-uniform; the host refuses every value that is no codec rate)
    if (lane < 40) st16(dst + lane * 8, ld16(src + lane * 8));
    return;
  }
  const int n_ext = rate / 50;
  const int n_in = dir == 0 ? n_ext : 320, n_out = dir == 0 ? 320 : n_ext;
  // rows of 160 / 320 / 640 / 960 samples, strides of 320 / 960, in a 16-byte aligned buffer; f > 0: src - in_stride is row
  // f - 1 of this span; n_in > RS_H
  rs_span_pass(tab + dir * 3 + di, rsb_all + w * ((RS_H + 960 + 3) & ~3), lane, state + (size_t)row.id * st::RS_BYTES, f,
               row.n_frames, src, src - in_stride + n_in - RS_H,
               in + (size_t)(row.frame0 + row.n_frames - 1) * in_stride + n_in - RS_H, n_in, dst, n_out);
}

// span_logmel_kernel with the filterbank of the row's rate: P4 = the four rates' MelP (model.h d_mel_rate[0], the table
// logmel_rates_kernel indexes).  Both frames of a workgroup are one span's, so one filterbank serves the workgroup.
__global__ __launch_bounds__(256) void span_logmel_rates_kernel(const MelP* __restrict__ P4, const SpanDtxRow* __restrict__ rows,
                                                                 const SpanRsRow* __restrict__ rate_rows, int n_rows,
                                                                 uint8_t* __restrict__ state, const int16_t* __restrict__ pcm,
                                                                 float* __restrict__ mel) {
  const int r = span_row_of_workgroup(rows, n_rows, &SpanDtxRow::wg0, (int)blockIdx.x);
  span_logmel_row(P4[mel_rate_index(rate_rows[r].pad[0])], rows[r], (int)blockIdx.x, state, pcm, mel);
}

// span_noise_scan_kernel with the constants of the row's rate: np_tab = the four rates' NoiseP (rates_ensure's d_noise_tab).
__global__ __launch_bounds__(64) void span_noise_scan_rates_kernel(const NoiseP* __restrict__ np_tab,
                                                                    const SpanDtxRow* __restrict__ rows,
                                                                    const SpanRsRow* __restrict__ rate_rows, int n_rows,
                                                                    uint8_t* __restrict__ state, const float* __restrict__ mel,
                                                                    int32_t* __restrict__ flag_out, int v_noise, int v_active,
                                                                    long long* __restrict__ map, int32_t* __restrict__ counts) {
  if ((int)blockIdx.x >= n_rows) return;
  span_dtx_scan(np_tab[mel_rate_index(rate_rows[blockIdx.x].pad[0])], rows, state, mel, flag_out, v_noise, v_active, map, counts);
}

}  // namespace lyra
