// spans_packed_kernels.hip -- the span calls with a sample rate per span on a PACKED external-rate buffer
// (include/lyra_hip_spans_packed.h; api.hip, spans_packed_api.inc).  span_resample_rates_kernel (spans_rates_kernels.hip) with
// one difference: the external-rate buffer is one flat array of samples, span s's frames back to back from a base, each
// rate / 50 samples long, instead of rows padded to a stride.  The 16 kHz side, the designs, the slots and the arithmetic
// (rs_span_pass, resample_pass.h) are that kernel's, so per frame the output is bit for bit the padded kernel's.
#include "kernels.h"
#include "resample_pass.h"

namespace lyra {

namespace {
__device__ __forceinline__ i32x4 ld16(const void* p) { return *reinterpret_cast<const i32x4*>(p); }
__device__ __forceinline__ void st16(void* p, i32x4 v) { *reinterpret_cast<i32x4*>(p) = v; }
}  // namespace

// dir 0: in = the flat external-rate buffer, out = the 16 kHz buffer [frames][320]; dir 1 the reverse.
// One wavefront per frame, four frames of ONE span per workgroup; LDS rows sized for the 48 kHz hop (resample_rates_lds_bytes()).
//   the span's base    SpanRsRow::pad[1] * 8 samples (the host refuses a base that is no multiple of 8 or does not fit the
//                      word): frame f of the span lies at base + f * (rate / 50), in 64-bit arithmetic.  Rows are 160 / 320 /
//                      640 / 960 samples long, so every row is 16-byte aligned in a 16-byte aligned buffer and the vector path
//                      of rs_load holds.  The 16 kHz side is indexed by buffer frame (row.frame0 + f) as ever.
//   frame f > 0        on the external side the FIR's history is the 34 samples directly in front of the row: frame f - 1's
//                      last, contiguous.  On the 16 kHz side rows are 320 apart and 320 long: the same.
//   frame 0 of a span  history from the span stream's slot -- never from the buffer: in a packed buffer the samples in front of a
//                      span are another span's, at another rate -- and the only wavefront that writes the slot: the span's last
//                      34 input samples and the phase word.
//   the phase          as in span_resample_rates_kernel: later frames read the word the frame-0 wavefront may be replacing; old
//                      and new value differ by a multiple of n_in, n_in is a multiple of down and down divides 6, so `first`
//                      (rs_fir) is the same from either.
//   16 kHz             320 samples per frame are copied, no slot is read or written.
//   decode             a span writes n_frames * (rate / 50) samples from its base: nothing in front, behind or between spans.
__global__ __launch_bounds__(256) void span_resample_packed_kernel(const ResampleP* __restrict__ tab, int dir,
                                                                    const SpanRsRow* __restrict__ rows, int n_rows,
                                                                    uint8_t* __restrict__ state, const int16_t* __restrict__ in,
                                                                    int16_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float rsb_all[];   // [4][RS_TAPS - 1 + 960, padded to 4]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const SpanRsRow row = rows[span_row_of_workgroup(rows, n_rows, &SpanRsRow::wg0, (int)blockIdx.x)];
  const long long f = ((long long)blockIdx.x - row.wg0) * 4 + w;   // frame of the span
  if (f >= row.n_frames) return;   // (wave-uniform)
  const int rate = row.pad[0];
  const int di = rs_design_index(rate);
  const int n_ext = rate / 50;
  const long long at_ext = (long long)row.pad[1] * 8 + f * n_ext, at16 = (row.frame0 + f) * 320;   // in samples
  const int16_t* src = in + (dir == 0 ? at_ext : at16);
  int16_t* dst = out + (dir == 0 ? at16 : at_ext);
  if (di < 0) {   // (workgroup-uniform; the host refuses every value that is no codec rate)
    if (lane < 40) st16(dst + lane * 8, ld16(src + lane * 8));
    return;
  }
  const int n_in = dir == 0 ? n_ext : 320, n_out = dir == 0 ? 320 : n_ext;
  // rows of 160 / 320 / 640 / 960 samples from a base that is a multiple of 8, in a 16-byte aligned buffer; f > 0: the samples in
  // front of src are the end of row f - 1 of this span, on either side; f == 0: src is the span's first row (n_in > RS_H)
  rs_span_pass(tab + dir * 3 + di, rsb_all + w * ((RS_H + 960 + 3) & ~3), lane, state + (size_t)row.id * st::RS_BYTES, f,
               row.n_frames, src, src - RS_H, src + row.n_frames * n_in - RS_H, n_in, dst, n_out);
}

}  // namespace lyra
