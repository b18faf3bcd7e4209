// spans_kernels.hip -- lyra_hip_encode_spans_dev / lyra_hip_decode_spans_dev (api.hip, spans_api.inc; plan: spans_plan.h): the
// row movement of a step and the hand-over of a time-parallel transcode.  The stage kernels and the quantizer read and write
// dense [B][.] rows; the caller's buffers are frame-major.  Per step one gather in front of the stages and, on steps that
// produce, one scatter behind them; all step-dependent decisions are taken here from the rows' plan and the step number, so the
// host enqueues the whole call from one upload.  Pure data movement: 16-byte units for PCM rows (640 bytes), bytes for packet
// rows (8 / 15 / 23 bytes, unaligned by nature); consecutive lanes move consecutive units of a row, rows are contiguous in
// the dense buffer.  Every access is guarded by the row count of the step and the row's own step range.
// The one kernel here that computes is span_resample_kernel at the end: the spans' resampler at 8 / 32 / 48 kHz, one launch per call.
#include "kernels.h"
#include "resample_pass.h"

namespace lyra {

__device__ __forceinline__ i32x4 ld16(const uint8_t* p) { return *reinterpret_cast<const i32x4*>(p); }
__device__ __forceinline__ void st16(uint8_t* p, i32x4 v) { *reinterpret_cast<i32x4*>(p) = v; }

// thread -> (row, unit) of a [B][units] grid
__device__ __forceinline__ bool span_unit(int B, int units, int* r, int* u) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  *r = (int)(t / units);
  *u = (int)(t - (long long)*r * units);
  return *r < B;
}

__global__ __launch_bounds__(256) void span_gather_kernel(const SpanRow* __restrict__ rows, int B, int step,
                                                           const uint8_t* __restrict__ frames, int row_bytes, int unit16,
                                                           uint8_t* __restrict__ dense, int32_t* __restrict__ step_ids,
                                                           const long long* __restrict__ map) {
  const int units = unit16 ? row_bytes >> 4 : row_bytes;
  int r, u;
  if (!span_unit(B, units, &r, &u)) return;
  const SpanRow row = rows[r];
  const bool runs = step < row.n_steps;
  if (u == 0) step_ids[r] = runs ? row.id : -1;
  if (!runs) return;
  const long long at = row.frame0 + step;   // (map: a compacted index, lyra_hip_encode_spans_dtx_dev)
  const uint8_t* src = frames + (size_t)(map ? map[at] : at) * row_bytes;
  uint8_t* dst = dense + (size_t)r * row_bytes;
  if (unit16) st16(dst + u * 16, ld16(src + u * 16));
  else dst[u] = src[u];
}

__global__ __launch_bounds__(256) void span_scatter_kernel(const SpanRow* __restrict__ rows, int B, int step,
                                                            const uint8_t* __restrict__ dense, int row_bytes, int unit16,
                                                            uint8_t* __restrict__ frames,
                                                            const long long* __restrict__ map) {
  const int units = unit16 ? row_bytes >> 4 : row_bytes;
  int r, u;
  if (!span_unit(B, units, &r, &u)) return;
  const SpanRow row = rows[r];
  if (step >= row.n_steps || step < row.n_warm) return;   // ended, or still warming up: nothing is stored
  const uint8_t* src = dense + (size_t)r * row_bytes;
  const long long at = row.frame0 + step;
  uint8_t* dst = frames + (size_t)(map ? map[at] : at) * row_bytes;
  if (unit16) st16(dst + u * 16, ld16(src + u * 16));
  else dst[u] = src[u];
}

// One workgroup per row, walking the three regions of the side as reset_kernel does.  A lane that is about to replay the hops
// in front of its chunk starts from the reset state, except that its ring phase words are those the span's own stream will
// have at the lane's first hop (target's now + phase_add): both then write every hop to the same ring rows, and after the
// warm-up the lane's slots equal the sequential stream's byte for byte.  target < 0: the plain reset state (phase 0).
__global__ __launch_bounds__(256) void span_lane_init_kernel(const ResetP* __restrict__ Pp, const SpanRow* __restrict__ rows, int n,
                                                              int r0, StateMap sm) {
  const ResetP& P = *Pp;
  const int b = blockIdx.x;
  if (b >= n) return;
  const SpanRow row = rows[b];
#pragma unroll 1
  for (int r = r0; r < r0 + 3; ++r) {
    const int bytes = sm.bytes[r];
    uint8_t* base = sm.base[r] + (size_t)row.id * bytes;
    const bool ringed = r == st::R_E1 || r == st::R_E2 || r == st::R_D0 || r == st::R_D1;
    for (int o = threadIdx.x * 16; o < bytes; o += 256 * 16) {
      const int w = (reset_fill(P, r, o) & 255) * 0x01010101;
      i32x4 q = (i32x4){w, w, w, w};
      if (o == 0 && ringed && row.target >= 0) {
        const int ph = *reinterpret_cast<const int*>(sm.base[r] + (size_t)row.target * bytes + st::PHASE);
        q[0] = (int)((unsigned)(ph + row.phase_add) % (unsigned)st::PHASE_MOD);
      }
      st16(base + o, q);
    }
  }
}
static_assert(st::PHASE == 0 && st::HDR >= 16, "the phase word is word 0 of the first 16-byte step of a ringed region");

__global__ __launch_bounds__(256) void span_handover_kernel(const SpanRow* __restrict__ rows, int n, int r0, StateMap sm) {
  const int b = blockIdx.x;
  if (b >= n) return;
  const SpanRow row = rows[b];
  if (!row.handover || row.target < 0) return;   // (workgroup-uniform)
#pragma unroll 1
  for (int r = r0; r < r0 + 3; ++r) {
    const int bytes = sm.bytes[r];
    const uint8_t* src = sm.base[r] + (size_t)row.id * bytes;
    uint8_t* dst = sm.base[r] + (size_t)row.target * bytes;
    for (int o = threadIdx.x * 16; o < bytes; o += 256 * 16) st16(dst + o, ld16(src + o));
  }
}

// The resampler of a span call at 8 / 32 / 48 kHz (lyra_hip_encode_spans_ext_dev / lyra_hip_decode_spans_ext_dev): every frame
// of every span in ONE launch, in front of the steps (encode: external rate -> 16 kHz) or behind them (decode).  The FIR's
// whole state is its last 34 input samples and the decimation phase, and inside a span those samples lie in the input buffer
// right in front of the frame, so no frame waits for another.  One wavefront per frame, four frames of ONE span per workgroup
// (rows[] names the first workgroup of each span with frames: span_row_of_workgroup).  Frame 0 of a span takes its history from
// the span stream's slot -- never from the buffer, the rows in front may be another span's -- and alone writes the slot; later
// frames take the 34 samples in front of the frame (rs_span_pass, resample_pass.h: the FIR is resample_kernel's).
__global__ __launch_bounds__(256) void span_resample_kernel(ResampleP P, const SpanRsRow* __restrict__ rows, int n_rows,
                                                             uint8_t* __restrict__ state, const int16_t* __restrict__ in,
                                                             int n_in, int16_t* __restrict__ out, int n_out) {
  extern __shared__ __attribute__((aligned(16))) float rsb_all[];   // [4][RS_TAPS - 1 + n_in, padded to 4]
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const SpanRsRow row = rows[span_row_of_workgroup(rows, n_rows, &SpanRsRow::wg0, (int)blockIdx.x)];
  const long long f = ((long long)blockIdx.x - row.wg0) * 4 + w;   // frame of the span
  if (f >= row.n_frames) return;   // (wave-uniform)
  // rows of 160 / 320 / 640 / 960 samples in a 16-byte aligned buffer; n_in > RS_H: `last` lies inside the span's last frame
  const int16_t* src = in + (size_t)(row.frame0 + f) * n_in;
  rs_span_pass(&P, rsb_all + w * ((RS_H + n_in + 3) & ~3), lane, state + (size_t)row.id * st::RS_BYTES, f, row.n_frames, src,
               src - RS_H, in + (size_t)(row.frame0 + row.n_frames) * n_in - RS_H, n_in, out + (size_t)(row.frame0 + f) * n_out,
               n_out);
}

}  // namespace lyra
