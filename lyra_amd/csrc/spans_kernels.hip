// spans_kernels.hip -- lyra_hip_encode_spans_dev / lyra_hip_decode_spans_dev (api.hip, spans_api.inc; plan: spans_plan.h): the
// row movement of a step and the hand-over of a time-parallel transcode.  The stage kernels and the quantizer read and write
// dense [B][.] rows; the caller's buffers are frame-major.  Per step one gather in front of the stages and, on steps that
// produce, one scatter behind them; all step-dependent decisions are taken here from the rows' plan and the step number, so the
// host enqueues the whole call from one upload.  Pure data movement: 16-byte units for PCM rows (640 bytes), bytes for packet
// rows (8 / 15 / 23 bytes, unaligned by nature); consecutive lanes move consecutive units of a row, rows are contiguous in
// the dense buffer.  Every access is guarded by the row count of the step and the row's own step range.
#include "kernels.h"

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
                                                           uint8_t* __restrict__ dense, int32_t* __restrict__ step_ids) {
  const int units = unit16 ? row_bytes >> 4 : row_bytes;
  int r, u;
  if (!span_unit(B, units, &r, &u)) return;
  const SpanRow row = rows[r];
  const bool runs = step < row.n_steps;
  if (u == 0) step_ids[r] = runs ? row.id : -1;
  if (!runs) return;
  const uint8_t* src = frames + (size_t)(row.frame0 + step) * row_bytes;
  uint8_t* dst = dense + (size_t)r * row_bytes;
  if (unit16) st16(dst + u * 16, ld16(src + u * 16));
  else dst[u] = src[u];
}

__global__ __launch_bounds__(256) void span_scatter_kernel(const SpanRow* __restrict__ rows, int B, int step,
                                                            const uint8_t* __restrict__ dense, int row_bytes, int unit16,
                                                            uint8_t* __restrict__ frames) {
  const int units = unit16 ? row_bytes >> 4 : row_bytes;
  int r, u;
  if (!span_unit(B, units, &r, &u)) return;
  const SpanRow row = rows[r];
  if (step >= row.n_steps || step < row.n_warm) return;   // ended, or still warming up: nothing is stored
  const uint8_t* src = dense + (size_t)r * row_bytes;
  uint8_t* dst = frames + (size_t)(row.frame0 + step) * row_bytes;
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

}  // namespace lyra
