// spans_mixed_kernels.hip -- lyra_hip_encode_spans_mixed_dev / lyra_hip_decode_spans_lossy_mixed_dev (api.hip,
// spans_mixed_api.inc): the row movement of a step whose rows each have a bitrate of their own.  The same two places in a step
// as spans_kernels.hip's gather and scatter, the same plan rows and the same guards -- the row count of the step, the row's own
// step range -- plus one int32 per dense row beside step_ids: the row's bit count (encode) or packet size (decode), which the
// mixed quantizer kernels read per row.  Packet rows are MAX_PACKET_BYTES apart in the caller's buffer and in the dense one, and
// only a row's own first bytes move: byte lanes, consecutive lanes consecutive bytes of a row (8 / 15 / 23 bytes, unaligned by
// nature).  PCM rows move in 16-byte units.  Pure data movement.
#include "kernels.h"
#include "lossy_plan.h"

namespace lyra {

namespace {
__device__ __forceinline__ i32x4 ld16(const uint8_t* p) { return *reinterpret_cast<const i32x4*>(p); }
__device__ __forceinline__ void st16(uint8_t* p, i32x4 v) { *reinterpret_cast<i32x4*>(p) = v; }

// thread -> (row, unit) of a [B][units] grid
__device__ __forceinline__ bool span_unit(int B, int units, int* r, int* u) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  *r = (int)(t / units);
  *u = (int)(t - (long long)*r * units);
  return *r < B;
}
}  // namespace

// frame_bits != nullptr (encode): frames = PCM [frames][640], moved in 40 units of 16 bytes; step_size[r] = frame_bits[frame].
//   A row that has ended carries 4, a valid count: rvq_encode_mixed_kernel judges the count of every row < B, masked or not.
// else (decode): frames = packets [frames][MAX_PACKET_BYTES]; step_size[r] = tick_bytes[compacted index], and that many bytes
//   of the row move.  A row that has ended carries 0: no stages.
__global__ __launch_bounds__(256) void span_gather_mixed_kernel(const SpanRow* __restrict__ rows, int B, int step,
                                                                 const uint8_t* __restrict__ frames,
                                                                 const int32_t* __restrict__ frame_bits,
                                                                 const uint8_t* __restrict__ tick_bytes,
                                                                 uint8_t* __restrict__ dense, int32_t* __restrict__ step_ids,
                                                                 int32_t* __restrict__ step_size,
                                                                 const long long* __restrict__ map) {
  const bool enc = frame_bits != nullptr;
  const int units = enc ? 40 : MAX_PACKET_BYTES;
  int r, u;
  if (!span_unit(B, units, &r, &u)) return;
  const SpanRow row = rows[r];
  const bool runs = step < row.n_steps;
  if (!runs) {
    if (u == 0) {
      step_ids[r] = -1;
      step_size[r] = enc ? 4 : 0;
    }
    return;
  }
  const long long at = row.frame0 + step;   // (map: a compacted index)
  const size_t frame = (size_t)(map ? map[at] : at);
  if (enc) {
    if (u == 0) {
      step_ids[r] = row.id;
      step_size[r] = frame_bits[frame];
    }
    st16(dense + (size_t)r * 640 + u * 16, ld16(frames + frame * 640 + u * 16));
  } else {
    const int size = min((int)tick_bytes[at], MAX_PACKET_BYTES);
    if (u == 0) {
      step_ids[r] = row.id;
      step_size[r] = size;
    }
    if (u < size) dense[(size_t)r * MAX_PACKET_BYTES + u] = frames[frame * MAX_PACKET_BYTES + u];
  }
}

// dense packets [B][MAX_PACKET_BYTES] of the rows past their warm-up -> the first (step_bits[r] + 7) / 8 bytes of the frame's
// row, and that size to packet_bytes[frame].  The bytes behind them are never written.
__global__ __launch_bounds__(256) void span_scatter_mixed_kernel(const SpanRow* __restrict__ rows, int B, int step,
                                                                  const uint8_t* __restrict__ dense,
                                                                  const int32_t* __restrict__ step_bits,
                                                                  uint8_t* __restrict__ frames,
                                                                  int32_t* __restrict__ packet_bytes,
                                                                  const long long* __restrict__ map) {
  int r, u;
  if (!span_unit(B, MAX_PACKET_BYTES, &r, &u)) return;
  const SpanRow row = rows[r];
  if (step >= row.n_steps || step < row.n_warm) return;   // ended, or still warming up: nothing is stored
  const int size = min(max((step_bits[r] + 7) >> 3, 0), MAX_PACKET_BYTES);
  const long long at = row.frame0 + step;
  const size_t frame = (size_t)(map ? map[at] : at);
  if (u == 0) packet_bytes[frame] = size;
  if (u < size) frames[frame * MAX_PACKET_BYTES + u] = dense[(size_t)r * MAX_PACKET_BYTES + u];
}

}  // namespace lyra
