// spans_lossy_kernels.hip -- lyra_hip_decode_spans_lossy_dev (api.hip, spans_lossy_api.inc; plan: spans_lossy_plan.h): the legs of
// LyraDecoder's packet-loss path over whole spans, behind the chunked decoder steps.  The plan has fixed on the host what every
// tick does; what is left for the device, in stream order:
//   span_lossy_feat_kernel    a step's concealed rows get ZeroFeatureEstimator's 64 x 0.0f in place of the RVQ decode;
//   span_logmel_map_kernel    the estimator's log-mel of every RECEIVED frame in one launch: span_logmel_kernel with the previous
//                             hop taken from the previous received frame of the span (both call span_logmel, logmel_stages.h);
//   span_lossy_scan_kernel    the recurrence over the received list, one wavefront per span (span_noise_scan, span_noise_scan.h,
//                             as span_noise_scan_kernel, with hooks of its own); it also writes the estimate to a snapshot row after the
//                             frames the plan marks, and is_noise of the received frames;
//   span_cng_kernel           comfort noise + mix of every run_cng tick.  The phases are counter-based, so every frame's inverse
//                             STFT is independent; only the overlap-add is ordered, and a hop overlaps the three frames in front
//                             of it: workgroup k synthesises frames k - 3 .. k (cng_frame, cng_frame.h, as cng_kernel) and
//                             adds them oldest first, exactly the additions the sequential accumulator has seen.  No scratch.
//                             A second launch, one workgroup per span, leaves the accumulator and the hop counter;
//   span_lossy_finish_kernel  is_comfort_noise, is_noise of the frames without a packet, the final control word.
#include "kernels.h"
#include "lossy_plan.h"
#include "cng_frame.h"
#include "logmel_stages.h"
#include "span_noise_scan.h"

namespace lyra {

// io[r]: a stream id in, that stream's control word out (one thread per span; the one thing the host waits for)
__global__ __launch_bounds__(256) void span_lossy_ctl_read_kernel(int32_t* __restrict__ io, int n, int max_streams,
                                                                   const uint8_t* __restrict__ cng_state) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int id = io[r];
  if (id < 0 || id >= max_streams) return;
  io[r] = (int32_t)*reinterpret_cast<const uint32_t*>(cng_state + (size_t)id * st::CNG_BYTES + LOSSY_CTL);
}

// rows of step `step` whose tick conceals: feats[r][0..63] = 0.0f (lossy_plan_tile.inc does the same per tick).
// gen_received[c]: entry c of the compacted run_gen list came with a packet.
__global__ __launch_bounds__(256) void span_lossy_feat_kernel(const SpanRow* __restrict__ rows, int B, int step,
                                                               const uint8_t* __restrict__ gen_received,
                                                               float* __restrict__ feats) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int r = (int)(t >> 6), d = (int)(t & 63);
  if (r >= B) return;
  const SpanRow row = rows[r];
  if (step >= row.n_steps) return;
  if (!gen_received[row.frame0 + step]) feats[(size_t)r * 64 + d] = 0.f;
}

// One workgroup per pair of consecutive RECEIVED frames (j0, j0 + 1) of one span.
//   received frame 0: previous hop from the span stream's N_PREV; the only workgroup that writes the slot: N_PREV = the span's
//                     last received frame.  Read and write are one workgroup's, a barrier apart.
//   later ones:       previous hop = the received frame in front, wherever it lies in the buffer.
// pcm holds the GENERATIVE hops of the received frames (the mix runs behind this pass).  Output as span_logmel_kernel's.
__global__ __launch_bounds__(256) void span_logmel_map_kernel(const MelP* __restrict__ Pp, const SpanLossyRow* __restrict__ rows,
                                                               int n_rows, uint8_t* __restrict__ state,
                                                               const SpanLossyRx* __restrict__ rx,
                                                               const int16_t* __restrict__ pcm, float* __restrict__ mel) {
  const SpanLossyRow row = rows[span_row_of_workgroup(rows, n_rows, &SpanLossyRow::rx_wg0, (int)blockIdx.x)];
  const int j0 = ((int)blockIdx.x - row.rx_wg0) * 2;
  if (j0 >= row.n_rx) return;   // (workgroup-uniform, before any barrier)
  const bool two = j0 + 1 < row.n_rx, first = j0 == 0;
  const SpanLossyRx* list = rx + row.rx0;
  int16_t* slot_prev = reinterpret_cast<int16_t*>(state + (size_t)row.id * st::NOISE_BYTES + st::N_PREV);
  const int16_t* cur0 = pcm + (size_t)list[j0].frame * 320;
  const int16_t* cur1 = two ? pcm + (size_t)list[j0 + 1].frame * 320 : cur0;
  const int16_t* prev0 = first ? slot_prev : pcm + (size_t)list[j0 - 1].frame * 320;
  const int16_t* prev1 = two ? cur0 : prev0;
  const int16_t* last = pcm + (size_t)list[row.n_rx - 1].frame * 320;
  span_logmel(*Pp, two, first, cur0, cur1, prev0, prev1, slot_prev, last, mel + (size_t)(row.rx0 + j0) * SPAN_MEL_ROW);
}

// One wavefront per span over its received list.  snaps[row][160]: the estimate (N_EST) after the entries whose snap names a
// row, and on entry where the span's snap_v0 does; entry_noise[span row]: is_noise() on entry (span_lossy_finish_kernel hands
// it to the frames in front of the first packet).  is_noise may be null.
__global__ __launch_bounds__(64) void span_lossy_scan_kernel(NoiseP P, const SpanLossyRow* __restrict__ rows, int n_rows,
                                                              uint8_t* __restrict__ state, const float* __restrict__ mel,
                                                              const SpanLossyRx* __restrict__ rx, int32_t* __restrict__ is_noise_out,
                                                              float* __restrict__ snaps, int32_t* __restrict__ entry_noise) {
  if ((int)blockIdx.x >= n_rows) return;
  const SpanLossyRow row = rows[blockIdx.x];
  struct Hooks {
    struct Extra { long long frame; int snap; };
    int lane;
    const SpanLossyRx* list;
    int snap_v0;
    int32_t* is_noise_out;
    float* snaps;
    int32_t* entry_noise;
    __device__ __forceinline__ Extra load_extra(long long j, bool in) const { return in ? Extra{list[j].frame, list[j].snap} : Extra{0, -1}; }
    __device__ __forceinline__ void snapshot(int at, const float (&est)[3]) const {
      if (at < 0) return;   // (wave-uniform)
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (lane + 64 * i < 160) snaps[(size_t)at * 160 + lane + 64 * i] = est[i];
    }
    __device__ __forceinline__ void on_entry(const float (&est)[3], int last_is_noise) const {
      snapshot(snap_v0, est);
      if (lane == 0) *entry_noise = last_is_noise;
    }
    __device__ __forceinline__ void on_frame(long long, bool is_noise, long long, const float (&est)[3], Extra x) const {
      if (lane == 0 && is_noise_out) is_noise_out[x.frame] = is_noise ? 1 : 0;
      snapshot(x.snap, est);
    }
    __device__ __forceinline__ void on_exit(long long) const {}
  } hooks{(int)threadIdx.x, rx + row.rx0, row.snap_v0, is_noise_out, snaps, entry_noise + blockIdx.x};
  span_noise_scan(P, hooks.lane, state + (size_t)row.id * st::NOISE_BYTES, mel + (size_t)row.rx0 * SPAN_MEL_ROW, row.n_rx, hooks);
}

// Comfort noise and mix.  final == 0: grid = the run_cng ticks of all rows; workgroup k of a span produces tick k: its hop is
// accumulator positions 320 k .. 320 k + 319 of the span's time line, each the sum, oldest first, of what the sequential
// accumulator held there -- the slot's C_OLA on entry while that still reaches (position < 1024), else the 0.0 that the shift
// brought in (so that -0.0 cannot survive) -- and of frames k - 3 .. k.  Frame j has hop counter C_HOP + j and reads the
// estimate snapshot of its tick.  The clipped hop is the tick's output or is cross-faded with the generative hop already in
// pcm16[frame] (lossy_fade_sample, as lossy_mix_kernel), in place.  Nothing of the slot is written.
// final != 0: grid = rows; the workgroup of a span with n_cng > 0 forms positions 320 n_cng .. + 1023 the same way -- what the
// sequential accumulator holds after the span -- and writes C_OLA and C_HOP + n_cng.
__global__ __launch_bounds__(256) void span_cng_kernel(const MelP* __restrict__ Pp, unsigned long long seed,
                                                        const SpanLossyRow* __restrict__ rows, int n_rows, int final,
                                                        uint8_t* __restrict__ state, const SpanLossyCng* __restrict__ ticks,
                                                        const float* __restrict__ snaps, const float* __restrict__ fade_w,
                                                        int16_t* __restrict__ pcm16) {
  const MelP& P = *Pp;
  extern __shared__ __attribute__((aligned(16))) double dsm[];
  double* re = dsm;
  double* im = dsm + 1024;
  double* mel = dsm + 2048;   // [160]
  __shared__ int16_t hop_out[320];
  const int tid = threadIdx.x;
  int rw, tk;
  if (final) {
    rw = blockIdx.x;
    if (rw >= n_rows) return;
    tk = rows[rw].n_cng;
    if (tk == 0) return;   // (workgroup-uniform, like every return here)
  } else {
    rw = span_row_of_workgroup(rows, n_rows, &SpanLossyRow::cng_wg0, (int)blockIdx.x);
    tk = (int)blockIdx.x - rows[rw].cng_wg0;
    if (tk >= rows[rw].n_cng) return;
  }
  const SpanLossyRow row = rows[rw];
  const SpanLossyCng* list = ticks + row.cng0;
  uint8_t* slot = state + (size_t)row.id * st::CNG_BYTES;
  const unsigned long long hop0 = *reinterpret_cast<const unsigned long long*>(slot + st::C_HOP);
  double* ola = reinterpret_cast<double*>(slot + st::C_OLA);
  // (the slot key is zero unless the stream was imported from another id or context: state_layout.h C_KEY)
  const unsigned long long sd = seed ^ (unsigned long long)(unsigned)row.id ^ *reinterpret_cast<const unsigned long long*>(slot + st::C_KEY);
  double acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long long p = 320ll * tk + tid + 256 * q;
    acc[q] = p < 1024 ? ola[p] : 0.0;
  }
  const int j_last = tk < row.n_cng ? tk : row.n_cng - 1;
#pragma unroll 1
  for (int j = tk > 3 ? tk - 3 : 0; j <= j_last; ++j) {
    const float* feat = snaps + (size_t)list[j].snap * 160;
    const unsigned long long hop = hop0 + (unsigned long long)j;
    cng_frame(P, tid, feat, sd, hop, re, im, mel);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int at = 320 * (tk - j) + tid + 256 * q;   // the accumulator position inside frame j
      if (at < 1024) acc[q] = acc[q] + cng_windowed(re, at);
    }
    __syncthreads();   // re[] is rebuilt by the next frame
  }
  if (final) {   // (every read of the old accumulator lies in front of the loop's barriers; n_cng >= 1)
#pragma unroll
    for (int q = 0; q < 4; ++q) ola[tid + 256 * q] = acc[q];
    if (tid == 0) *reinterpret_cast<unsigned long long*>(slot + st::C_HOP) = hop0 + (unsigned long long)row.n_cng;
    return;
  }
  const SpanLossyCng tick = list[tk];
  const int16_t* g = pcm16 + (size_t)tick.frame * 320;
  int16_t* o = pcm16 + (size_t)tick.frame * 320;
  const int16_t* c = hop_out;
  const bool gen = tick.info & LOSSY_GEN;
  const int fade = (tick.info >> 8) * 320, dir = (tick.info & LOSSY_TO_CNG) ? 1 : -1;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int i = tid + 256 * q;
    if (i >= 320) break;
    double y = acc[q];
    y = y < -32768.0 ? -32768.0 : (y > 32767.0 ? 32767.0 : y);   // ClipToInt16<double>
    hop_out[i] = (int16_t)y;   // (read back by this thread alone)
    o[i] = !gen ? c[i] : lossy_fade_sample(fade_w, fade, dir, i, g, c);
  }
}

// One thread per frame of every span (frames[info0 + f] belongs to frame frame0 + f of the row): is_comfort_noise; is_noise of a
// frame without a packet = that of the received frame `back` frames in front of it, which span_lossy_scan_kernel wrote and this
// kernel never writes, or with back == 0 the estimator's is_noise() on entry.  The thread of a span's first frame leaves the
// control word.  is_noise / is_cn may be null.
__global__ __launch_bounds__(256) void span_lossy_finish_kernel(const SpanLossyRow* __restrict__ rows, int n_rows, long long total,
                                                                 const SpanLossyFrame* __restrict__ frames,
                                                                 uint8_t* __restrict__ cng_state,
                                                                 const int32_t* __restrict__ entry_noise,
                                                                 int32_t* is_noise, int32_t* __restrict__ is_cn) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  int lo = 0, hi = n_rows - 1;   // the last row that starts at or in front of p
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[mid].info0 <= p) lo = mid; else hi = mid - 1;
  }
  const SpanLossyRow row = rows[lo];
  const long long f = p - row.info0;
  if (f >= row.n_frames) return;
  const long long frame = row.frame0 + f;
  const SpanLossyFrame x = frames[p];
  if (is_cn) is_cn[frame] = (x.info & LOSSY_CN) ? 1 : 0;
  if (is_noise && !(x.info & LOSSY_RX)) is_noise[frame] = x.back ? is_noise[frame - x.back] : entry_noise[lo];
  if (f == 0) *reinterpret_cast<uint32_t*>(cng_state + (size_t)row.id * st::CNG_BYTES + LOSSY_CTL) = row.ctl_out;
}

}  // namespace lyra
