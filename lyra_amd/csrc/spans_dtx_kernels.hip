// spans_dtx_kernels.hip -- lyra_hip_encode_spans_dtx_dev / lyra_hip_noise_spans_dev (api.hip, spans_api.inc): the NoiseEstimator
// of a DTX encoder over whole spans, in front of the chunked steps.  LyraEncoder::Encode (lyra_encoder.cc:113-156) hands the
// estimator the 16 kHz input audio and nothing else -- no encoder state, no features -- so the decisions of a whole recording
// can be computed before any encoder stage runs.  Two kernels:
//   span_logmel_kernel      the estimator's log-mel front end.  Its state is one hop of history (N_PREV), and inside a span that
//                           hop is the row in front of the frame: every frame of every span in ONE launch (the argument of
//                           span_resample_kernel).  The arithmetic is logmel_body's: both call the stages of logmel_stages.h.
//   span_noise_scan_kernel  the recurrence.  It is serial in time but small (160 bins, five floats per bin, two integers): one
//                           wavefront per span walks its frames with the state in registers.  Same float operations in the same
//                           order as noise_update_wave (misc_kernels.hip), restated here because the state lives elsewhere.
#include "kernels.h"
#include "logmel_stages.h"
#include "span_noise_scan.h"

namespace lyra {

// One workgroup per pair of consecutive frames (f0, f0 + 1) of ONE span (rows[] names the first workgroup of each span with
// frames; the lookup is on blockIdx alone); a span of an odd number of frames ends in a workgroup of one frame.
//   frame 0 of a span: previous hop from the span stream's N_PREV -- never from the buffer, the row in front may be another
//                      span's -- and the only workgroup that writes the slot: N_PREV = the span's last frame, what n_frames
//                      calls of logmel_kernel leave.  Read and write are one workgroup's, a barrier apart.
//   later frames:      previous hop = the row in front of the frame.
// Output per frame: the 160 log-mel bins and, beside them, Average() of the bins as noise_update_wave forms it (sequential
// float sum from 0.f, then / 160.f): it does not depend on the estimator's state, so it is taken off the serial scan.
__global__ __launch_bounds__(256) void span_logmel_kernel(const MelP* __restrict__ P1, const SpanDtxRow* __restrict__ rows,
                                                           int n_rows, uint8_t* __restrict__ state,
                                                           const int16_t* __restrict__ pcm, float* __restrict__ mel) {
  // one filterbank per call
  span_logmel_row(*P1, rows[span_row_of_workgroup(rows, n_rows, &SpanDtxRow::wg0, (int)blockIdx.x)], (int)blockIdx.x, state, pcm, mel);
}

// One wavefront per span, lane l owns bins l, l + 64, l + 128 (< 160) as in noise_update_wave.  The slot is read once, the frames
// are walked in order -- ComputeIsNoise, then DecayBounds or the update -- and the slot is written once.  Mel rows do not depend
// on the state: the rows of the next four frames are requested while the current four are worked on.  Average(smoothed) does
// depend on it and stays a sequential 160-term chain: the 160 values go through LDS and lane 0 sums them.
__global__ __launch_bounds__(64) void span_noise_scan_kernel(NoiseP P, const SpanDtxRow* __restrict__ rows, int n_rows,
                                                              uint8_t* __restrict__ state, const float* __restrict__ mel,
                                                              int32_t* __restrict__ flag_out, int v_noise, int v_active,
                                                              long long* __restrict__ map, int32_t* __restrict__ counts) {
  if ((int)blockIdx.x >= n_rows) return;
  span_dtx_scan(P, rows, state, mel, flag_out, v_noise, v_active, map, counts);
}

}  // namespace lyra
