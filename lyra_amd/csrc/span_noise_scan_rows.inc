// span_noise_scan_rows.inc -- text of span_noise_scan_kernel (spans_dtx_kernels.hip) and span_noise_scan_rates_kernel
// (spans_rates_kernels.hip): the wavefront's row and the hooks of a DTX scan, then span_noise_scan.inc.
// In scope: P (NoiseP), rows (SpanDtxRow; blockIdx.x < n_rows), state, mel, flag_out, v_noise, v_active, map, counts.
  const int lane = threadIdx.x;
  const SpanDtxRow row = rows[blockIdx.x];
  uint8_t* base = state + (size_t)row.id * st::NOISE_BYTES;
  const float* m = mel + (size_t)row.region * SPAN_MEL_ROW;
  const long long n = row.n_frames;
  struct Extra {};
  auto load_extra = [](long long, bool) { return Extra(); };
  auto on_entry = [](const float (&)[3], int) {};
  auto on_frame = [&](long long j, bool is_noise, long long active, const float (&)[3], Extra) {
    if (lane == 0) {
      const long long frame = row.frame0 + j;
      flag_out[frame] = is_noise ? v_noise : v_active;
      if (map && !is_noise) map[row.region + active] = frame;
    }
  };
  auto on_exit = [&](long long active) {
    if (lane == 0) counts[blockIdx.x] = (int32_t)active;
  };
#include "span_noise_scan.inc"
