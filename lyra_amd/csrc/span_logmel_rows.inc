// span_logmel_rows.inc -- text of span_logmel_kernel (spans_dtx_kernels.hip) and span_logmel_rates_kernel (spans_rates_kernels.hip):
// the workgroup's row, its pair of frames and their neighbours, then span_logmel.inc.
// In scope: rows / n_rows (SpanDtxRow), state, pcm, mel, and mel_of_row(i): the MelP of row i.
  int lo = 0, hi = n_rows - 1;   // the last row whose first workgroup is not behind this one
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rows[mid].wg0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const SpanDtxRow row = rows[lo];
  const long long f0 = ((long long)blockIdx.x - row.wg0) * 2;
  if (f0 >= row.n_frames) return;   // (workgroup-uniform, before any barrier)
  const MelP* Pp = mel_of_row(lo);
  const bool two = f0 + 1 < row.n_frames, first = f0 == 0;
  int16_t* slot_prev = reinterpret_cast<int16_t*>(state + (size_t)row.id * st::NOISE_BYTES + st::N_PREV);
  const int16_t* cur0 = pcm + (size_t)(row.frame0 + f0) * 320;
  const int16_t* cur1 = two ? cur0 + 320 : cur0;
  const int16_t* prev0 = first ? slot_prev : cur0 - 320;
  const int16_t* prev1 = two ? cur0 : prev0;
  const int16_t* last = pcm + (size_t)(row.frame0 + row.n_frames - 1) * 320;
  float* out = mel + (size_t)(row.region + f0) * SPAN_MEL_ROW;
#include "span_logmel.inc"
