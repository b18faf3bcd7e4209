// resample_fir.inc -- the polyphase FIR of one wavefront's pass, textually shared by resample_kernel, resample_rates_kernel
// (misc_kernels.hip: one stream's call) and span_resample_kernel (spans_kernels.hip: one frame of a span).  The stream-per-
// wavefront kernels follow it with resample_slot.inc, the write-back of the slot.  Expects in scope: P (ResampleP), rsb (the
// wavefront's LDS row [H history | n_in new samples]), n_in, n_out, in_pos, dst, lane.
  auto clip = [](float acc) { return (int16_t)(acc < -32768.f ? -32768.f : (acc > 32767.f ? 32767.f : acc)); };   // ClipToInt16 (dsp_utils.h:56-72)
  if (P.down == 1) {
    // interpolation: output k * up + ph is phase ph of the window at input k -- a lane takes input positions
    // k = lane, lane + 64, ...: one window of 35 samples in registers feeds all `up` phases, coefficients are scalars
    for (int k = lane; k < n_in; k += 64) {
      float win[st::RS_TAPS];
#pragma unroll
      for (int j = 0; j < st::RS_TAPS; ++j) win[j] = rsb[k + j];
#pragma unroll
      for (int ph = 0; ph < 3; ++ph) {
        if (ph < P.up) {
          float acc = 0.f;
#pragma unroll
          for (int j = 0; j < st::RS_TAPS; ++j) acc = acc + P.coef[ph][j] * win[j];
          dst[k * P.up + ph] = clip(acc);
        }
      }
    }
  } else {
    // decimation: the first input index (0-based in this call) that yields an output follows from the carried phase
    const int first = (P.down - in_pos % P.down) % P.down;
    for (int o = lane; o < n_out; o += 64) {
      const int k = first + o * P.down;
      float acc = 0.f;
#pragma unroll
      for (int j = 0; j < st::RS_TAPS; ++j) acc = acc + P.coef[0][j] * rsb[k + j];
      dst[o] = clip(acc);
    }
  }
