// resample_slot.inc -- the write-back of one stream's resampler slot behind resample_fir.inc, textually shared by
// resample_kernel and resample_rates_kernel (misc_kernels.hip).  Expects in scope: rsb, n_in, in_pos, hist, slot, lane, H.
  // (same wavefront wrote and read this row: no barrier needed before the history leaves it)
  if (lane < H) hist[lane] = rsb[n_in + lane];
  // only the decimation phase is ever used: kept modulo 6 = lcm of the possible `down` factors (1, 2, 3), so the
  // counter never wraps out of phase however long the stream runs (the oracle keeps an unbounded counter)
  if (lane == 0) *reinterpret_cast<int*>(slot + st::RS_IN_POS) = (in_pos + n_in) % 6;
