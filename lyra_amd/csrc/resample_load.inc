// resample_load.inc -- the new samples of one stream's pass into its LDS row, textually shared by resample_kernel and
// resample_rates_kernel (misc_kernels.hip).  Expects in scope: rsb, src, n_in, vec, lane, H.
  if (vec) {
    for (int c = lane; c * 8 < n_in; c += 64) {
      const i32x4 raw = *reinterpret_cast<const i32x4*>(src + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) rsb[H + c * 8 + e] = (float)(int16_t)((raw[e >> 1] >> ((e & 1) * 16)) & 0xffff);
    }
  } else {
    for (int i = lane; i < n_in; i += 64) rsb[H + i] = (float)src[i];
  }
