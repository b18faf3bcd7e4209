// logmel_band.inc -- text of logmel_body (misc_kernels.hip) and span_logmel_kernel (spans_dtx_kernels.hip): one (frame f, band) item -> lm.
// In scope: dsm, f, the band edges e0 / e1 / e2, the weights wt.
    const double* mag = dsm + f;          // |X_f[i]| = mag[2 * i]
    double acc = 0.0;
    double v = mag[2 * e0], wv = wt[e0];
    for (int i = e0; i < e2; ++i) {
      const double vn = mag[2 * i + 2], wn = wt[i + 1];
      const double w = v * wv;
      acc += i < e1 ? v - w : w;
      v = vn; wv = wn;
    }
    float x = (float)acc;
    x = x > 500.f ? x : 500.f;
    // log evaluated in double and rounded once: identical on host and device (oracle/lyra_oracle.c log_f)
    const float lm = (float)log((double)x) / 10.f;
