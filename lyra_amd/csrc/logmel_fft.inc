// logmel_fft.inc -- text of logmel_body (misc_kernels.hip) and span_logmel_kernel (spans_dtx_kernels.hip): radix-4 passes 2..5, the two magnitude spectra, the mel weights into LDS.
// In scope: what logmel_window.inc left, dsm, wl.  Defines wl1.
  // four more radix-4 passes; pass s combines four L-point transforms (L = 4^s) into one 4L-point one:
  //   y_q = sum_r (-i)^(r q) W_4L^(r k) F_r[k].  The twiddles of pass s+1 (L2-resident table) are requested before
  // the butterflies of pass s, so their latency hides behind the LDS round trip and the barrier.
#pragma unroll
  for (int s = 1; s < 5; ++s) {
    const int L = 1 << (2 * s);
    const int k = tid & (L - 1), g = tid >> (2 * s);
    f64x2* p = z + g * 4 * L + k;
    double n1r = 1.0, n1i = 0.0, n2r = 1.0, n2i = 0.0, n3r = 1.0, n3i = 0.0;
    if (s < 4) {
      const int Ln = 4 * L, kn = tid & (Ln - 1);
      const int t1 = kn * (256 >> (2 * (s + 1)));     // W_4L^k = W_1024^(k * 1024 / 4L)
      n1r = P.tw4_re[t1]; n1i = P.tw4_im[t1]; n2r = P.tw4_re[2 * t1]; n2i = P.tw4_im[2 * t1];
      n3r = P.tw4_re[3 * t1]; n3i = P.tw4_im[3 * t1];
    }
    const f64x2 xa = p[0], x1 = p[L], x2 = p[2 * L], x3 = p[3 * L];
    const double br = __builtin_fma(x1.x, w1r, -(x1.y * w1i)), bi = __builtin_fma(x1.x, w1i, x1.y * w1r);
    const double cr = __builtin_fma(x2.x, w2r, -(x2.y * w2i)), ci = __builtin_fma(x2.x, w2i, x2.y * w2r);
    const double dr = __builtin_fma(x3.x, w3r, -(x3.y * w3i)), di = __builtin_fma(x3.x, w3i, x3.y * w3r);
    const double s0r = xa.x + cr, s0i = xa.y + ci, s1r = xa.x - cr, s1i = xa.y - ci;
    const double s2r = br + dr, s2i = bi + di, s3r = br - dr, s3i = bi - di;
    p[0] = (f64x2){s0r + s2r, s0i + s2i};
    p[L] = (f64x2){s1r + s3i, s1i - s3r};         // (a - c) - i (b - d)
    p[2 * L] = (f64x2){s0r - s2r, s0i - s2i};
    p[3 * L] = (f64x2){s1r - s3i, s1i + s3r};     // (a - c) + i (b - d)
    w1r = n1r; w1i = n1i; w2r = n2r; w2i = n2i; w3r = n3r; w3i = n3i;
    __syncthreads();
  }
  LYRA_TSTAMP(112);
  // Z = FFT(a + i b):  A[k] = (Z[k] + conj(Z[N-k])) / 2,  B[k] = (Z[k] - conj(Z[N-k])) / (2 i).  In place: the item
  // for bin k <= 512 reads Z[k] and Z[N - k] and writes index k only; index k < 512 is read by no other item and
  // indices > 512 are never written, so no staging buffer (and no barrier before the writes) is needed.
  for (int k = tid; k <= 512; k += 256) {
    const int nk = (1024 - k) & 1023;
    const f64x2 zz = z[k], yy = z[nk];
    const double Ar = 0.5 * (zz.x + yy.x), Ai = 0.5 * (zz.y - yy.y);
    const double Br = 0.5 * (zz.y + yy.y), Bi = 0.5 * (yy.x - zz.x);
    z[k] = (f64x2){__builtin_sqrt(Ar * Ar + Ai * Ai), __builtin_sqrt(Br * Br + Bi * Bi)};
  }
  __syncthreads();
  LYRA_TSTAMP(113);
  // the mel weights go to the now dead upper half of the buffer: the band loops below would otherwise wait for one L2
  // round trip per bin
  wl[tid] = wsel0;
  wl[tid + 256] = wsel1;
  if (tid == 0) wl[512] = wsel2;
  double* wl1 = kRates ? dsm + 2048 : wl;   // frame 1's weights
  if constexpr (kRates) {
    wl1[tid] = vsel0;
    wl1[tid + 256] = vsel1;
    if (tid == 0) wl1[512] = vsel2;
  }
  __syncthreads();
