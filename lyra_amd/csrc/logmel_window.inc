// logmel_window.inc -- text of logmel_body (misc_kernels.hip) and span_logmel_kernel (spans_dtx_kernels.hip): the window of two frames and the first radix-4 pass.
// In scope: tid, P / PA / PB (MelP), kRates, two, prev0 / prev1 / cur0 / cur1 (int16 pointers), z (the FFT buffer).
  // window = [previous hop | this hop] x periodic Hann, zero-padded to 1024.  The first radix-4 pass of a decimation-in-
  // time transform combines x[n], x[n+256], x[n+512], x[n+768]: thread n reads its own three window samples of both
  // frames (x[n+768] = 0; x[n+512] = 0 for n >= 128) straight from memory, does that butterfly in registers and writes
  // the four results where the second pass expects them (4 * digit-reverse(n) + q) -- no staging pass, no scatter of
  // single samples.  The samples of this hop it holds are exactly the stream's next history: thread n >= 64 holds
  // sample n-64 of the hop, thread n < 128 sample n+192.
  const int n = tid;
  const bool has1 = n >= 64, has2 = n < 128;
  const int16_t a0 = prev0[n], a1 = prev1[n];
  const int16_t b0s = has1 ? cur0[n - 64] : prev0[n + 256], b1s = has1 ? cur1[n - 64] : prev1[n + 256];
  const int16_t c0s = has2 ? cur0[n + 192] : (int16_t)0, c1s = has2 ? cur1[n + 192] : (int16_t)0;
  const double h0 = P.hann[n], h1 = P.hann[n + 256], h2 = has2 ? P.hann[n + 512] : 0.0;
  // twiddles of the second pass (L = 4), requested before the first butterfly; mel weights and band edges for the epilogue
  double w1r, w1i, w2r, w2i, w3r, w3i;
  {
    const int t1 = (tid & 3) * 64;
    w1r = P.tw4_re[t1]; w1i = P.tw4_im[t1]; w2r = P.tw4_re[2 * t1]; w2i = P.tw4_im[2 * t1];
    w3r = P.tw4_re[3 * t1]; w3i = P.tw4_im[3 * t1];
  }
  const double wsel0 = PA.w[tid], wsel1 = PA.w[tid + 256], wsel2 = tid == 0 ? PA.w[512] : 0.0;
  double vsel0 = 0.0, vsel1 = 0.0, vsel2 = 0.0;
  if constexpr (kRates) { vsel0 = PB.w[tid]; vsel1 = PB.w[tid + 256]; vsel2 = tid == 0 ? PB.w[512] : 0.0; }
  // band sums: 320 (frame, band) items on 256 threads -- thread t < 160 takes (frame 0, band t), thread t >= 160 takes
  // (frame 1, band t - 96) i.e. the 96 widest bands, and threads t < 64 then also take (frame 1, band t), the narrow ones:
  // the longest chain is ONE wide band (<= 18 bins)
  const int my_band = tid < 160 ? tid : tid - 96;
  const int* bandp = (kRates && tid >= 160) ? PB.band : PA.band;
  const int be0 = bandp[my_band], be1 = bandp[my_band + 1], be2 = bandp[my_band + 2];
  int ce0 = be0, ce1 = be1, ce2 = be2;   // edges of the second item (frame 1, band tid) of threads < 64
  if constexpr (kRates) { if (tid < 64) { ce0 = PB.band[tid]; ce1 = PB.band[tid + 1]; ce2 = PB.band[tid + 2]; } }
  {
    const double ar = (double)a0 * h0, ai = two ? (double)a1 * h0 : 0.0;
    const double br = (double)b0s * h1, bi = two ? (double)b1s * h1 : 0.0;
    const double cr = (double)c0s * h2, ci = two ? (double)c1s * h2 : 0.0;
    const double s0r = ar + cr, s0i = ai + ci, s1r = ar - cr, s1i = ai - ci;   // d = 0: b + d = b - d = b
    unsigned r = __brev((unsigned)n) >> 24;                                     // reverse the four base-4 digits of n
    r = ((r & 0xAAu) >> 1) | ((r & 0x55u) << 1);
    f64x2* o = z + 4 * r;
    o[0] = (f64x2){s0r + br, s0i + bi};
    o[1] = (f64x2){s1r + bi, s1i - br};     // (a - c) - i b
    o[2] = (f64x2){s0r - br, s0i - bi};
    o[3] = (f64x2){s1r - bi, s1i + br};     // (a - c) + i b
  }
