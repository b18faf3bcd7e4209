// lossy_mix.inc -- text of lossy_mix_kernel (lossy_kernels.hip) and span_cng_kernel (spans_lossy_kernels.hip): one sample of the
// cross-fade of MaybeOverlapAndInsert (lyra_decoder.cc:342-373) where both hops run.
// In scope: fade_w (the host-built table), fade / dir (where the fade starts, its direction), i (the sample), g / c (the
// generative and the comfort-noise hop, int16), v (int16 result).
      const float w = fade_w[fade + i * dir - TWIN_FADE_LO];
      const float x = (float)g[i] * w;
      const float y = (float)c[i] * (1.f - w);
      v = (int16_t)(int)(x + y);
