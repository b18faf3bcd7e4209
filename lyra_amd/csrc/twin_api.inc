// twin_api.inc -- part of api.hip: the device half of BatchLyraDecoder (lyra_amd/host/lyra_batch_codec.cc), include/lyra_hip.h
// "Decoder twin".  LyraDecoder::DecodeSamplesInternal (lyra_decoder.cc:228-315) keeps, per stream, the conditioned hop of
// the generative model and of the comfort-noise generator and hands out slices of them; here those hops stay ON THE
// DEVICE in two [max_streams][320] arrays indexed by stream id, the host twin runs the per-stream state machine on
// integers and tells the device, round by round, which slices go where.  One request = any number of
//   lyra_hip_twin_decode / _conceal / _comfort_noise   (RunConditioning of the streams that start a hop)
//   lyra_hip_twin_assemble                              (RunModel slices + MaybeOverlapAndInsert)
//   lyra_hip_twin_noise                                 (noise_estimator_->ReceiveSamples on completed received hops)
// all enqueued on the decode-side stream without synchronising, then ONE lyra_hip_twin_fetch: optional resampling
// (BufferedResampler's Resample, buffered_resampler.cc:120-128), one D2H, one synchronise.  Host arguments are copied
// into a pinned arena at call time, so the caller's arrays may be reused as soon as a call returns.

namespace {

void twin_free(lyra_hip_ctx* c) {
  dfree(c->d_twin_gan, c->d_twin_cng, c->d_twin_noise, c->d_twin_out, c->d_twin_ext, c->d_twin_iota, c->d_twin_args);
  if (c->h_twin_args) (void)hipHostFree(c->h_twin_args);
  c->h_twin_args = nullptr;
  c->twin_out_cap = c->twin_ext_cap = c->twin_args_cap = c->twin_args_used = 0;
  c->twin_out_n = 0;
}

// MaybeOverlapAndInsert's cross-fade weight for fade_progress TWIN_FADE_LO + i (also lyra_hip_decode_lossy_dev's mix)
std::vector<float> fade_weights() {
  std::vector<float> w((size_t)TWIN_FADE_N);
  const int kFadeDurationSamples = 640;   // GetFadeDurationSamples (lyra_decoder.cc:53-62)
  for (int i = 0; i < TWIN_FADE_N; ++i) {
    const int fade_progress = TWIN_FADE_LO + i;
    // the expression of MaybeOverlapAndInsert (lyra_decoder.cc:364-365), evaluated as C++ evaluates it there
    const float overlap_weight = (1.f + std::cos(fade_progress * M_PI / kFadeDurationSamples)) / 2.f;
    w[(size_t)i] = overlap_weight;
  }
  return w;
}
// The table on the device: created at first use by whichever of its users (the twin's assemble, the lossy tick's mix,
// decode_samples' slices) comes first, freed by lyra_hip_destroy
int fade_ensure(lyra_hip_ctx* c) {
  if (c->d_fade) return 0;
  const std::vector<float> w = fade_weights();
  float* p = nullptr;
  HIPCHK(c, dalloc(&p, w.size()));
  const hipError_t e = hipMemcpy(p, w.data(), w.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(p);
    return fail(c, LYRA_HIP_EHIP, "upload of the fade weights failed: %s", hipGetErrorString(e));
  }
  c->d_fade = p;
  return 0;
}

int twin_ensure(lyra_hip_ctx* c) {
  int rc = fade_ensure(c);
  if (rc) return rc;
  if (c->d_twin_gan) return 0;
  const size_t n = (size_t)c->max_streams;
  HIPCHK(c, dalloc(&c->d_twin_gan, n * 320));
  HIPCHK(c, dalloc(&c->d_twin_cng, n * 320));
  HIPCHK(c, dalloc(&c->d_twin_noise, n * 320));
  HIPCHK(c, dalloc(&c->d_twin_iota, n));
  c->twin_args_cap = 2 * (n * 1024 + 65536);   // two halves: one per request in flight (lyra_hip_twin_fetch_begin)
  HIPCHK(c, dalloc(&c->d_twin_args, c->twin_args_cap));
  HIPCHK(c, hipHostMalloc((void**)&c->h_twin_args, c->twin_args_cap, hipHostMallocDefault));
  std::vector<int32_t> iota(n);
  for (size_t i = 0; i < n; ++i) iota[i] = (int32_t)i;
  HIPCHK(c, hipMemcpy(c->d_twin_iota, iota.data(), n * 4, hipMemcpyHostToDevice));
  return 0;
}

// host argument -> pinned arena -> device arena (same offset), asynchronous on the decode-side stream
int twin_stage(lyra_hip_ctx* c, const void* src, size_t bytes, void** d_out) {
  const size_t need = (bytes + 255) & ~(size_t)255;
  // With pipelined requests (lyra_hip_twin_fetch_begin / _end) the previous request's arguments may not have been uploaded
  // yet when this one is staged: requests alternate between the two halves of the arena, and a request may only start
  // while at most one other is still in flight -- the half's previous user has ended by then.
  const size_t half = c->twin_args_cap / 2, base = (size_t)(c->pl_begun[PL_TWIN_FETCH] & 1) * half;
  if (c->twin_args_used == 0 && pl_in_flight(c, PL_TWIN_FETCH) >= PL_DEPTH)
    return fail(c, LYRA_HIP_EINVAL, "twin: two requests are already in flight (lyra_hip_twin_fetch_end)");
  if (c->twin_args_used + need > half) {   // half full: everything staged so far has to be consumed first
    HIPCHK(c, hipStreamSynchronize(c->sd[0]));
    c->twin_args_used = 0;
    if (need > half) return fail(c, LYRA_HIP_EINVAL, "twin: argument of %zu bytes exceeds the staging arena", bytes);
  }
  const size_t off = base + c->twin_args_used;
  std::memcpy(c->h_twin_args + off, src, bytes);
  HIPCHK(c, hipMemcpyAsync(c->d_twin_args + off, c->h_twin_args + off, bytes, hipMemcpyHostToDevice, c->sd[0]));
  c->twin_args_used += need;
  *d_out = c->d_twin_args + off;
  return 0;
}

int twin_begin(lyra_hip_ctx* c, const int32_t* ids, int B, int32_t** d_ids) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if ((rc = check_ids_host(c, ids, B))) return rc;
  if ((rc = ensure_scratch(c, B))) return rc;
  if ((rc = twin_ensure(c))) return rc;
  if ((rc = dec_side_begin(c, 0))) return rc;   // include/lyra_hip.h "Streams" (1)
  return twin_stage(c, ids, (size_t)B * 4, (void**)d_ids);
}

// A twin call is a decode-side call on sd[0] like any other: it ends with the decode-side "done" record, so that a later
// split decode_dev (LYRA_HIP_SUBBATCHES > 1, chunks on sd[1..]) and the encode side's two-buffer rule are ordered after
// its state writes.
int twin_done(lyra_hip_ctx* c) {
  int rc = dec_side_done(c, 0, 1);
  if (!rc) c->n_dec_calls++;
  return rc;
}

int twin_scatter(lyra_hip_ctx* c, const int32_t* d_ids, int B, int16_t* dst) {
  hipLaunchKernelGGL(twin_scatter_kernel, dim3(B), dim3(128), 0, c->sd[0], (const int16_t*)c->d_pcm_out, d_ids, B, dst);
  HIPCHK(c, hipGetLastError());
  return twin_done(c);
}

}  // namespace

extern "C" {

int lyra_hip_twin_decode(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets, int num_bits) {
  if (!c || !packets) return c ? fail(c, LYRA_HIP_EINVAL, "null pointer") : LYRA_HIP_EINVAL;
  int rc = check_bits(c, num_bits);
  if (rc) return rc;
  DEVSCOPE(c);
  int32_t* d_ids;
  uint8_t* d_pk;
  if ((rc = twin_begin(c, ids, B, &d_ids))) return rc;
  if ((rc = twin_stage(c, packets, (size_t)B * (size_t)((num_bits + 7) / 8), (void**)&d_pk))) return rc;
  // SetEncodedPacket's DecodeToLossyFeatures + AddFeatures, then RunConditioning (lyra_decoder.cc:198-206, :317-326)
  if ((rc = launch_generate(c, 0, 0, d_ids, B, nullptr, c->d_pcm_out, d_pk, num_bits / 4))) return rc;
  return twin_scatter(c, d_ids, B, c->d_twin_gan);
}

int lyra_hip_twin_conceal(lyra_hip_ctx* c, const int32_t* ids, int B) {
  if (!c) return LYRA_HIP_EINVAL;
  DEVSCOPE(c);
  int32_t* d_ids;
  int rc = twin_begin(c, ids, B, &d_ids);
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(c->d_lossy, 0, (size_t)B * 64 * 4, c->sd[0]));   // ZeroFeatureEstimator::Estimate
  if ((rc = launch_generate(c, 0, 0, d_ids, B, c->d_lossy, c->d_pcm_out))) return rc;
  return twin_scatter(c, d_ids, B, c->d_twin_gan);
}

int lyra_hip_twin_comfort_noise(lyra_hip_ctx* c, const int32_t* ids, int B) {
  if (!c) return LYRA_HIP_EINVAL;
  DEVSCOPE(c);
  int32_t* d_ids;
  int rc = twin_begin(c, ids, B, &d_ids);
  if (rc) return rc;
  // AddFeatures(noise_estimator_->noise_estimate()) + RunConditioning (lyra_decoder.cc:328-340): the estimate is read in place
  if ((rc = launch_cng(c, c->sd[0], d_ids, B, nullptr, c->d_pcm_out))) return rc;
  return twin_scatter(c, d_ids, B, c->d_twin_cng);
}

int lyra_hip_twin_assemble(lyra_hip_ctx* c, const lyra_hip_twin_slice* slices, int B, int out_samples) {
  if (!c || !slices) return c ? fail(c, LYRA_HIP_EINVAL, "null pointer") : LYRA_HIP_EINVAL;
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (out_samples <= 0) return fail(c, LYRA_HIP_EINVAL, "twin_assemble: out_samples %d", out_samples);
  static_assert(sizeof(lyra_hip_twin_slice) == sizeof(TwinSlice), "slice layout");
  for (int i = 0; i < B; ++i) {
    const lyra_hip_twin_slice& s = slices[i];
    const int n = s.gen_n > s.cng_n ? s.gen_n : s.cng_n;
    if (s.id < 0 || s.id >= c->max_streams || s.gen_n < 0 || s.cng_n < 0 || (s.gen_n && s.cng_n && s.gen_n != s.cng_n) ||
        s.gan_off < 0 || s.gan_off + s.gen_n > 320 || s.cng_off < 0 || s.cng_off + s.cng_n > 320 || s.out_off < 0 ||
        s.out_off + n > out_samples || (s.fade_dir != 1 && s.fade_dir != -1) || s.noise_row >= c->max_streams ||
        s.fade < TWIN_FADE_LO + 320 || s.fade > TWIN_FADE_LO + TWIN_FADE_N - 1 - 320)
      return fail(c, LYRA_HIP_EINVAL, "twin_assemble: slice %d is inconsistent", i);
  }
  DEVSCOPE(c);
  if ((rc = twin_ensure(c))) return rc;
  if (c->twin_out_n == 0) {   // first slice set of a request: size the output rows
    const size_t need = (size_t)c->max_streams * (size_t)out_samples;
    if (need > c->twin_out_cap) {
      HIPCHK(c, hipStreamSynchronize(c->sd[0]));   // (a pipelined predecessor's rows live in the OTHER buffer, pipe_api.inc)
      if (c->d_twin_out) (void)hipFree(c->d_twin_out);
      c->d_twin_out = nullptr;
      c->twin_out_cap = 0;
      HIPCHK(c, dalloc(&c->d_twin_out, need));
      c->twin_out_cap = need;
    }
    c->twin_out_n = out_samples;
  } else if (c->twin_out_n != out_samples) {
    return fail(c, LYRA_HIP_EINVAL, "twin_assemble: out_samples changed inside a request (%d -> %d)", c->twin_out_n, out_samples);
  }
  TwinSlice* d_sl;
  if ((rc = twin_stage(c, slices, (size_t)B * sizeof(TwinSlice), (void**)&d_sl))) return rc;
  hipLaunchKernelGGL(twin_assemble_kernel, dim3(B), dim3(256), 0, c->sd[0], (const TwinSlice*)d_sl, B,
                     (const int16_t*)c->d_twin_gan, (const int16_t*)c->d_twin_cng, (const float*)c->d_fade,
                     c->d_twin_out, out_samples, c->d_twin_noise);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// `ids` in the order of the noise_row values 0 .. B-1 handed out by the preceding lyra_hip_twin_assemble
int lyra_hip_twin_noise(lyra_hip_ctx* c, const int32_t* ids, int B) {
  if (!c) return LYRA_HIP_EINVAL;
  DEVSCOPE(c);
  int32_t* d_ids;
  int rc = twin_begin(c, ids, B, &d_ids);
  if (rc) return rc;
  // lyra_hip_noise_receive_dev(DECODER) updates the same estimator slots on the noise stream: after everything enqueued there
  if ((rc = wait_noise_stream(c))) return rc;
  if ((rc = launch_noise(c, 1, c->sd[0], d_ids, B, c->d_twin_noise, c->d_flag_dec, nullptr))) return rc;
  return twin_done(c);
}

// Ends the request: rows 0 .. num_streams-1 of the assembled output, resampled to out_rate when it is not 16000
// (chunks of at most 960 internal samples -- the resampler is streaming, chunking is exact), to host memory.
int lyra_hip_twin_fetch(lyra_hip_ctx* c, int num_streams, int num_internal_samples, int out_rate, int16_t* out) {
  if (!c) return LYRA_HIP_EINVAL;
  int rc = check_batch(c, num_streams);
  if (rc) return rc;
  DEVSCOPE(c);
  const int n = num_internal_samples;
  // Every failing exit abandons the request: the staged arguments are consumed (synchronise) and the request state is reset,
  // so that the caller's next request starts clean whatever its out_samples is.
  auto abandon = [&](int code) {
    (void)hipStreamSynchronize(c->sd[0]);
    c->twin_args_used = 0;
    c->twin_out_n = 0;
    return code;
  };
  if (n < 0 || (n > 0 && (!out || c->twin_out_n != n))) {
    const int assembled = c->twin_out_n;
    return abandon(fail(c, LYRA_HIP_EINVAL, "twin_fetch: %d samples requested, %d assembled", n, assembled));
  }
  if (n > 0) {
    const int16_t* src = c->d_twin_out;
    size_t row = (size_t)n;
    if (out_rate != 16000) {
      ResampleP P;
      if (!resample_design(16000, out_rate, &P)) return abandon(fail(c, LYRA_HIP_EINVAL, "twin_fetch: unsupported rate %d", out_rate));
      if (n % P.down != 0)
        return abandon(fail(c, LYRA_HIP_EINVAL, "twin_fetch: %d internal samples are not a multiple of %d", n, P.down));
      const int n_ext = n * P.up / P.down;
      const size_t need = (size_t)c->max_streams * (size_t)n_ext;
      if (need > c->twin_ext_cap) {
        if (c->d_twin_ext) (void)hipFree(c->d_twin_ext);
        c->d_twin_ext = nullptr;
        c->twin_ext_cap = 0;
        HIPCHK(c, dalloc(&c->d_twin_ext, need));
        c->twin_ext_cap = need;
      }
      const int step = 960 / P.up;   // internal samples per chunk: at most 960 in and at most 960 out
      for (int s0 = 0; s0 < n; s0 += step) {
        const int n_in = n - s0 < step ? n - s0 : step;
        if ((rc = launch_resample(c, 1, c->d_twin_iota, num_streams, c->d_twin_out + s0, n_in, 16000, out_rate,
                                  c->d_twin_ext + (size_t)s0 * P.up / P.down, nullptr, n, n_ext)))
          return abandon(rc);
      }
      src = c->d_twin_ext;
      row = (size_t)n_ext;
    }
    HIPCHK(c, hipMemcpyAsync(out, src, (size_t)num_streams * row * 2, hipMemcpyDeviceToHost, c->sd[0]));
  }
  HIPCHK(c, hipStreamSynchronize(c->sd[0]));
  c->twin_args_used = 0;
  c->twin_out_n = 0;
  return 0;
}

}  // extern "C"
