// lossy_api.inc -- part of api.hip: lyra_hip_decode_lossy_dev, LyraDecoder::SetEncodedPacket (when a packet arrived) +
// DecodeSamples(one hop) for hop-synchronous receivers, with the reference's packet-loss concealment, comfort noise and
// cross-fades (lyra_decoder.cc:172-373) run on the device.  The per-stream control state (concealment / fade progress,
// fade direction) is one word in the stream's comfort-noise slot (lossy_plan.h).  One tick is
//   decode stream: rvq_decode of the packet rows -> lossy_plan_kernel (transition, id lists, zero features of the rows
//                  that conceal) -> the decoder chain on the generative list (TileCtx: id -1 writes no state, no output);
//   noise stream:  cng_kernel on the comfort-noise list (reads the estimate BEFORE this tick's update) -> lossy_mix_kernel
//                  -> the decoder-side NoiseEstimator on the received rows' generative hop -> the output resampler,
// the noise-stream half being ONE noise call as in noise_and_resample_deferred (lyra_hip_run_steps_dev's decoder legs).

namespace {

Bufs lossy_call_bufs(lyra_hip_ctx* c) {   // per frame of `lossy_cap`
  return {BUF(c->d_lossy_ids[0], 3),  BUF(c->d_lossy_info[0], 1), BUF(c->d_lossy_gan[0], 320), BUF(c->d_lossy_ids[1], 3),
          BUF(c->d_lossy_info[1], 1), BUF(c->d_lossy_gan[1], 320), BUF(c->d_lossy_cng, 320),   BUF(c->d_lossy_feat, 64)};
}
void lossy_free_call_bufs(lyra_hip_ctx* c) {
  free_bufs(lossy_call_bufs(c));
  c->lossy_cap = 0;
}
void lossy_free(lyra_hip_ctx* c) {
  lossy_free_call_bufs(c);
  dfree(c->d_lossy_err);
}

int lossy_ensure(lyra_hip_ctx* c, int B) {
  int rc = fade_ensure(c);
  if (rc) return rc;
  if ((rc = err_word_ensure(c, &c->d_lossy_err))) return rc;
  if (B <= c->lossy_cap) return 0;
  if ((rc = sync_all(c))) return rc;   // (the buffers of the calls in flight)
  lossy_free_call_bufs(c);
  if ((rc = alloc_bufs(c, lossy_call_bufs(c), (size_t)B))) return rc;
  c->lossy_cap = B;
  return 0;
}

// launch_noise (decoder side) on the noise stream for the rows of an id list (-1: skip): the estimator sees received hops only
// (lyra_decoder.cc:304-311)
int launch_noise_masked(lyra_hip_ctx* c, const int32_t* d_est_ids, int B, const int16_t* d_pcm, int32_t* d_is_noise) {
  { ProfScope ps(c, K_NOISE, c->sn);
    hipLaunchKernelGGL(logmel_masked_kernel, dim3(cdiv(B, 2)), dim3(256), logmel_lds_bytes(), c->sn, c->model.d_mel_rate[1],
                       d_pcm, d_est_ids, B, c->sm.base[st::R_NOISE_D], (int)st::NOISE_BYTES, (int)st::N_PREV, (float*)nullptr, 1,
                       noise_params(16000), d_is_noise, (int32_t*)nullptr); }
  HIPCHK(c, hipGetLastError());
  return 0;
}

// The end of a decode-side call whose second half runs on the noise stream (the lossy tick, decode_samples), after that
// half's noise_dev_done.  Strict call order (lyra_hip_set_serial): the decode-side call ends with its noise-stream half.
int serial_noise_half_done(lyra_hip_ctx* c) {
  if (!c->serial) return 0;
  HIPCHK(c, hipStreamWaitEvent(c->sd[0], c->ev_noise[(c->n_noise_calls - 1) & 1], 0));
  const int slot = (int)((c->n_dec_calls - 1) & 1);
  for (int j = 0; j < c->nsub; ++j) HIPCHK(c, hipEventRecord(c->ev_dec[slot][j], c->sd[0]));
  if (c->nsub == 1) c->noise_done_dec = c->n_noise_calls;
  return 0;
}

// One tick of B streams.  d_pkt_bytes / d_rx may be null (every packet whole / every row received).
int lossy_tick_launch(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_packets, const int32_t* d_pkt_bytes,
                      const uint8_t* d_rx, int num_bits, int ext, int16_t* d_pcm16, int16_t* d_pcm_ext, int32_t* d_is_noise,
                      int32_t* d_is_cn, int mixed, const int32_t* d_rates, const int32_t* d_offsets, long n_pcm) {
  DEVSCOPE(c);
  int rc = ensure_scratch(c, B);
  if (rc) return rc;
  if ((rc = lossy_ensure(c, B))) return rc;
  const int set = (int)(c->n_lossy_calls & 1);
  const size_t cap = (size_t)c->lossy_cap;
  int32_t* gen_ids = c->d_lossy_ids[set];
  int32_t* cng_ids = gen_ids + cap;
  int32_t* est_ids = gen_ids + 2 * cap;
  int32_t* info = c->d_lossy_info[set];
  int16_t* gan = c->d_lossy_gan[set];
  // ---- decode stream: one unsplit decode-side call (on split contexts it stands for every chunk, dec_side_done) ----
  if ((rc = dec_side_begin(c, 0, 1))) return rc;
  if (mixed == LOSSY_UNIFORM) {
    if ((rc = launch_rvq_decode(c, 0, B, nullptr, d_packets, num_bits / 4, c->d_lossy_feat))) return rc;
    hipLaunchKernelGGL(lossy_plan_kernel, dim3(cdiv(B, 256)), dim3(256), 0, c->sd[0], d_ids, B, d_pkt_bytes, (num_bits + 7) / 8,
                       d_rx, c->sm.base[st::R_CNG], gen_ids, cng_ids, est_ids, info, c->d_lossy_feat, c->d_lossy_err);
  } else {   // rows LYRA_HIP_MAX_PACKET_BYTES apart, each at the stage count of its size (mixed_api.inc)
    const int from_bits = mixed == LOSSY_MIXED_BITS ? 1 : 0;
    { ProfScope ps(c, K_RVQ_DEC, c->sd[0]);
      hipLaunchKernelGGL(rvq_decode_mixed_kernel, dim3(cdiv(B, 4)), dim3(256), 0, c->sd[0], c->model.cb, d_packets, d_pkt_bytes,
                         from_bits, B, c->d_lossy_feat); }
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(lossy_plan_mixed_kernel, dim3(cdiv(B, 256)), dim3(256), 0, c->sd[0], d_ids, B, d_pkt_bytes, from_bits,
                       d_rx, c->sm.base[st::R_CNG], gen_ids, cng_ids, est_ids, info, c->d_lossy_feat, c->d_lossy_err);
  }
  HIPCHK(c, hipGetLastError());
  if ((rc = launch_generate(c, 0, 0, gen_ids, B, c->d_lossy_feat, gan))) return rc;
  if ((rc = dec_side_done(c, 0, 1))) return rc;
  c->n_dec_calls++;
  // ---- noise stream: comfort noise, mix, estimator, resampler as ONE noise call --------------------------------------
  if ((rc = noise_dev_begin(c))) return rc;
  if ((rc = launch_cng(c, c->sn, cng_ids, B, nullptr, c->d_lossy_cng))) return rc;
  hipLaunchKernelGGL(lossy_mix_kernel, dim3(cdiv(B, 4)), dim3(256), 0, c->sn, d_ids, B, (const int32_t*)info,
                     (const int16_t*)gan, (const int16_t*)c->d_lossy_cng, (const float*)c->d_fade, d_pcm16,
                     (const uint8_t*)c->sm.base[st::R_NOISE_D], d_is_noise, d_is_cn);
  HIPCHK(c, hipGetLastError());
  // (bridge_api.inc: the hop and the mix's flags are complete here; the estimator behind reads `gan` only)
  if (c->lossy_mix_hook) HIPCHK(c, hipEventRecord(c->lossy_mix_hook, c->sn));
  if ((rc = launch_noise_masked(c, est_ids, B, gan, d_is_noise))) return rc;
  if (d_rates && n_pcm >= 0) {   // per-stream rates, packed rows (decode_streams_api.inc): d_pcm_ext holds n_pcm samples with
    // row b at d_offsets[b] (null: b * LYRA_HIP_MAX_EXT_HOP); a row that leaves the buffer writes nothing
    { ProfScope ps(c, K_RESAMPLE, c->sn);
      hipLaunchKernelGGL(resample_streams_out_kernel, dim3(cdiv(B, 4)), dim3(256), resample_rates_lds_bytes(), c->sn,
                         (const ResampleP*)c->d_rs_tab, d_rates, d_ids, B, c->sm.base[st::R_RS_D], (const int16_t*)d_pcm16, 320,
                         d_pcm_ext, d_offsets, (int)LYRA_HIP_MAX_EXT_HOP, n_pcm, c->d_rates_err); }
    HIPCHK(c, hipGetLastError());
    c->rs_sn_pending = true;
  } else if (d_rates) {   // per-stream rates (rates_api.inc): d_pcm_ext rows LYRA_HIP_MAX_EXT_HOP apart
    if ((rc = launch_resample_rates(c, 1, d_ids, d_rates, B, d_pcm16, 320, d_pcm_ext, LYRA_HIP_MAX_EXT_HOP, nullptr, c->sn)))
      return rc;
    c->rs_sn_pending = true;
  } else if (ext != 16000) {
    if ((rc = launch_resample(c, 1, d_ids, B, d_pcm16, 320, 16000, ext, d_pcm_ext, nullptr, 0, 0, c->sn))) return rc;
    c->rs_sn_pending = true;
  }
  if ((rc = noise_dev_done(c))) return rc;
  c->n_lossy_calls++;
  return serial_noise_half_done(c);
}

}  // namespace

extern "C" {

int lyra_hip_decode_lossy_dev(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_packets,
                              const int32_t* d_packet_bytes, int num_bits, int sample_rate_hz, int16_t* d_pcm16,
                              int16_t* d_pcm_ext, int32_t* d_is_noise, int32_t* d_is_comfort_noise) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if ((rc = check_bits(c, num_bits))) return rc;
  if ((rc = check_rate(c, sample_rate_hz))) return rc;
  if (!d_ids || !d_packets || !d_packet_bytes || !d_pcm16 || (sample_rate_hz != 16000 && !d_pcm_ext))
    return fail(c, LYRA_HIP_EINVAL, "decode_lossy: null pointer");
  return lossy_tick_launch(c, d_ids, B, d_packets, d_packet_bytes, nullptr, num_bits, sample_rate_hz, d_pcm16, d_pcm_ext,
                           d_is_noise, d_is_comfort_noise);
}

long lyra_hip_decode_lossy_errors(lyra_hip_ctx* c, int clear) {
  return read_error_counter(c, &lyra_hip_ctx::d_lossy_err, clear);
}

}  // extern "C"
