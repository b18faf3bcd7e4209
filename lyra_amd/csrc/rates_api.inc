// rates_api.inc -- part of api.hip: per-stream sample rates on the device path, one call per side.
//   lyra_hip_encode_rates_dev: LyraEncoder::Encode (lyra_encoder.cc:113-156) for a batch whose encoders were created at
//     different rates (LyraEncoder::Create, lyra_encoder.cc:59: no resampler at 16 kHz): resample_rates_kernel (each row's own
//     design -> the 16 kHz hop, and the id list with -1 where the rate is no codec rate), then encode16 on that list
//     with logmel_rates_kernel as the DTX estimator (each row's own filterbank and constants, noise_estimator.cc:96-124).
//   lyra_hip_decode_lossy_rates_dev: lossy_tick_launch with resample_rates_kernel (16 kHz -> each row's rate) as the last
//     launch of the tick's noise-stream call; the decoder-side estimator is a 16 kHz one at every rate (lyra_decoder.cc:129).
// Neither reads lyra_hip_set_encoder_sample_rate's setting; neither splits on contexts with LYRA_HIP_SUBBATCHES > 1.

namespace {

void rates_free(lyra_hip_ctx* c) {
  dfree(c->d_rs_tab, c->d_noise_tab, c->d_rates_err, c->d_rates_bits);
  c->rates_bits_val = -1;
}

// The tables the per-row kernels index by rate: built by the very functions the uniform calls pass by value
// (resample_design, noise_params), so every float is the same.
int rates_ensure(lyra_hip_ctx* c) {
  if (c->d_rs_tab) return 0;
  static const int kRs[3] = {8000, 32000, 48000}, kAll[4] = {8000, 16000, 32000, 48000};
  std::vector<ResampleP> tab(6);
  for (int i = 0; i < 3; ++i)
    if (!resample_design(kRs[i], 16000, &tab[i]) || !resample_design(16000, kRs[i], &tab[3 + i]))
      return fail(c, LYRA_HIP_EHIP, "rates: resampler design");
  NoiseP np[4];
  for (int i = 0; i < 4; ++i) np[i] = noise_params(kAll[i]);
  if (const int rc = err_word_ensure(c, &c->d_rates_err)) return rc;
  HIPCHK(c, dalloc(&c->d_rs_tab, tab.size()));
  HIPCHK(c, dalloc(&c->d_noise_tab, 4));
  HIPCHK(c, hipMemcpy(c->d_rs_tab, tab.data(), tab.size() * sizeof(ResampleP), hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->d_noise_tab, np, sizeof np, hipMemcpyHostToDevice));
  HIPCHK(c, set_lds(logmel_rates_kernel, logmel_rates_lds_bytes()));
  HIPCHK(c, set_lds(logmel_streams_kernel, logmel_rates_lds_bytes()));
  return 0;
}

// launch_noise(side 0) with the rate per row; rows of id -1 are skipped.  d_dtx (lyra_hip_encode_streams_dev): one flag per
// row, rows without DTX pass through.
int launch_noise_rates(lyra_hip_ctx* c, hipStream_t st_, const int32_t* d_ids, const int32_t* d_rates, int B,
                       const int16_t* d_pcm, int32_t* d_is_noise, int32_t* d_masked_ids, const int32_t* d_dtx) {
  { ProfScope ps(c, K_NOISE, st_);
    if (d_dtx)
      hipLaunchKernelGGL(logmel_streams_kernel, dim3(cdiv(B, 2)), dim3(256), logmel_rates_lds_bytes(), st_, c->model.d_mel_rate[0],
                         d_pcm, d_ids, d_rates, d_dtx, B, c->sm.base[st::R_NOISE_E], (int)st::NOISE_BYTES, (int)st::N_PREV,
                         (const NoiseP*)c->d_noise_tab, d_is_noise, d_masked_ids);
    else
    hipLaunchKernelGGL(logmel_rates_kernel, dim3(cdiv(B, 2)), dim3(256), logmel_rates_lds_bytes(), st_, c->model.d_mel_rate[0],
                       d_pcm, d_ids, d_rates, B, c->sm.base[st::R_NOISE_E], (int)st::NOISE_BYTES, (int)st::N_PREV,
                       (const NoiseP*)c->d_noise_tab, d_is_noise, d_masked_ids); }
  HIPCHK(c, hipGetLastError());
  return 0;
}

// launch_resample with the design per row.  dir 0: the encoder's slots, rows in_stride apart in, 320 out; dir 1: the decoder's.
int launch_resample_rates(lyra_hip_ctx* c, int dir, const int32_t* d_ids, const int32_t* d_rates, int B, const int16_t* d_in,
                          int in_stride, int16_t* d_out, int out_stride, int32_t* d_ids_out, hipStream_t st_) {
  { ProfScope ps(c, K_RESAMPLE, st_);
    hipLaunchKernelGGL(resample_rates_kernel, dim3(cdiv(B, 4)), dim3(256), resample_rates_lds_bytes(), st_,
                       (const ResampleP*)c->d_rs_tab, dir, d_rates, d_ids, B, c->sm.base[dir == 0 ? st::R_RS_E : st::R_RS_D], d_in,
                       in_stride, d_out, out_stride, d_ids_out, c->d_rates_err); }
  HIPCHK(c, hipGetLastError());
  return 0;
}

// encode_ext_resample with the rate per row: *in = the 16 kHz hops, *ids = the id list of the rows with a codec rate.
// n_pcm >= 0 (lyra_hip_encode_streams_dev): d_pcm_ext holds n_pcm samples with row b at d_offsets[b] (null: b * 960), and a
// row that leaves the buffer is named -1 too (resample_streams_kernel).
int encode_rates_resample(lyra_hip_ctx* c, const int32_t* d_ids, const int32_t* d_rates, int B, const int16_t* d_pcm_ext,
                          const int16_t** in, const int32_t** ids, const int32_t* d_offsets, long n_pcm) {
  DEVSCOPE(c);
  int rc = ensure_scratch(c, B);
  if (rc) return rc;
  if ((rc = wait_ahead(c))) return rc;
  if ((rc = encq_begin(c, 0, 1))) return rc;
  // The id list travels with the call's features and `live`: without DTX it is the quantizer's mask, read on sq[0] while the
  // next call's resampler already runs on se[0].  One list per call parity, rewritten only after the quantizer of the call
  // before the previous one (encq_buffer_free), as encode16 does for `live`.
  int32_t* vids = c->d_rate_ids_call[c->n_encq_calls & 1];
  const EventList busy = encq_buffer_free(c, 0, 1);
  for (int i = 0; i < busy.n; ++i) HIPCHK(c, hipStreamWaitEvent(c->se[0], busy.e[i], 0));
  if (n_pcm >= 0) {
    { ProfScope ps(c, K_RESAMPLE, c->se[0]);
      hipLaunchKernelGGL(resample_streams_kernel, dim3(cdiv(B, 4)), dim3(256), resample_rates_lds_bytes(), c->se[0],
                         (const ResampleP*)c->d_rs_tab, d_rates, d_ids, B, c->sm.base[st::R_RS_E], d_pcm_ext, d_offsets,
                         (int)LYRA_HIP_MAX_EXT_HOP, n_pcm, c->d_rs16[0], 320, vids, c->d_rates_err); }
    HIPCHK(c, hipGetLastError());
  } else if ((rc = launch_resample_rates(c, 0, d_ids, d_rates, B, d_pcm_ext, LYRA_HIP_MAX_EXT_HOP, c->d_rs16[0], 320, vids,
                                         c->se[0]))) {
    return rc;
  }
  if ((rc = se0_to_chunks(c))) return rc;
  *in = c->d_rs16[0];
  *ids = vids;
  return 0;
}

// resample_in_ahead with the rate per row (run_steps, MIXED_RATE): hop `step` on the quantizer stream, two steps ahead
int resample_rates_in_ahead(lyra_hip_ctx* c, const int32_t* d_ids, const int32_t* d_rates, int B, const int16_t* d_in, long step) {
  const int p = (int)(step % lyra_hip_ctx::RS_RING);
  int rc = launch_resample_rates(c, 0, d_ids, d_rates, B, d_in, LYRA_HIP_MAX_EXT_HOP, c->d_rs16[p], 320, c->d_rate_ids[p], c->sq[0]);
  if (rc) return rc;
  HIPCHK(c, hipEventRecord(c->ev_rs_in[p], c->sq[0]));
  return ahead_end(c);
}

// run_steps, MIXED_RATE without MIXED_BITRATE: num_bits in every row of a library buffer (rewritten only when it changes)
int rates_uniform_bits(lyra_hip_ctx* c, int num_bits, const int32_t** bits) {
  DEVSCOPE(c);
  if (!c->d_rates_bits) HIPCHK(c, dalloc(&c->d_rates_bits, (size_t)c->max_streams));
  if (c->rates_bits_val != num_bits) {
    int rc = sync_all(c);   // (calls in flight may still read the old value)
    if (rc) return rc;
    const std::vector<int32_t> h((size_t)c->max_streams, num_bits);
    HIPCHK(c, hipMemcpy(c->d_rates_bits, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    c->rates_bits_val = num_bits;
  }
  *bits = c->d_rates_bits;
  return 0;
}

}  // namespace

extern "C" {

int lyra_hip_encode_rates_dev(lyra_hip_ctx* c, const int32_t* d_ids, int B, const int16_t* d_pcm_ext,
                              const int32_t* d_sample_rates, const int32_t* d_num_bits, int dtx, uint8_t* d_packets,
                              int32_t* d_packet_bytes) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (!d_ids || !d_pcm_ext || !d_sample_rates || !d_num_bits || !d_packets || !d_packet_bytes)
    return fail(c, LYRA_HIP_EINVAL, "encode_rates: null pointer");
  { DEVSCOPE(c); if ((rc = rates_ensure(c))) return rc; }
  const int16_t* in = nullptr;
  const int32_t* ids = nullptr;
  if ((rc = encode_rates_resample(c, d_ids, d_sample_rates, B, d_pcm_ext, &in, &ids))) return rc;
  return encode16(c, ids, B, in, dtx != 0, 0, d_num_bits, d_sample_rates, d_packets, d_packet_bytes);
}

int lyra_hip_decode_lossy_rates_dev(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_packets,
                                    const int32_t* d_packet_bytes, const int32_t* d_sample_rates, int16_t* d_pcm16,
                                    int16_t* d_pcm_ext, int32_t* d_is_noise, int32_t* d_is_comfort_noise) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (!d_ids || !d_packets || !d_packet_bytes || !d_sample_rates || !d_pcm16 || !d_pcm_ext)
    return fail(c, LYRA_HIP_EINVAL, "decode_lossy_rates: null pointer");
  { DEVSCOPE(c); if ((rc = rates_ensure(c))) return rc; }
  return lossy_tick_launch(c, d_ids, B, d_packets, d_packet_bytes, nullptr, 0, 16000, d_pcm16, d_pcm_ext, d_is_noise,
                           d_is_comfort_noise, LOSSY_MIXED_BYTES, d_sample_rates);
}

long lyra_hip_rates_errors(lyra_hip_ctx* c, int clear) {
  return read_error_counter(c, &lyra_hip_ctx::d_rates_err, clear);
}

}  // extern "C"
