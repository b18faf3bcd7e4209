// mixed_api.inc -- part of api.hip: per-stream bitrates on the device path, one call per side.
//   lyra_hip_encode_mixed_dev: LyraEncoder::Encode (lyra_encoder.cc:113-156) with each stream's own bitrate (set_bitrate,
//     :158-166): resampler, DTX decision, feature extractor as lyra_hip_encode_ext_dev, then rvq_encode_mixed_kernel -- every
//     frame at bits[b] / 4 stages, packet rows LYRA_HIP_MAX_PACKET_BYTES apart.
//   lyra_hip_decode_lossy_mixed_dev: lossy_tick_launch with the sizes of SetEncodedPacket's PacketSizeToNumQuantizedBits
//     (lyra_decoder.cc:172-179, lyra_config.h:99-106) per row: rvq_decode_mixed_kernel + lossy_plan_mixed_kernel.
// Neither splits on contexts with LYRA_HIP_SUBBATCHES > 1 (one call stands for every chunk, as lyra_hip_encode_dtx_dev and
// lyra_hip_decode_lossy_dev do).
#include "lossy_plan.h"

static_assert(lyra::MAX_PACKET_BYTES == LYRA_HIP_MAX_PACKET_BYTES, "packet row stride of the mixed kernels");

namespace {

// One unsplit encode-side call at 16 kHz: [noise estimator ->] extractor on se[0], quantizer on sq[0] (the structure of
// lyra_hip_encode_dev with one chunk, and of lyra_hip_encode_dtx_dev).  d_rates (rates_api.inc): the estimator runs with each
// row's own rate, and d_ids may hold -1 for rows that are absent from this hop (no state advances, packet_bytes 0).
int encode_mixed16(lyra_hip_ctx* c, const int32_t* d_ids, int B, const int16_t* d_pcm, const int32_t* d_bits, bool dtx,
                   uint8_t* d_packets, int32_t* d_packet_bytes, const int32_t* d_rates) {
  DEVSCOPE(c);
  int rc = ensure_scratch(c, B);
  if (rc) return rc;
  if (!c->d_mixed_err) {
    HIPCHK(c, dalloc(&c->d_mixed_err, 1));
    HIPCHK(c, hipMemset(c->d_mixed_err, 0, 4));
  }
  if ((rc = encq_begin(c, 0))) return rc;
  float* feat = encq_features(c);
  int32_t* live = nullptr;
  if (dtx) {   // as lyra_hip_encode_dtx_dev: the mask travels with the features, one buffer per parity
    live = (c->n_encq_calls & 1) ? c->d_live_ids2 : c->d_live_ids;
    const EventList busy = encq_buffer_free(c, 0, 1);
    for (int i = 0; i < busy.n; ++i) HIPCHK(c, hipStreamWaitEvent(c->se[0], busy.e[i], 0));
    rc = d_rates ? launch_noise_rates(c, c->se[0], d_ids, d_rates, B, d_pcm, c->d_flag_enc, live)
                 : launch_noise(c, 0, c->se[0], d_ids, B, d_pcm, c->d_flag_enc, live);
    if (!rc) rc = launch_extract(c, 0, 0, live, B, d_pcm, feat);
  } else {
    rc = launch_extract(c, 0, 0, d_ids, B, d_pcm, feat, encq_buffer_free(c, 0, 1));
  }
  if (!rc) rc = encq_handoff(c, 0);
  if (!rc) {
    { ProfScope ps(c, K_RVQ_ENC, c->sq[0]);
      hipLaunchKernelGGL(rvq_encode_mixed_kernel, dim3(cdiv(B, 16)), dim3(64), 0, c->sq[0], c->model.cb, c->model.cbn, feat, B,
                         d_bits, d_packets, (const int32_t*)(live ? live : d_rates ? d_ids : nullptr), d_packet_bytes, c->d_rvq_stats, c->d_mixed_err); }
    HIPCHK(c, hipGetLastError());
    rc = encq_done(c, 0);
  }
  c->encq_nk[c->n_encq_calls & 1] = 1;
  c->n_encq_calls++;
  c->enc_last_nk = 1;
  return rc;
}

}  // namespace

extern "C" {

int lyra_hip_encode_mixed_dev(lyra_hip_ctx* c, const int32_t* d_ids, int B, const int16_t* d_pcm_ext, int sample_rate_hz,
                              const int32_t* d_num_bits, int dtx, uint8_t* d_packets, int32_t* d_packet_bytes) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if ((rc = check_rate(c, sample_rate_hz))) return rc;
  if (!d_ids || !d_pcm_ext || !d_num_bits || !d_packets || !d_packet_bytes)
    return fail(c, LYRA_HIP_EINVAL, "encode_mixed: null pointer");
  const int ext = sample_rate_hz;
  if (dtx && c->enc_noise_rate != ext)   // as lyra_hip_encode_ext_dev
    return fail(c, LYRA_HIP_EINVAL, "encode_mixed: DTX at %d Hz but the encoder-side noise estimator is set up for %d Hz "
                "(call lyra_hip_set_encoder_sample_rate(%d) first)", ext, c->enc_noise_rate, ext);
  const int16_t* in = d_pcm_ext;
  if (ext != 16000 && (rc = encode_ext_resample(c, d_ids, B, d_pcm_ext, ext, &in))) return rc;
  return encode_mixed16(c, d_ids, B, in, d_num_bits, dtx != 0, d_packets, d_packet_bytes);
}

long lyra_hip_encode_mixed_errors(lyra_hip_ctx* c, int clear) {
  if (!c) return LYRA_HIP_EINVAL;
  if (!c->d_mixed_err) return 0;
  DEVSCOPE(c);
  int rc = sync_all(c);
  if (rc) return rc;
  unsigned n = 0;
  HIPCHK(c, hipMemcpy(&n, c->d_mixed_err, 4, hipMemcpyDeviceToHost));
  if (clear) HIPCHK(c, hipMemset(c->d_mixed_err, 0, 4));
  return (long)n;
}

int lyra_hip_decode_lossy_mixed_dev(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_packets,
                                    const int32_t* d_packet_bytes, int sample_rate_hz, int16_t* d_pcm16, int16_t* d_pcm_ext,
                                    int32_t* d_is_noise, int32_t* d_is_comfort_noise) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if ((rc = check_rate(c, sample_rate_hz))) return rc;
  if (!d_ids || !d_packets || !d_packet_bytes || !d_pcm16 || (sample_rate_hz != 16000 && !d_pcm_ext))
    return fail(c, LYRA_HIP_EINVAL, "decode_lossy_mixed: null pointer");
  return lossy_tick_launch(c, d_ids, B, d_packets, d_packet_bytes, nullptr, 0, sample_rate_hz, d_pcm16, d_pcm_ext, d_is_noise,
                           d_is_comfort_noise, LOSSY_MIXED_BYTES);
}

}  // extern "C"
