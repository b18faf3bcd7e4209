// mixed_api.inc -- part of api.hip: per-stream bitrates on the device path, one call per side.
//   lyra_hip_encode_mixed_dev: LyraEncoder::Encode (lyra_encoder.cc:113-156) with each stream's own bitrate (set_bitrate,
//     :158-166): resampler, DTX decision, feature extractor as lyra_hip_encode_ext_dev, then rvq_encode_mixed_kernel -- every
//     frame at bits[b] / 4 stages, packet rows LYRA_HIP_MAX_PACKET_BYTES apart (api.hip encode16 with d_bits).
//   lyra_hip_decode_lossy_mixed_dev: lossy_tick_launch with the sizes of SetEncodedPacket's PacketSizeToNumQuantizedBits
//     (lyra_decoder.cc:172-179, lyra_config.h:99-106) per row: rvq_decode_mixed_kernel + lossy_plan_mixed_kernel.
// Neither splits on contexts with LYRA_HIP_SUBBATCHES > 1 (one call stands for every chunk, as lyra_hip_encode_dtx_dev and
// lyra_hip_decode_lossy_dev do).
#include "lossy_plan.h"

static_assert(lyra::MAX_PACKET_BYTES == LYRA_HIP_MAX_PACKET_BYTES, "packet row stride of the mixed kernels");

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
  return encode16(c, d_ids, B, in, dtx != 0, 0, d_num_bits, nullptr, d_packets, d_packet_bytes);
}

long lyra_hip_encode_mixed_errors(lyra_hip_ctx* c, int clear) {
  return read_error_counter(c, &lyra_hip_ctx::d_mixed_err, clear);
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
