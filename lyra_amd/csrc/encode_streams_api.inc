// encode_streams_api.inc -- part of api.hip: encoders of any rate, bitrate and DTX setting in one batch
// (include/lyra_hip_encode_streams.h).
//   lyra_hip_encode_streams_dev: lyra_hip_encode_rates_dev with the DTX switch per row (logmel_streams_kernel: a row without
//     DTX takes the path of an absent row through the estimator, lyra_encoder.cc:80) and with audio rows at offsets of their
//     own inside one buffer (resample_streams_kernel: a row that leaves the buffer is an absent row).
//   lyra_hip_encode_streams_begin / _end: its two-deep host-buffer form, as lyra_hip_encode_begin / _end (pipe_api.inc); where
//     the arrays lie in the slot: host_staging::encode_streams.  begin() waits for the audio upload on the host in every branch, so the caller's buffer is free on
//     return and no kernel needs a cross-stream edge behind a copy.
#include "../../include/lyra_hip_encode_streams.h"

extern "C" {

int lyra_hip_encode_streams_dev(lyra_hip_ctx* c, const int32_t* d_ids, int B, const int16_t* d_pcm_ext, long n_pcm_samples,
                                const int32_t* d_pcm_offsets, const int32_t* d_sample_rates, const int32_t* d_num_bits,
                                const int32_t* d_dtx, uint8_t* d_packets, int32_t* d_packet_bytes) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (!d_ids || !d_pcm_ext || !d_sample_rates || !d_num_bits || !d_packets || !d_packet_bytes)
    return fail(c, LYRA_HIP_EINVAL, "encode_streams: null pointer");
  if (n_pcm_samples < 0) return fail(c, LYRA_HIP_EINVAL, "encode_streams: n_pcm_samples %ld", n_pcm_samples);
  { DEVSCOPE(c); if ((rc = rates_ensure(c))) return rc; }
  const int16_t* in = nullptr;
  const int32_t* ids = nullptr;
  if ((rc = encode_rates_resample(c, d_ids, d_sample_rates, B, d_pcm_ext, &in, &ids, d_pcm_offsets, n_pcm_samples))) return rc;
  return encode16(c, ids, B, in, d_dtx != nullptr, 0, d_num_bits, d_sample_rates, d_packets, d_packet_bytes, d_dtx);
}

int lyra_hip_encode_streams_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const int16_t* pcm, const int32_t* sample_rates,
                                  const int32_t* num_bits, const int32_t* dtx) {
  if (!c) return LYRA_HIP_EINVAL;
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (!pcm || !sample_rates || !num_bits) return fail(c, LYRA_HIP_EINVAL, "encode_streams_begin: null pointer");
  if ((rc = check_ids_host(c, ids, B))) return rc;
  for (int b = 0; b < B; ++b) {
    if ((rc = check_rate(c, sample_rates[b]))) return rc;
    if ((rc = check_bits(c, num_bits[b]))) return rc;
  }
  if ((rc = pl_admit(c, PL_ENCODE_STREAMS, "encode_streams_begin"))) return rc;
  DEVSCOPE(c);
  if ((rc = ensure_scratch(c, B))) return rc;
  if ((rc = rates_ensure(c))) return rc;
  HostSlot& S = host_slot_begin(c, PL_ENCODE_STREAMS);
  const host_staging::EncodeStreams L = host_staging::encode_streams((size_t)B, (size_t)c->max_streams);
  if ((rc = host_slot_ensure(c, S, L.room))) return rc;
  std::memcpy(S.h_in + L.ids, ids, (size_t)B * 4);
  std::memcpy(S.h_in + L.rates, sample_rates, (size_t)B * 4);
  std::memcpy(S.h_in + L.bits, num_bits, (size_t)B * 4);
  int32_t* h_dtx = slot_at<int32_t>(S.h_in, L.dtx);
  int32_t* h_offsets = slot_at<int32_t>(S.h_in, L.offsets);
  long total = 0;
  for (int b = 0; b < B; ++b) {
    h_dtx[b] = dtx ? (dtx[b] != 0) : 0;
    h_offsets[b] = (int32_t)total;   // (at most max_streams * 960 < 2^31: lyra_hip_create's bound on max_streams)
    total += sample_rates[b] / 50;
  }
  // With another call of this pipeline in flight the uploads go on the copy stream (the noise stream, as pipe_api.inc) and run
  // under its kernels; with none, on the extractor's own stream.  Either way the host waits for them HERE: `pcm` is the
  // caller's again on return, and every kernel below is enqueued after its inputs have arrived.  (The noise stream also ends
  // the decode-side calls: on a context that decodes as well this wait covers decoder kernels that are on it -- see the header.)
  hipStream_t up = c->pl_begun[PL_ENCODE_STREAMS] != c->pl_ended[PL_ENCODE_STREAMS] ? c->sn : c->se[0];
  uint8_t* d_meta = S.d_in + L.d_meta;
  int16_t* d_pcm = slot_at<int16_t>(S.d_in, L.d_pcm);
  uint8_t* d_pk = S.d_out + L.d_packets;
  int32_t* d_len = slot_at<int32_t>(S.d_out, L.d_packet_bytes);
  HIPCHK(c, hipMemcpyAsync(d_meta, S.h_in, L.meta_bytes, hipMemcpyHostToDevice, up));
  HIPCHK(c, hipMemcpyAsync(d_pcm, pcm, (size_t)total * 2, hipMemcpyHostToDevice, up));
  HIPCHK(c, hipStreamSynchronize(up));
  // empty packets, and the bytes behind a shorter one, read back as zeros; the extractor's stream is ahead of the quantizer's
  HIPCHK(c, hipMemsetAsync(d_pk, 0, (size_t)B * LYRA_HIP_MAX_PACKET_BYTES, c->se[0]));
  if ((rc = lyra_hip_encode_streams_dev(c, slot_at<int32_t>(d_meta, L.ids), B, d_pcm, total, slot_at<int32_t>(d_meta, L.offsets),
                                        slot_at<int32_t>(d_meta, L.rates), slot_at<int32_t>(d_meta, L.bits),
                                        dtx ? slot_at<int32_t>(d_meta, L.dtx) : nullptr, d_pk, d_len)))
    return rc;
  // packets and lengths are written by the quantizer on sq[0] (the call is not split): their download rides on that stream
  HIPCHK(c, hipMemcpyAsync(S.h_out + L.h_packets, d_pk, (size_t)B * LYRA_HIP_MAX_PACKET_BYTES, hipMemcpyDeviceToHost, c->sq[0]));
  HIPCHK(c, hipMemcpyAsync(S.h_out + L.h_packet_bytes, d_len, (size_t)B * 4, hipMemcpyDeviceToHost, c->sq[0]));
  return host_slot_begun(c, PL_ENCODE_STREAMS, S, B, c->sq[0]);
}

int lyra_hip_encode_streams_end(lyra_hip_ctx* c, uint8_t* packets, int32_t* packet_bytes) {
  if (!c) return LYRA_HIP_EINVAL;
  HostSlot* oldest = host_slot_oldest(c, PL_ENCODE_STREAMS);
  if (!oldest) return LYRA_HIP_EINVAL;
  if (!packets || !packet_bytes) return fail(c, LYRA_HIP_EINVAL, "encode_streams_end: null pointer");
  DEVSCOPE(c);
  HostSlot& S = *oldest;
  if (const int rc = host_slot_ended(c, PL_ENCODE_STREAMS, S, true)) return rc;
  const host_staging::EncodeStreams L = host_staging::encode_streams((size_t)S.B, (size_t)c->max_streams);
  std::memcpy(packets, S.h_out + L.h_packets, (size_t)S.B * LYRA_HIP_MAX_PACKET_BYTES);
  std::memcpy(packet_bytes, S.h_out + L.h_packet_bytes, (size_t)S.B * 4);
  return 0;
}

}  // extern "C"
