// decode_streams_api.inc -- part of api.hip: decoders of any sample rate and packet size in one batch, the hop-synchronous
// receiver (include/lyra_hip_decode_streams.h).
//   lyra_hip_decode_streams_dev: lyra_hip_decode_lossy_rates_dev with each row's samples at an offset of its own inside one
//     buffer (resample_streams_out_kernel: a row that leaves the buffer writes nothing and leaves its resampler slot alone)
//     and with the 16 kHz hop optional (library scratch by call parity, as the tick's own buffers).  Nothing else of the
//     tick changes, so the packed form needs no state of its own.
//   lyra_hip_decode_streams_begin / _end: its two-deep host-buffer form, the input side as lyra_hip_decode_samples_begin
//     (pinned staging, uploaded on the decode-side stream, no synchronisation), the rest as lyra_hip_encode_streams_begin /
//     _end: one download behind the tick on the noise stream, end() waits for its event only.  Where the arrays lie in the
//     slot: host_staging::decode_streams.
#include "../../include/lyra_hip_decode_streams.h"

namespace {

void dstr_free(lyra_hip_ctx* c) {
  dfree(c->d_dstr16[0], c->d_dstr16[1]);
  c->dstr16_cap = 0;
}

// The 16 kHz hop of a call that was given no d_pcm16.  Two sets, picked by lossy-call parity as d_lossy_gan is.  The parity
// is NOT what keeps call n + 1 off call n's hop today: the mix that writes the hop and the resampler that reads it both run on
// the noise stream, in order, so one set would do.  Two are kept so that the scratch obeys the same rule as the tick's other
// per-call buffers and stays safe should a reader of the hop ever leave the noise stream.  Apart from the tick's own
// buffers, so that the calls that hand a d_pcm16 over never pay for it; allocated on first use.
int dstr16_ensure(lyra_hip_ctx* c, int B) {
  if (B <= c->dstr16_cap) return 0;
  int rc = sync_all(c);   // (the buffers of the calls in flight)
  if (rc) return rc;
  dfree(c->d_dstr16[0], c->d_dstr16[1]);
  c->dstr16_cap = 0;
  for (auto& p : c->d_dstr16) HIPCHK(c, dalloc(&p, (size_t)B * 320));
  c->dstr16_cap = B;
  return 0;
}

}  // namespace

extern "C" {

int lyra_hip_decode_streams_dev(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_packets,
                                const int32_t* d_packet_bytes, const int32_t* d_sample_rates, int16_t* d_pcm,
                                long n_pcm_samples, const int32_t* d_pcm_offsets, int16_t* d_pcm16, int32_t* d_is_noise,
                                int32_t* d_is_comfort_noise) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (!d_ids || !d_packets || !d_packet_bytes || !d_sample_rates || !d_pcm)
    return fail(c, LYRA_HIP_EINVAL, "decode_streams: null pointer");
  if (n_pcm_samples < 0) return fail(c, LYRA_HIP_EINVAL, "decode_streams: n_pcm_samples %ld", n_pcm_samples);
  { DEVSCOPE(c);
    if ((rc = rates_ensure(c))) return rc;
    if (!d_pcm16) {
      if ((rc = dstr16_ensure(c, B))) return rc;
      d_pcm16 = c->d_dstr16[c->n_lossy_calls & 1];
    } }
  return lossy_tick_launch(c, d_ids, B, d_packets, d_packet_bytes, nullptr, 0, 16000, d_pcm16, d_pcm, d_is_noise,
                           d_is_comfort_noise, LOSSY_MIXED_BYTES, d_sample_rates, d_pcm_offsets, n_pcm_samples);
}

int lyra_hip_decode_streams_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets,
                                  const int32_t* packet_bytes, const int32_t* sample_rates) {
  if (!c) return LYRA_HIP_EINVAL;
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (!packets || !packet_bytes || !sample_rates) return fail(c, LYRA_HIP_EINVAL, "decode_streams_begin: null pointer");
  if ((rc = check_ids_host(c, ids, B))) return rc;
  for (int b = 0; b < B; ++b) {
    if ((rc = check_rate(c, sample_rates[b]))) return rc;
    const int pb = packet_bytes[b];   // PacketSizeToNumQuantizedBits (lyra_config.h:99-106), 0: no packet on this hop
    if (pb != 0 && pb != 8 && pb != 15 && pb != LYRA_HIP_MAX_PACKET_BYTES)
      return fail(c, LYRA_HIP_EINVAL, "decode_streams_begin: packet of %d bytes at position %d (0, 8, 15 or 23)", pb, b);
  }
  if ((rc = pl_admit(c, PL_DECODE_STREAMS, "decode_streams_begin"))) return rc;
  DEVSCOPE(c);
  if ((rc = ensure_scratch(c, B))) return rc;
  HostSlot& S = host_slot_begin(c, PL_DECODE_STREAMS);
  const host_staging::DecodeStreams L = host_staging::decode_streams((size_t)B, (size_t)c->max_streams);
  if ((rc = host_slot_ensure(c, S, L.room))) return rc;
  // everything the tick allocates or builds on first use, BEFORE anything is enqueued: a failure here leaves the streams idle
  if ((rc = rates_ensure(c))) return rc;
  if ((rc = lossy_ensure(c, B))) return rc;
  if ((rc = dstr16_ensure(c, B))) return rc;
  std::memcpy(S.h_in + L.ids, ids, (size_t)B * 4);
  std::memcpy(S.h_in + L.packet_bytes, packet_bytes, (size_t)B * 4);
  std::memcpy(S.h_in + L.rates, sample_rates, (size_t)B * 4);
  int32_t* h_offsets = slot_at<int32_t>(S.h_in, L.offsets);
  long total = 0;
  for (int b = 0; b < B; ++b) {
    h_offsets[b] = (int32_t)total;   // (at most max_streams * 960 < 2^31: lyra_hip_create's bound on max_streams)
    total += sample_rates[b] / 50;
  }
  std::memcpy(S.h_in + L.packets, packets, (size_t)B * LYRA_HIP_MAX_PACKET_BYTES);
  // one upload from pinned staging on the decode-side stream, in front of the tick's first kernel: the caller's arrays are
  // free on return and nothing waits on the host
  HIPCHK(c, hipMemcpyAsync(S.d_in, S.h_in, L.in_bytes, hipMemcpyHostToDevice, c->sd[0]));
  if ((rc = lyra_hip_decode_streams_dev(c, slot_at<int32_t>(S.d_in, L.ids), B, S.d_in + L.packets,
                                        slot_at<int32_t>(S.d_in, L.packet_bytes), slot_at<int32_t>(S.d_in, L.rates),
                                        slot_at<int16_t>(S.d_out, L.pcm), total, slot_at<int32_t>(S.d_in, L.offsets), nullptr,
                                        slot_at<int32_t>(S.d_out, L.is_noise), slot_at<int32_t>(S.d_out, L.is_comfort_noise))))
    return rc;
  // flags and samples are written by the noise-stream half: their download rides on that stream, behind the resampler
  HIPCHK(c, hipMemcpyAsync(S.h_out, S.d_out, L.pcm + (size_t)total * 2, hipMemcpyDeviceToHost, c->sn));
  S.total = total;
  return host_slot_begun(c, PL_DECODE_STREAMS, S, B, c->sn);
}

int lyra_hip_decode_streams_end(lyra_hip_ctx* c, int16_t* pcm, int32_t* is_noise, int32_t* is_comfort_noise) {
  if (!c) return LYRA_HIP_EINVAL;
  HostSlot* oldest = host_slot_oldest(c, PL_DECODE_STREAMS);
  if (!oldest) return LYRA_HIP_EINVAL;
  if (!pcm) return fail(c, LYRA_HIP_EINVAL, "decode_streams_end: null pointer");
  DEVSCOPE(c);
  HostSlot& S = *oldest;
  if (const int rc = host_slot_ended(c, PL_DECODE_STREAMS, S, true)) return rc;
  const size_t n = (size_t)S.B;
  const host_staging::DecodeStreams L = host_staging::decode_streams(n, (size_t)c->max_streams);
  if (is_noise) std::memcpy(is_noise, S.h_out + L.is_noise, n * 4);
  if (is_comfort_noise) std::memcpy(is_comfort_noise, S.h_out + L.is_comfort_noise, n * 4);
  std::memcpy(pcm, S.h_out + L.pcm, (size_t)S.total * 2);
  return 0;
}

}  // extern "C"
