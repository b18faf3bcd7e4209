// decode_samples_streams_api.inc -- part of api.hip: lyra_hip_decode_samples_streams_dev
// (include/lyra_hip_decode_samples_streams.h), lyra_hip_decode_samples_any_dev with a sample rate, a request size and an output
// offset per row (decode_samples_streams_plan.h).  The call is the any-size call's (ds_run, decode_samples_api.inc) with
//   - max_hops rounds, given by the caller: the rows' sizes are on the device, a launch count is not;
//   - ds_plan_streams_kernel in place of ds_plan_any_kernel: round 0 validates each row and plans an invalid one as a row
//     without a packet and with a request of 0 samples;
//   - ds_slice_kernel ALWAYS into the internal-rate scratch [cap][1280] (unchanged: its stride is a launch constant, and the
//     flags it writes are those of the uniform call), and ds_splice_streams_kernel behind the last round for every rate: the
//     resampler of the row's own design from the context's table, or the copy of a 16 kHz row to its offset.
// Every other kernel, the per-round and per-parity buffering (Dsa's buffers are shared: the three DecodeSamples calls take
// turns by n_ds_calls) and the "count on the decode stream, samples on the noise stream" rule are the any-size call's.
#include "decode_samples_streams_plan.h"
#include "../../include/lyra_hip_decode_samples_streams.h"

static_assert(lyra::DSS_ROW_STRIDE == LYRA_HIP_DECODE_SAMPLES_MAX_HOPS * LYRA_HIP_MAX_EXT_HOP, "documented default row stride");

namespace {

static_assert(host_staging::MAX_HOPS * host_staging::MAX_EXT_HOP == lyra::DSS_ROW_STRIDE, "the staging's rows are the call's");

void dss_free(lyra_hip_ctx* c) {
  dfree(c->dss.d_call);
  c->dss.cap = 0;
}

int dss_ensure(lyra_hip_ctx* c, int B) {
  Dss* A = &c->dss;
  if (B <= A->cap) return 0;
  int rc = sync_all(c);   // (the words of the calls in flight)
  if (rc) return rc;
  dfree(A->d_call);
  A->cap = 0;
  HIPCHK(c, dalloc(&A->d_call, (size_t)2 * DSS_CALL_WORDS * (size_t)B));
  A->cap = B;
  return 0;
}

// everything the call allocates or builds on first use
int dss_ensure_all(lyra_hip_ctx* c, int B) {
  int rc = ensure_scratch(c, B);
  if (!rc) rc = rates_ensure(c);   // the per-row designs and the invalid-row counter
  if (!rc) rc = ds_ensure(c, B);   // the streams' rings and held hops, the error word, the rows the DecodeSamples calls share
  if (!rc) rc = dsa_ensure(c, B);  // the per-round buffers and the internal-rate scratch of the any-size call
  if (!rc) rc = dss_ensure(c, B);
  return rc;
}

int dss_launch(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_packets, const int32_t* d_pkt_bytes,
               const int32_t* d_rates, const int32_t* d_sizes, int max_hops, int16_t* d_pcm, long n_pcm,
               const int32_t* d_offsets, int32_t* d_is_noise, int32_t* d_is_cn) {
  DEVSCOPE(c);
  int rc = dss_ensure_all(c, B);
  if (rc) return rc;
  Dsa* A = dsa_of(c);
  const Dss* S = &c->dss;
  const size_t set = (size_t)(c->n_ds_calls & 1);
  DsCall K = {d_ids, B, d_packets, d_pkt_bytes, max_hops, true, nullptr, nullptr, nullptr, 0, A->d_pcm16, DSA_MAX_INTERNAL, true,
              d_is_noise, d_is_cn};
  dsa_round_bufs(A, set, &K);
  int32_t* call = S->d_call + set * DSS_CALL_WORDS * (size_t)S->cap;
  return ds_run(
      c, K,
      [&](int r) {
        hipLaunchKernelGGL(ds_plan_streams_kernel, dim3(cdiv(B, 256)), dim3(256), 0, c->sd[0], d_ids, B,
                           r == 0 ? d_pkt_bytes : nullptr, r, d_rates, d_sizes, d_offsets, max_hops, n_pcm, c->sm.base[st::R_RS_D],
                           call, c->sm.base[st::R_CNG], K.ids_of(r, 0), K.ids_of(r, 1), K.ids_of(r, 2), K.ids_of(r, 3), K.info_of(r),
                           c->d_ds_feat, c->d_ds_ring, c->d_ds_err, c->d_rates_err);
      },
      [&] {
        { ProfScope ps(c, K_RESAMPLE, c->sn);
          hipLaunchKernelGGL(ds_splice_streams_kernel, dim3(cdiv(B, 4)), dim3(256), ds_splice_lds_bytes(), c->sn,
                             (const ResampleP*)c->d_rs_tab, d_ids, B, (const int32_t*)call, c->sm.base[st::R_RS_D],
                             (const int16_t*)A->d_pcm16, DSA_MAX_INTERNAL, d_pcm, d_offsets); }
        HIPCHK(c, hipGetLastError());
        return 0;
      });
}

}  // namespace

extern "C" {

int lyra_hip_decode_samples_streams_dev(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_packets,
                                        const int32_t* d_packet_bytes, const int32_t* d_sample_rates,
                                        const int32_t* d_num_samples, int max_hops, int16_t* d_pcm, long n_pcm_samples,
                                        const int32_t* d_pcm_offsets, int32_t* d_is_noise, int32_t* d_is_comfort_noise) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (!d_ids || !d_packets || !d_packet_bytes || !d_sample_rates || !d_num_samples || !d_pcm)
    return fail(c, LYRA_HIP_EINVAL, "decode_samples_streams: null pointer");
  if (max_hops < 1 || max_hops > DSA_MAX_HOPS)
    return fail(c, LYRA_HIP_EINVAL, "decode_samples_streams: max_hops %d outside 1..%d", max_hops, DSA_MAX_HOPS);
  if (n_pcm_samples < 0) return fail(c, LYRA_HIP_EINVAL, "decode_samples_streams: n_pcm_samples %ld", n_pcm_samples);
  return dss_launch(c, d_ids, B, d_packets, d_packet_bytes, d_sample_rates, d_num_samples, max_hops, d_pcm, n_pcm_samples,
                    d_pcm_offsets, d_is_noise, d_is_comfort_noise);
}

int lyra_hip_decode_samples_streams_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets,
                                          const int32_t* packet_bytes, const int32_t* sample_rates, const int32_t* num_samples) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if (!packets || !packet_bytes || !sample_rates || !num_samples)
    return fail(c, LYRA_HIP_EINVAL, "decode_samples_streams_begin: null pointer");
  if ((rc = check_ids_host(c, ids, B))) return rc;
  for (int b = 0; b < B; ++b) {
    const int v = dss_size_verdict(sample_rates[b], num_samples[b]);
    if (v == DSS_BAD_RATE) return check_rate(c, sample_rates[b]);
    if (v != DSS_OK)
      return fail(c, LYRA_HIP_EINVAL, "decode_samples_streams_begin: %d samples at %d Hz at position %d: a request must be 0..%d "
                  "samples (%d hops)", num_samples[b], sample_rates[b], b, DSA_MAX_HOPS * (sample_rates[b] / 50), DSA_MAX_HOPS);
    const int pb = packet_bytes[b];   // PacketSizeToNumQuantizedBits (lyra_config.h:99-106), 0: no packet
    if (pb != 0 && pb != 8 && pb != 15 && pb != LYRA_HIP_MAX_PACKET_BYTES)
      return fail(c, LYRA_HIP_EINVAL, "decode_samples_streams_begin: packet of %d bytes at position %d (0, 8, 15 or 23)", pb, b);
  }
  if ((rc = pl_admit(c, PL_DECODE_SAMPLES_STREAMS, "decode_samples_streams_begin"))) return rc;
  DEVSCOPE(c);
  // everything the call allocates or builds on first use, BEFORE anything is enqueued: a failure here leaves the streams idle
  // (the slot holds the rows of the largest request it has carried: it grows with B, unlike the other pipelines')
  HostSlot& S = host_slot_begin(c, PL_DECODE_SAMPLES_STREAMS);
  const size_t n = (size_t)B;
  const host_staging::DecodeSamplesStreams L = host_staging::decode_samples_streams(n);
  if ((rc = host_slot_ensure(c, S, L.room))) return rc;
  if ((rc = dss_ensure_all(c, B))) return rc;
  std::vector<long> offs(n);
  const long total = dss_packed_offsets(num_samples, B, offs.data());
  std::memcpy(S.h_in + L.ids, ids, n * 4);
  std::memcpy(S.h_in + L.packet_bytes, packet_bytes, n * 4);
  std::memcpy(S.h_in + L.rates, sample_rates, n * 4);
  std::memcpy(S.h_in + L.sizes, num_samples, n * 4);
  int32_t* h_offsets = slot_at<int32_t>(S.h_in, L.offsets);
  for (int b = 0; b < B; ++b) h_offsets[b] = (int32_t)offs[b];   // (at most max_streams * 3840 < 2^31: lyra_hip_create's bound on max_streams)
  std::memcpy(S.h_in + L.packets, packets, n * LYRA_HIP_MAX_PACKET_BYTES);
  // one upload from pinned staging on the decode-side stream, in front of the call's first kernel
  HIPCHK(c, hipMemcpyAsync(S.d_in, S.h_in, L.in_bytes, hipMemcpyHostToDevice, c->sd[0]));
  if ((rc = dss_launch(c, slot_at<int32_t>(S.d_in, L.ids), B, S.d_in + L.packets, slot_at<int32_t>(S.d_in, L.packet_bytes),
                       slot_at<int32_t>(S.d_in, L.rates), slot_at<int32_t>(S.d_in, L.sizes),
                       dss_batch_rounds(sample_rates, num_samples, B), slot_at<int16_t>(S.d_out, L.pcm), total,
                       slot_at<int32_t>(S.d_in, L.offsets), slot_at<int32_t>(S.d_out, L.is_noise),
                       slot_at<int32_t>(S.d_out, L.is_comfort_noise))))
    return rc;
  // flags and samples are written by the noise-stream half: their download rides on that stream, behind the splice
  HIPCHK(c, hipMemcpyAsync(S.h_out, S.d_out, L.pcm + (size_t)total * 2, hipMemcpyDeviceToHost, c->sn));
  S.total = total;
  return host_slot_begun(c, PL_DECODE_SAMPLES_STREAMS, S, B, c->sn);
}

int lyra_hip_decode_samples_streams_end(lyra_hip_ctx* c, int16_t* pcm, int32_t* is_noise, int32_t* is_comfort_noise) {
  if (!c) return LYRA_HIP_EINVAL;
  HostSlot* oldest = host_slot_oldest(c, PL_DECODE_SAMPLES_STREAMS);
  if (!oldest) return LYRA_HIP_EINVAL;
  HostSlot& S = *oldest;
  if (S.total > 0 && !pcm) return fail(c, LYRA_HIP_EINVAL, "decode_samples_streams_end: null pointer");
  DEVSCOPE(c);
  if (const int rc = host_slot_ended(c, PL_DECODE_SAMPLES_STREAMS, S, true)) return rc;
  const size_t n = (size_t)S.B;
  const host_staging::DecodeSamplesStreams L = host_staging::decode_samples_streams(n);
  if (is_noise) std::memcpy(is_noise, S.h_out + L.is_noise, n * 4);
  if (is_comfort_noise) std::memcpy(is_comfort_noise, S.h_out + L.is_comfort_noise, n * 4);
  if (S.total > 0) std::memcpy(pcm, S.h_out + L.pcm, (size_t)S.total * 2);
  return 0;
}

}  // extern "C"
