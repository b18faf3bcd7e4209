// encode_streams_api.inc -- part of api.hip: encoders of any rate, bitrate and DTX setting in one batch
// (include/lyra_hip_encode_streams.h).
//   lyra_hip_encode_streams_dev: lyra_hip_encode_rates_dev with the DTX switch per row (logmel_streams_kernel: a row without
//     DTX takes the path of an absent row through the estimator, lyra_encoder.cc:80) and with audio rows at offsets of their
//     own inside one buffer (resample_streams_kernel: a row that leaves the buffer is an absent row).
//   lyra_hip_encode_streams_begin / _end: its two-deep host-buffer form, as lyra_hip_encode_begin / _end (pipe_api.inc) with
//     slots of its own.  begin() waits for the audio upload on the host in every branch, so the caller's buffer is free on
//     return and no kernel needs a cross-stream edge behind a copy.
#include "../../include/lyra_hip_encode_streams.h"

namespace {

struct EsSlot {
  int32_t* h_meta = nullptr;   // pinned: [ids | rates | bits | dtx | offsets], B each (room for max_streams each)
  uint8_t* h_out = nullptr;    // pinned: [packets [max_streams][23] (24 apart per stream in total) | packet_bytes]
  int32_t* d_meta = nullptr;   // the same five arrays on the device
  int16_t* d_in = nullptr;     // [max_streams * 960] packed audio
  uint8_t* d_pk = nullptr;     // [max_streams][23]
  int32_t* d_len = nullptr;    // [max_streams]
  hipEvent_t ev_done = nullptr;
  int B = 0;
};
struct EsHost { EsSlot slot[2]; };

void es_free(lyra_hip_ctx* c) {
  EsHost* E = static_cast<EsHost*>(c->es_host);
  if (!E) return;
  for (EsSlot& S : E->slot) {
    if (S.h_meta) (void)hipHostFree(S.h_meta);
    if (S.h_out) (void)hipHostFree(S.h_out);
    dfree(S.d_meta, S.d_in, S.d_pk, S.d_len);
    if (S.ev_done) (void)hipEventDestroy(S.ev_done);
  }
  delete E;
  c->es_host = nullptr;
}

int es_slot_ensure(lyra_hip_ctx* c, EsSlot* S) {
  const size_t n = (size_t)c->max_streams;
  if (!S->h_meta) HIPCHK(c, hipHostMalloc((void**)&S->h_meta, n * 5 * 4, hipHostMallocDefault));
  if (!S->h_out) HIPCHK(c, hipHostMalloc((void**)&S->h_out, n * 24 + n * 4, hipHostMallocDefault));
  if (!S->d_meta) HIPCHK(c, dalloc(&S->d_meta, n * 5));
  if (!S->d_in) HIPCHK(c, dalloc(&S->d_in, n * LYRA_HIP_MAX_EXT_HOP));
  if (!S->d_pk) HIPCHK(c, dalloc(&S->d_pk, n * LYRA_HIP_MAX_PACKET_BYTES));
  if (!S->d_len) HIPCHK(c, dalloc(&S->d_len, n));
  if (!S->ev_done) HIPCHK(c, hipEventCreateWithFlags(&S->ev_done, hipEventDisableTiming));
  return 0;
}

}  // namespace

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
  if (!c->es_host) c->es_host = new EsHost();
  EsSlot& S = static_cast<EsHost*>(c->es_host)->slot[c->pl_begun[PL_ENCODE_STREAMS] & 1];
  if ((rc = es_slot_ensure(c, &S))) return rc;
  // (the slot's previous user, two calls back, has ended: its kernels have read d_meta / d_in, its download has left h_out)
  const size_t n = (size_t)B;
  int32_t* h = S.h_meta;
  long total = 0;
  for (int b = 0; b < B; ++b) {
    h[b] = ids[b];
    h[n + b] = sample_rates[b];
    h[2 * n + b] = num_bits[b];
    h[3 * n + b] = dtx ? (dtx[b] != 0) : 0;
    h[4 * n + b] = (int32_t)total;   // (at most max_streams * 960 < 2^31: lyra_hip_create's bound on max_streams)
    total += sample_rates[b] / 50;
  }
  // With another call of this pipeline in flight the uploads go on the copy stream (the noise stream, as pipe_api.inc) and run
  // under its kernels; with none, on the extractor's own stream.  Either way the host waits for them HERE: `pcm` is the
  // caller's again on return, and every kernel below is enqueued after its inputs have arrived.  (The noise stream also ends
  // the decode-side calls: on a context that decodes as well this wait covers decoder kernels that are on it -- see the header.)
  hipStream_t up = c->pl_begun[PL_ENCODE_STREAMS] != c->pl_ended[PL_ENCODE_STREAMS] ? c->sn : c->se[0];
  HIPCHK(c, hipMemcpyAsync(S.d_meta, h, n * 5 * 4, hipMemcpyHostToDevice, up));
  HIPCHK(c, hipMemcpyAsync(S.d_in, pcm, (size_t)total * 2, hipMemcpyHostToDevice, up));
  HIPCHK(c, hipStreamSynchronize(up));
  // empty packets, and the bytes behind a shorter one, read back as zeros; the extractor's stream is ahead of the quantizer's
  HIPCHK(c, hipMemsetAsync(S.d_pk, 0, (size_t)B * LYRA_HIP_MAX_PACKET_BYTES, c->se[0]));
  const int32_t* m = S.d_meta;
  if ((rc = lyra_hip_encode_streams_dev(c, m, B, S.d_in, total, m + 4 * n, m + n, m + 2 * n, dtx ? m + 3 * n : nullptr, S.d_pk,
                                        S.d_len)))
    return rc;
  // packets and lengths are written by the quantizer on sq[0] (the call is not split): their download rides on that stream
  HIPCHK(c, hipMemcpyAsync(S.h_out, S.d_pk, (size_t)B * LYRA_HIP_MAX_PACKET_BYTES, hipMemcpyDeviceToHost, c->sq[0]));
  HIPCHK(c, hipMemcpyAsync(S.h_out + (size_t)c->max_streams * 24, S.d_len, (size_t)B * 4, hipMemcpyDeviceToHost, c->sq[0]));
  HIPCHK(c, hipEventRecord(S.ev_done, c->sq[0]));
  S.B = B;
  c->pl_begun[PL_ENCODE_STREAMS]++;
  return 0;
}

int lyra_hip_encode_streams_end(lyra_hip_ctx* c, uint8_t* packets, int32_t* packet_bytes) {
  if (!c) return LYRA_HIP_EINVAL;
  if (!c->es_host || c->pl_ended[PL_ENCODE_STREAMS] == c->pl_begun[PL_ENCODE_STREAMS]) return fail(c, LYRA_HIP_EINVAL, "encode_streams_end: no call in flight");
  if (!packets || !packet_bytes) return fail(c, LYRA_HIP_EINVAL, "encode_streams_end: null pointer");
  DEVSCOPE(c);
  EsSlot& S = static_cast<EsHost*>(c->es_host)->slot[c->pl_ended[PL_ENCODE_STREAMS] & 1];
  c->pl_ended[PL_ENCODE_STREAMS]++;                   // whatever happens below, the slot is given back
  HIPCHK(c, hipEventSynchronize(S.ev_done));
  std::memcpy(packets, S.h_out, (size_t)S.B * LYRA_HIP_MAX_PACKET_BYTES);
  std::memcpy(packet_bytes, S.h_out + (size_t)c->max_streams * 24, (size_t)S.B * 4);
  return 0;
}

}  // extern "C"
