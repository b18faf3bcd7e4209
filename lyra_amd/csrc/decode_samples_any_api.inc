// decode_samples_any_api.inc -- part of api.hip: lyra_hip_decode_samples_any_dev (include/lyra_hip_decode_samples_any.h),
// LyraDecoder::SetEncodedPacket + DecodeSamples(n) for ANY n of 0..4 hops, BufferedResampler's leftover included
// (decode_samples_any_plan.h).  The call is lyra_hip_decode_samples_dev's machinery (decode_samples_api.inc) run in R <= 4
// ROUNDS of at most one hop, with the internal length per row:
//   decode stream: rvq_decode_mixed_kernel -> per round r: ds_plan_any_kernel (round 0 derives each row's n_int from its leftover
//                  count, advances the count and delivers the packet) -> the decoder chain on the rows that start a hop;
//   noise stream:  per round r: comfort noise (pass 1) -> estimator input -> estimator -> comfort noise (pass 2) ->
//                  ds_slice_kernel at internal offset 320 r of the row; then, at 8 / 32 / 48 kHz, ds_splice_kernel: resampler
//                  over n_int[b] samples, old leftover + new samples to the caller's row, surplus to the slot,
// one decode-side call and one noise call.  Both streams run their rounds in order, so the estimator update of round r is
// seen by the comfort-noise hop of its pass 2 and by everything in round r + 1.  What a round's decode-stream half hands its
// noise-stream half -- id lists, info words, the hops that started -- is buffered PER ROUND (and by call parity, as the
// one-hop call's), so the decode stream never waits for the noise stream inside a call; the per-row call words {old leftover
// count, used, n_int, new count} are buffered by call parity.  A row whose rounds are over plans 0 samples: a no-op.
#include "decode_samples_any_plan.h"
#include "../../include/lyra_hip_decode_samples_any.h"

static_assert(lyra::DSA_MAX_HOPS == LYRA_HIP_DECODE_SAMPLES_MAX_HOPS, "documented number of hops per request");

namespace {

struct DsaHostSlot {
  uint8_t* h_in = nullptr;     // pinned: ids [max_streams] | packet bytes [max_streams] | packets [max_streams][24]
  int32_t* d_ids = nullptr; int32_t* d_nb = nullptr; uint8_t* d_pk = nullptr;
  int16_t* d_out = nullptr;    // [max_streams][4 * 960]
  hipEvent_t ev_ready = nullptr;
  int B = 0, n = 0;
};
struct Dsa {
  int cap = 0;                       // rows the call buffers hold; set once all of them exist
  int32_t* d_ids = nullptr;          // [2 call parities][4 rounds][4 lists][cap]
  int32_t* d_info = nullptr;         // [2][4][cap][4]
  int16_t* d_gan_new = nullptr;      // [2][4][cap][320]
  int32_t* d_call = nullptr;         // [2][cap][4]
  int16_t* d_pcm16 = nullptr;        // [cap][1280] internal-rate output in front of the resampler (noise stream only)
  DsaHostSlot slot[2];
};

Dsa* dsa_of(lyra_hip_ctx* c) {
  if (!c->dsa) c->dsa = new Dsa();
  return static_cast<Dsa*>(c->dsa);
}
void dsa_free_call_buffers(Dsa* A) {
  dfree(A->d_ids, A->d_info, A->d_gan_new, A->d_call, A->d_pcm16);
  A->cap = 0;
}
void dsa_free(lyra_hip_ctx* c) {
  Dsa* A = static_cast<Dsa*>(c->dsa);
  if (!A) return;
  for (DsaHostSlot& S : A->slot) {
    if (S.h_in) (void)hipHostFree(S.h_in);
    dfree(S.d_ids, S.d_nb, S.d_pk, S.d_out);
    if (S.ev_ready) (void)hipEventDestroy(S.ev_ready);
  }
  dsa_free_call_buffers(A);
  delete A;
  c->dsa = nullptr;
}

int dsa_ensure(lyra_hip_ctx* c, int B) {
  Dsa* A = dsa_of(c);
  if (B <= A->cap) return 0;
  int rc = sync_all(c);   // (the buffers of the calls in flight)
  if (rc) return rc;
  dsa_free_call_buffers(A);
  const size_t n = (size_t)B;
  HIPCHK(c, dalloc(&A->d_ids, 2 * DSA_MAX_HOPS * 4 * n));
  HIPCHK(c, dalloc(&A->d_info, 2 * DSA_MAX_HOPS * 4 * n));
  HIPCHK(c, dalloc(&A->d_gan_new, 2 * DSA_MAX_HOPS * 320 * n));
  HIPCHK(c, dalloc(&A->d_call, 2 * 4 * n));
  HIPCHK(c, dalloc(&A->d_pcm16, (size_t)DSA_MAX_INTERNAL * n));
  A->cap = B;   // (only now: a failed allocation above leaves cap 0, and the next call frees what exists and starts over)
  return 0;
}

int dsa_launch(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_packets, const int32_t* d_pkt_bytes, int n_ext,
               int ext, int16_t* d_pcm_ext, int32_t* d_is_noise, int32_t* d_is_cn) {
  DEVSCOPE(c);
  int rc = ensure_scratch(c, B);
  if (rc) return rc;
  if ((rc = ds_ensure(c, B))) return rc;   // the streams' rings and held hops, the error word, the rows both calls share
  if ((rc = dsa_ensure(c, B))) return rc;
  ResampleP P;
  if (ext != 16000 && !resample_design(16000, ext, &P)) return fail(c, LYRA_HIP_EINVAL, "decode_samples_any: no resampler design");
  Dsa* A = dsa_of(c);
  const int R = ds_any_rounds(n_ext, ext);
  const size_t cap = (size_t)A->cap, set = (size_t)(c->n_ds_calls & 1);
  auto ids_of = [&](int r, int list) { return A->d_ids + ((set * DSA_MAX_HOPS + r) * 4 + list) * cap; };
  auto info_of = [&](int r) { return A->d_info + (set * DSA_MAX_HOPS + r) * 4 * cap; };
  auto gan_of = [&](int r) { return A->d_gan_new + (set * DSA_MAX_HOPS + r) * 320 * cap; };
  int32_t* call = A->d_call + set * 4 * cap;
  // ---- decode stream: one unsplit decode-side call ---------------------------------------------------------------------
  if ((rc = dec_side_begin(c, 0, 1))) return rc;
  { ProfScope ps(c, K_RVQ_DEC, c->sd[0]);
    hipLaunchKernelGGL(rvq_decode_mixed_kernel, dim3(cdiv(B, 4)), dim3(256), 0, c->sd[0], c->model.cb, d_packets, d_pkt_bytes, 0, B,
                       c->d_ds_feat); }
  HIPCHK(c, hipGetLastError());
  for (int r = 0; r < (R > 0 ? R : 1); ++r) {   // (n == 0 is SetEncodedPacket alone: one plan, no pass, no hop)
    hipLaunchKernelGGL(ds_plan_any_kernel, dim3(cdiv(B, 256)), dim3(256), 0, c->sd[0], d_ids, B, r == 0 ? d_pkt_bytes : nullptr, r,
                       n_ext, ext, c->sm.base[st::R_RS_D], call, c->sm.base[st::R_CNG], ids_of(r, 0), ids_of(r, 1), ids_of(r, 2),
                       ids_of(r, 3), info_of(r), c->d_ds_feat, c->d_ds_ring, c->d_ds_err);
    HIPCHK(c, hipGetLastError());
    if (R > 0 && (rc = launch_generate(c, 0, 0, ids_of(r, 0), B, c->d_ds_feat, gan_of(r)))) return rc;
  }
  if ((rc = dec_side_done(c, 0, 1))) return rc;
  c->n_dec_calls++;
  // ---- noise stream: the rounds' comfort noise, estimator, comfort noise, slices; then the splice, as ONE noise call ------
  if ((rc = noise_dev_begin(c))) return rc;
  for (int r = 0; r < (R > 0 ? R : 1); ++r) {
    const int32_t* info = info_of(r);
    const int16_t* gan_new = gan_of(r);
    if (R > 0) {
      if ((rc = launch_cng(c, c->sn, ids_of(r, 1), B, nullptr, c->d_ds_cng_new))) return rc;
      hipLaunchKernelGGL(ds_est_gather_kernel, dim3(cdiv(B, 4)), dim3(256), 0, c->sn, d_ids, B, info, gan_new,
                         (const int16_t*)c->d_ds_gan, c->d_ds_est);
      HIPCHK(c, hipGetLastError());
      if ((rc = launch_noise_masked(c, ids_of(r, 3), B, c->d_ds_est, d_is_noise))) return rc;
      if ((rc = launch_cng(c, c->sn, ids_of(r, 2), B, nullptr, c->d_ds_cng_new))) return rc;
    }
    int16_t* out16 = ext == 16000 ? d_pcm_ext + 320 * r : A->d_pcm16 + 320 * r;
    hipLaunchKernelGGL(ds_slice_kernel, dim3(cdiv(B, 4)), dim3(256), 0, c->sn, d_ids, B, info, gan_new,
                       (const int16_t*)c->d_ds_cng_new, c->d_ds_gan, c->d_ds_cng, (const float*)c->d_fade, out16,
                       ext == 16000 ? n_ext : DSA_MAX_INTERNAL, (const uint8_t*)c->sm.base[st::R_NOISE_D], d_is_noise, d_is_cn);
    HIPCHK(c, hipGetLastError());
  }
  if (ext != 16000 && n_ext > 0) {
    { ProfScope ps(c, K_RESAMPLE, c->sn);
      hipLaunchKernelGGL(ds_splice_kernel, dim3(cdiv(B, 4)), dim3(256), ds_splice_lds_bytes(), c->sn, P, d_ids, B,
                         (const int32_t*)call, c->sm.base[st::R_RS_D], (const int16_t*)A->d_pcm16, DSA_MAX_INTERNAL, d_pcm_ext,
                         n_ext); }
    HIPCHK(c, hipGetLastError());
    c->rs_sn_pending = true;
  }
  if ((rc = noise_dev_done(c))) return rc;
  c->n_ds_calls++;
  return serial_noise_half_done(c);
}

int dsa_check_size(lyra_hip_ctx* c, int num_samples, int sample_rate_hz) {
  int rc = check_rate(c, sample_rate_hz);
  if (rc) return rc;
  if (!ds_any_valid(num_samples, sample_rate_hz))
    return fail(c, LYRA_HIP_EINVAL, "decode_samples_any: %d samples at %d Hz: a request must be 0..%d samples (%d hops)", num_samples,
                sample_rate_hz, DSA_MAX_HOPS * (sample_rate_hz / 50), DSA_MAX_HOPS);
  return 0;
}

}  // namespace

extern "C" {

int lyra_hip_decode_samples_any_dev(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_packets,
                                    const int32_t* d_packet_bytes, int num_samples, int sample_rate_hz, int16_t* d_pcm_ext,
                                    int32_t* d_is_noise, int32_t* d_is_comfort_noise) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if ((rc = dsa_check_size(c, num_samples, sample_rate_hz))) return rc;
  if (!d_ids || !d_packets || !d_packet_bytes || (num_samples > 0 && !d_pcm_ext))
    return fail(c, LYRA_HIP_EINVAL, "decode_samples_any: null pointer");
  return dsa_launch(c, d_ids, B, d_packets, d_packet_bytes, num_samples, sample_rate_hz, d_pcm_ext, d_is_noise,
                    d_is_comfort_noise);
}

// The same with HOST buffers, in two halves: lyra_hip_decode_samples_begin / _end with staging and row buffers of its own.
int lyra_hip_decode_samples_any_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets,
                                      const int32_t* packet_bytes, int num_samples, int sample_rate_hz) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if ((rc = dsa_check_size(c, num_samples, sample_rate_hz))) return rc;
  if (!packets || !packet_bytes) return fail(c, LYRA_HIP_EINVAL, "decode_samples_any_begin: null pointer");
  if ((rc = check_ids_host(c, ids, B))) return rc;
  DEVSCOPE(c);
  if (c->dsa_begun - c->dsa_ended >= 2)
    return fail(c, LYRA_HIP_EINVAL, "decode_samples_any_begin: two requests are already in flight (lyra_hip_decode_samples_any_end)");
  if (c->brg_begun != c->brg_ended)   // (the bridge runs on both sides' streams)
    return fail(c, LYRA_HIP_EINVAL, "decode_samples_any_begin: a lyra_hip_bridge_begin tick is in flight (lyra_hip_bridge_end)");
  { const PipeState* P = pipe_of(c);   // (one decode pipeline at a time: they share the decode-side streams' order)
    const DsHost* H = static_cast<const DsHost*>(c->ds_host);
    if ((P && P->d_begun != P->d_ended) || (H && H->begun != H->ended) || c->dstr_begun != c->dstr_ended)
      return fail(c, LYRA_HIP_EINVAL, "decode_samples_any_begin: a lyra_hip_decode_begin, lyra_hip_decode_streams_begin or "
                  "lyra_hip_decode_samples_begin request is in flight (call its _end first)");
    if (c->dss_begun != c->dss_ended)
      return fail(c, LYRA_HIP_EINVAL, "decode_samples_any_begin: a lyra_hip_decode_samples_streams_begin request is in flight "
                  "(lyra_hip_decode_samples_streams_end)"); }
  DsaHostSlot& S = dsa_of(c)->slot[c->dsa_begun & 1];
  const size_t n = (size_t)c->max_streams;
  if (!S.h_in) HIPCHK(c, hipHostMalloc((void**)&S.h_in, n * 32, hipHostMallocDefault));
  if (!S.d_ids) HIPCHK(c, dalloc(&S.d_ids, n));
  if (!S.d_nb) HIPCHK(c, dalloc(&S.d_nb, n));
  if (!S.d_pk) HIPCHK(c, dalloc(&S.d_pk, n * 24));
  if (!S.d_out) HIPCHK(c, dalloc(&S.d_out, n * DSA_MAX_HOPS * 960));
  if (!S.ev_ready) HIPCHK(c, hipEventCreateWithFlags(&S.ev_ready, hipEventDisableTiming));
  // (the slot's previous user, two requests back, has ended: its kernels on both streams have read these buffers)
  std::memcpy(S.h_in, ids, (size_t)B * 4);
  std::memcpy(S.h_in + n * 4, packet_bytes, (size_t)B * 4);
  std::memcpy(S.h_in + n * 8, packets, (size_t)B * LYRA_HIP_MAX_PACKET_BYTES);
  HIPCHK(c, hipMemcpyAsync(S.d_ids, S.h_in, (size_t)B * 4, hipMemcpyHostToDevice, c->sd[0]));
  HIPCHK(c, hipMemcpyAsync(S.d_nb, S.h_in + n * 4, (size_t)B * 4, hipMemcpyHostToDevice, c->sd[0]));
  HIPCHK(c, hipMemcpyAsync(S.d_pk, S.h_in + n * 8, (size_t)B * LYRA_HIP_MAX_PACKET_BYTES, hipMemcpyHostToDevice, c->sd[0]));
  if ((rc = dsa_launch(c, S.d_ids, B, S.d_pk, S.d_nb, num_samples, sample_rate_hz, S.d_out, nullptr, nullptr))) return rc;
  HIPCHK(c, hipEventRecord(S.ev_ready, c->sn));
  S.B = B;
  S.n = num_samples;
  c->dsa_begun++;
  return 0;
}

int lyra_hip_decode_samples_any_end(lyra_hip_ctx* c, int16_t* pcm) {
  if (!c) return LYRA_HIP_EINVAL;
  if (!c->dsa || c->dsa_ended == c->dsa_begun) return fail(c, LYRA_HIP_EINVAL, "decode_samples_any_end: no request in flight");
  DsaHostSlot& S = dsa_of(c)->slot[c->dsa_ended & 1];
  if (S.n > 0 && !pcm) return fail(c, LYRA_HIP_EINVAL, "decode_samples_any_end: null pointer");
  DEVSCOPE(c);
  c->dsa_ended++;
  if (S.n == 0) {
    HIPCHK(c, hipEventSynchronize(S.ev_ready));
    return 0;
  }
  const bool overlap = c->dsa_ended != c->dsa_begun;
  hipStream_t down = overlap ? c->sq[0] : c->sn;
  if (overlap) HIPCHK(c, hipStreamWaitEvent(down, S.ev_ready, 0));
  HIPCHK(c, hipMemcpyAsync(pcm, S.d_out, (size_t)S.B * (size_t)S.n * 2, hipMemcpyDeviceToHost, down));
  HIPCHK(c, hipStreamSynchronize(down));
  return 0;
}

}  // extern "C"
