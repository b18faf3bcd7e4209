// decode_samples_any_api.inc -- part of api.hip: lyra_hip_decode_samples_any_dev (include/lyra_hip_decode_samples_any.h),
// LyraDecoder::SetEncodedPacket + DecodeSamples(n) for ANY n of 0..4 hops, BufferedResampler's leftover included
// (decode_samples_any_plan.h).  The call is lyra_hip_decode_samples_dev's launcher (ds_run, decode_samples_api.inc) run in R <= 4
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

Dsa* dsa_of(lyra_hip_ctx* c) { return &c->dsa; }   // the call buffers (lyra_hip_ctx::dsa, api.hip)
void dsa_free_call_buffers(Dsa* A) {
  dfree(A->d_ids, A->d_info, A->d_gan_new, A->d_call, A->d_pcm16);
  A->cap = 0;
}
void dsa_free(lyra_hip_ctx* c) { dsa_free_call_buffers(&c->dsa); }

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

// the round buffers of a call of parity `set`, for the any-size and the per-row call
void dsa_round_bufs(const Dsa* A, size_t set, DsCall* K) {
  K->cap = (size_t)A->cap;
  K->ids = A->d_ids + set * DSA_MAX_HOPS * 4 * K->cap;
  K->info = A->d_info + set * DSA_MAX_HOPS * 4 * K->cap;
  K->gan_new = A->d_gan_new + set * DSA_MAX_HOPS * 320 * K->cap;
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
  const size_t set = (size_t)(c->n_ds_calls & 1);
  const bool direct = ext == 16000;
  DsCall K = {d_ids, B, d_packets, d_pkt_bytes, R > 0 ? R : 1, R > 0, nullptr, nullptr, nullptr, 0,
              direct ? d_pcm_ext : A->d_pcm16, direct ? n_ext : DSA_MAX_INTERNAL, !direct && n_ext > 0, d_is_noise, d_is_cn};
  dsa_round_bufs(A, set, &K);
  int32_t* call = A->d_call + set * 4 * K.cap;
  return ds_run(
      c, K,
      [&](int r) {
        hipLaunchKernelGGL(ds_plan_any_kernel, dim3(cdiv(B, 256)), dim3(256), 0, c->sd[0], d_ids, B, r == 0 ? d_pkt_bytes : nullptr,
                           r, n_ext, ext, c->sm.base[st::R_RS_D], call, c->sm.base[st::R_CNG], K.ids_of(r, 0), K.ids_of(r, 1),
                           K.ids_of(r, 2), K.ids_of(r, 3), K.info_of(r), c->d_ds_feat, c->d_ds_ring, c->d_ds_err);
      },
      [&] {
        { ProfScope ps(c, K_RESAMPLE, c->sn);
          hipLaunchKernelGGL(ds_splice_kernel, dim3(cdiv(B, 4)), dim3(256), ds_splice_lds_bytes(), c->sn, P, d_ids, B,
                             (const int32_t*)call, c->sm.base[st::R_RS_D], (const int16_t*)A->d_pcm16, DSA_MAX_INTERNAL, d_pcm_ext,
                             n_ext); }
        HIPCHK(c, hipGetLastError());
        return 0;
      });
}

int dsa_check_size(lyra_hip_ctx* c, int num_samples, int sample_rate_hz) {
  int rc = check_rate(c, sample_rate_hz);
  if (rc) return rc;
  if (!ds_any_valid(num_samples, sample_rate_hz))
    return fail(c, LYRA_HIP_EINVAL, "decode_samples_any: %d samples at %d Hz: a request must be 0..%d samples (%d hops)", num_samples,
                sample_rate_hz, DSA_MAX_HOPS * (sample_rate_hz / 50), DSA_MAX_HOPS);
  return 0;
}

static_assert(host_staging::MAX_HOPS == lyra::DSA_MAX_HOPS, "the staging's rows are the call's");
const DsHostForm kDsaHostForm = {PL_DECODE_SAMPLES_ANY, "decode_samples_any", (size_t)DSA_MAX_HOPS, dsa_check_size,
                                 lyra_hip_decode_samples_any_dev};

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

// The same with HOST buffers, in two halves: the staging of lyra_hip_decode_samples_begin / _end with slots of its own.
int lyra_hip_decode_samples_any_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets,
                                      const int32_t* packet_bytes, int num_samples, int sample_rate_hz) {
  return ds_host_begin(c, kDsaHostForm, ids, B, packets, packet_bytes, num_samples, sample_rate_hz);
}

int lyra_hip_decode_samples_any_end(lyra_hip_ctx* c, int16_t* pcm) { return ds_host_end(c, kDsaHostForm, pcm); }

}  // extern "C"
