// decode_samples_api.inc -- part of api.hip: lyra_hip_decode_samples_dev, LyraDecoder::SetEncodedPacket (for the rows that
// got a packet) + DecodeSamples(n) for a request size that is not tied to the 20 ms hop (lyra_decoder.cc:172-373), with
// no host decision and no synchronisation.  The per-stream state is seven integers in the stream's comfort-noise slot
// (decode_samples_plan.h); the hop in progress of the generative model and of the comfort-noise generator and the feature
// vectors that wait for their hop live in arrays indexed by stream id.  One call is
//   decode stream: rvq_decode_mixed_kernel on the packet rows -> ds_plan_kernel (transition of both passes, id lists,
//                  info words, feature ring, features of the hops that start) -> the decoder chain on the rows that start a
//                  generative hop (TileCtx: id -1 writes no state, no output);
//   noise stream:  cng_kernel on the rows whose comfort-noise hop starts in pass 1 (estimate BEFORE the call's update, as
//                  in lyra_hip_decode_lossy_dev) -> ds_est_gather_kernel -> the decoder-side NoiseEstimator on the whole
//                  received hops that complete -> cng_kernel on the rows whose comfort-noise hop starts in pass 2 (estimate
//                  AFTER the update: RunComfortNoiseGenerator reads noise_estimate() when the hop starts) ->
//                  ds_slice_kernel -> the output resampler on n * 16000 / rate samples per row,
// the noise-stream half being ONE noise call.  For n = one hop the kernels that touch a sample are the lossy call's, in
// its order.
#include "decode_samples_plan.h"

static_assert(lyra::DS_FIFO_DEPTH == LYRA_HIP_DECODE_SAMPLES_FIFO, "documented depth of the feature FIFO");

namespace {

Bufs ds_stream_bufs(lyra_hip_ctx* c) {   // per stream of the context
  return {BUF(c->d_ds_ring, DS_FIFO_DEPTH * 64), BUF(c->d_ds_gan, 320), BUF(c->d_ds_cng, 320)};
}
Bufs ds_call_bufs(lyra_hip_ctx* c) {   // per frame of `ds_cap`
  return {BUF(c->d_ds_ids[0], 4), BUF(c->d_ds_info[0], 4), BUF(c->d_ds_gan_new[0], 320), BUF(c->d_ds_ids[1], 4),
          BUF(c->d_ds_info[1], 4), BUF(c->d_ds_gan_new[1], 320), BUF(c->d_ds_cng_new, 320), BUF(c->d_ds_est, 320),
          BUF(c->d_ds_pcm16, 320), BUF(c->d_ds_feat, 64)};
}
void ds_free_call_buffers(lyra_hip_ctx* c) {
  free_bufs(ds_call_bufs(c));
  c->ds_cap = 0;
}

// lyra_hip_decode_samples_begin / _end: two requests in flight, each with pinned staging for its arguments and a device
// row buffer for its result.
struct DsHostSlot {
  uint8_t* h_in = nullptr;     // pinned: ids [max_streams] | packet bytes [max_streams] | packets [max_streams][24]
  int32_t* d_ids = nullptr; int32_t* d_nb = nullptr; uint8_t* d_pk = nullptr;
  int16_t* d_out = nullptr;    // [max_streams][960]
  hipEvent_t ev_ready = nullptr;
  int B = 0, n = 0;
};
struct DsHost { DsHostSlot slot[2]; long begun = 0, ended = 0; };

void ds_free(lyra_hip_ctx* c) {
  if (DsHost* H = static_cast<DsHost*>(c->ds_host)) {
    for (DsHostSlot& S : H->slot) {
      if (S.h_in) (void)hipHostFree(S.h_in);
      void* ds[] = {S.d_ids, S.d_nb, S.d_pk, S.d_out};
      for (void* p : ds) if (p) (void)hipFree(p);
      if (S.ev_ready) (void)hipEventDestroy(S.ev_ready);
    }
    delete H;
    c->ds_host = nullptr;
  }
  ds_free_call_buffers(c);
  free_bufs(ds_stream_bufs(c));
  dfree(c->d_ds_err);
}

int ds_ensure_streams(lyra_hip_ctx* c) {   // (also what lyra_hip_import_streams needs before it writes a decoder side)
  // by stream id; contents only matter while a stream's counters say so: no reset needed.  Each pointer is tested on its
  // own (alloc_bufs), so a call after a failed allocation allocates only what is still missing.
  // One spare row behind the last stream's: an imported DsState whose fields are each in their domain but contradict each
  // other can make ds_slice_kernel read up to a hop past a held hop (stream_blob.h).
  return alloc_bufs(c, ds_stream_bufs(c), (size_t)c->max_streams + 1);
}

int ds_ensure(lyra_hip_ctx* c, int B) {
  int rc = ds_ensure_streams(c);
  if (!rc) rc = fade_ensure(c);
  if (rc) return rc;
  if (!c->d_ds_err) {
    unsigned* p = nullptr;
    HIPCHK(c, dalloc(&p, 1));
    if (hipMemset(p, 0, 4) != hipSuccess) {
      (void)hipFree(p);
      return fail(c, LYRA_HIP_EHIP, "decode_samples: clearing the error word failed");
    }
    c->d_ds_err = p;
  }
  if (B <= c->ds_cap) return 0;
  if ((rc = sync_all(c))) return rc;   // (the buffers of the calls in flight)
  ds_free_call_buffers(c);
  if ((rc = alloc_bufs(c, ds_call_bufs(c), (size_t)B))) return rc;
  c->ds_cap = B;
  return 0;
}

int ds_launch(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_packets, const int32_t* d_pkt_bytes, int n_ext,
              int n_int, int ext, int16_t* d_pcm_ext, int32_t* d_is_noise, int32_t* d_is_cn) {
  DEVSCOPE(c);
  int rc = ensure_scratch(c, B);
  if (rc) return rc;
  if ((rc = ds_ensure(c, B))) return rc;
  const int set = (int)(c->n_ds_calls & 1);
  const size_t cap = (size_t)c->ds_cap;
  int32_t* gen_ids = c->d_ds_ids[set];
  int32_t* cng1_ids = gen_ids + cap;
  int32_t* cng2_ids = gen_ids + 2 * cap;
  int32_t* est_ids = gen_ids + 3 * cap;
  int32_t* info = c->d_ds_info[set];
  int16_t* gan_new = c->d_ds_gan_new[set];
  // ---- decode stream: one unsplit decode-side call (on split contexts it stands for every chunk, dec_side_done) ----
  if ((rc = dec_side_begin(c, 0, 1))) return rc;
  { ProfScope ps(c, K_RVQ_DEC, c->sd[0]);
    hipLaunchKernelGGL(rvq_decode_mixed_kernel, dim3(cdiv(B, 4)), dim3(256), 0, c->sd[0], c->model.cb, d_packets, d_pkt_bytes, 0, B,
                       c->d_ds_feat); }
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(ds_plan_kernel, dim3(cdiv(B, 256)), dim3(256), 0, c->sd[0], d_ids, B, d_pkt_bytes, n_int,
                     c->sm.base[st::R_CNG], gen_ids, cng1_ids, cng2_ids, est_ids, info, c->d_ds_feat, c->d_ds_ring, c->d_ds_err);
  HIPCHK(c, hipGetLastError());
  // (n == 0 is SetEncodedPacket alone: no pass, so no hop starts)
  if (n_int > 0 && (rc = launch_generate(c, 0, 0, gen_ids, B, c->d_ds_feat, gan_new))) return rc;
  if ((rc = dec_side_done(c, 0, 1))) return rc;
  c->n_dec_calls++;
  // ---- noise stream: comfort noise, estimator, comfort noise, slices, resampler as ONE noise call ---------------------
  if ((rc = noise_dev_begin(c))) return rc;
  if (n_int > 0) {
    if ((rc = launch_cng(c, c->sn, cng1_ids, B, nullptr, c->d_ds_cng_new))) return rc;
    hipLaunchKernelGGL(ds_est_gather_kernel, dim3(cdiv(B, 4)), dim3(256), 0, c->sn, d_ids, B, (const int32_t*)info,
                       (const int16_t*)gan_new, (const int16_t*)c->d_ds_gan, c->d_ds_est);
    HIPCHK(c, hipGetLastError());
    if ((rc = launch_noise_masked(c, est_ids, B, c->d_ds_est, d_is_noise))) return rc;   // the rows whose received hop completes
    if ((rc = launch_cng(c, c->sn, cng2_ids, B, nullptr, c->d_ds_cng_new))) return rc;
  }
  int16_t* out16 = ext == 16000 ? d_pcm_ext : c->d_ds_pcm16;
  hipLaunchKernelGGL(ds_slice_kernel, dim3(cdiv(B, 4)), dim3(256), 0, c->sn, d_ids, B, (const int32_t*)info,
                     (const int16_t*)gan_new, (const int16_t*)c->d_ds_cng_new, c->d_ds_gan, c->d_ds_cng,
                     (const float*)c->d_fade, out16, ext == 16000 ? n_ext : 320, (const uint8_t*)c->sm.base[st::R_NOISE_D],
                     d_is_noise, d_is_cn);
  HIPCHK(c, hipGetLastError());
  if (ext != 16000 && n_int > 0) {
    if ((rc = launch_resample(c, 1, d_ids, B, c->d_ds_pcm16, n_int, 16000, ext, d_pcm_ext, nullptr, 320, n_ext, c->sn))) return rc;
    c->rs_sn_pending = true;
  }
  if ((rc = noise_dev_done(c))) return rc;
  c->n_ds_calls++;
  return serial_noise_half_done(c);
}

}  // namespace

extern "C" {

int lyra_hip_decode_samples_dev(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_packets,
                                const int32_t* d_packet_bytes, int num_samples, int sample_rate_hz, int16_t* d_pcm_ext,
                                int32_t* d_is_noise, int32_t* d_is_comfort_noise) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if ((rc = check_rate(c, sample_rate_hz))) return rc;
  const int n_int = ds_internal_samples(num_samples, sample_rate_hz);
  if (n_int < 0)
    return fail(c, LYRA_HIP_EINVAL, "decode_samples: %d samples at %d Hz: a request must be 0..%d samples and a whole number of "
                "16 kHz samples (other sizes: BatchLyraDecoder)", num_samples, sample_rate_hz, sample_rate_hz / 50);
  if (!d_ids || !d_packets || !d_packet_bytes || (num_samples > 0 && !d_pcm_ext))
    return fail(c, LYRA_HIP_EINVAL, "decode_samples: null pointer");
  return ds_launch(c, d_ids, B, d_packets, d_packet_bytes, num_samples, n_int, sample_rate_hz, d_pcm_ext, d_is_noise,
                   d_is_comfort_noise);
}

long lyra_hip_decode_samples_errors(lyra_hip_ctx* c, int clear) {
  return read_error_counter(c, &lyra_hip_ctx::d_ds_err, clear);
}

// The same with HOST buffers, in two halves (the form of lyra_hip_decode_begin / _end): begin() copies ids, sizes and packets
// into pinned staging, uploads them on the decode-side stream and enqueues lyra_hip_decode_samples_dev into the slot's row
// buffer; end() downloads the OLDEST begun request straight into the caller's memory -- on the (idle) quantizer stream
// while a younger request's kernels run, on the noise stream itself when there is none -- and synchronises that stream only.
int lyra_hip_decode_samples_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets,
                                  const int32_t* packet_bytes, int num_samples, int sample_rate_hz) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if ((rc = check_rate(c, sample_rate_hz))) return rc;
  if (ds_internal_samples(num_samples, sample_rate_hz) < 0)
    return fail(c, LYRA_HIP_EINVAL, "decode_samples: %d samples at %d Hz: a request must be 0..%d samples and a whole number of "
                "16 kHz samples (other sizes: BatchLyraDecoder)", num_samples, sample_rate_hz, sample_rate_hz / 50);
  if (!packets || !packet_bytes) return fail(c, LYRA_HIP_EINVAL, "decode_samples_begin: null pointer");
  if ((rc = check_ids_host(c, ids, B))) return rc;
  DEVSCOPE(c);
  if (!c->ds_host) c->ds_host = new DsHost();
  DsHost* H = static_cast<DsHost*>(c->ds_host);
  if (H->begun - H->ended >= 2)
    return fail(c, LYRA_HIP_EINVAL, "decode_samples_begin: two requests are already in flight (lyra_hip_decode_samples_end)");
  if (c->brg_begun != c->brg_ended)   // (the bridge runs on both sides' streams)
    return fail(c, LYRA_HIP_EINVAL, "decode_samples_begin: a lyra_hip_bridge_begin tick is in flight (lyra_hip_bridge_end)");
  if (c->dstr_begun != c->dstr_ended)   // (as lyra_hip_decode_begin: one decode pipeline at a time)
    return fail(c, LYRA_HIP_EINVAL, "decode_samples_begin: a lyra_hip_decode_streams_begin call is in flight "
                "(lyra_hip_decode_streams_end)");
  if (c->dsa_begun != c->dsa_ended)
    return fail(c, LYRA_HIP_EINVAL, "decode_samples_begin: a lyra_hip_decode_samples_any_begin request is in flight "
                "(lyra_hip_decode_samples_any_end)");
  if (c->dss_begun != c->dss_ended)
    return fail(c, LYRA_HIP_EINVAL, "decode_samples_begin: a lyra_hip_decode_samples_streams_begin request is in flight "
                "(lyra_hip_decode_samples_streams_end)");
  DsHostSlot& S = H->slot[H->begun & 1];
  const size_t n = (size_t)c->max_streams;
  if (!S.h_in) HIPCHK(c, hipHostMalloc((void**)&S.h_in, n * 32, hipHostMallocDefault));
  if (!S.d_ids) HIPCHK(c, dalloc(&S.d_ids, n));
  if (!S.d_nb) HIPCHK(c, dalloc(&S.d_nb, n));
  if (!S.d_pk) HIPCHK(c, dalloc(&S.d_pk, n * 24));
  if (!S.d_out) HIPCHK(c, dalloc(&S.d_out, n * 960));
  if (!S.ev_ready) HIPCHK(c, hipEventCreateWithFlags(&S.ev_ready, hipEventDisableTiming));
  // (the slot's previous user, two requests back, has ended: its kernels on both streams have read these buffers)
  std::memcpy(S.h_in, ids, (size_t)B * 4);
  std::memcpy(S.h_in + n * 4, packet_bytes, (size_t)B * 4);
  std::memcpy(S.h_in + n * 8, packets, (size_t)B * LYRA_HIP_MAX_PACKET_BYTES);
  HIPCHK(c, hipMemcpyAsync(S.d_ids, S.h_in, (size_t)B * 4, hipMemcpyHostToDevice, c->sd[0]));
  HIPCHK(c, hipMemcpyAsync(S.d_nb, S.h_in + n * 4, (size_t)B * 4, hipMemcpyHostToDevice, c->sd[0]));
  HIPCHK(c, hipMemcpyAsync(S.d_pk, S.h_in + n * 8, (size_t)B * LYRA_HIP_MAX_PACKET_BYTES, hipMemcpyHostToDevice, c->sd[0]));
  if ((rc = lyra_hip_decode_samples_dev(c, S.d_ids, B, S.d_pk, S.d_nb, num_samples, sample_rate_hz, S.d_out, nullptr, nullptr)))
    return rc;
  HIPCHK(c, hipEventRecord(S.ev_ready, c->sn));
  S.B = B;
  S.n = num_samples;
  H->begun++;
  return 0;
}

int lyra_hip_decode_samples_end(lyra_hip_ctx* c, int16_t* pcm) {
  if (!c) return LYRA_HIP_EINVAL;
  DsHost* H = static_cast<DsHost*>(c->ds_host);
  if (!H || H->ended == H->begun) return fail(c, LYRA_HIP_EINVAL, "decode_samples_end: no request in flight");
  DsHostSlot& S = H->slot[H->ended & 1];
  if (S.n > 0 && !pcm) return fail(c, LYRA_HIP_EINVAL, "null pointer");
  DEVSCOPE(c);
  H->ended++;
  if (S.n == 0) {
    HIPCHK(c, hipEventSynchronize(S.ev_ready));
    return 0;
  }
  const bool overlap = H->ended != H->begun;
  hipStream_t down = overlap ? c->sq[0] : c->sn;
  if (overlap) HIPCHK(c, hipStreamWaitEvent(down, S.ev_ready, 0));
  HIPCHK(c, hipMemcpyAsync(pcm, S.d_out, (size_t)S.B * (size_t)S.n * 2, hipMemcpyDeviceToHost, down));
  HIPCHK(c, hipStreamSynchronize(down));
  return 0;
}

}  // extern "C"
