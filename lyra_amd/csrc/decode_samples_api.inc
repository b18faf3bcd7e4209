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
// This file also holds what the three DecodeSamples calls share on the host: ds_run, the one launcher (a DsCall says in what
// lyra_hip_decode_samples_dev, _any_dev and _streams_dev differ), and ds_host_begin / ds_host_end, the staging of the two
// uniform host forms.  The kernels' shared bodies are in decode_samples_rows.h.
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

void ds_free(lyra_hip_ctx* c) {
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
  if ((rc = err_word_ensure(c, &c->d_ds_err))) return rc;
  if (B <= c->ds_cap) return 0;
  if ((rc = sync_all(c))) return rc;   // (the buffers of the calls in flight)
  ds_free_call_buffers(c);
  if ((rc = alloc_bufs(c, ds_call_bufs(c), (size_t)B))) return rc;
  c->ds_cap = B;
  return 0;
}

// One DecodeSamples call, whichever of the three: everything in which lyra_hip_decode_samples_dev, _any_dev and _streams_dev
// differ, apart from the launch of a round's plan kernel and of the kernel that ends the call (ds_run's two arguments).
struct DsCall {
  const int32_t* d_ids; int B; const uint8_t* d_packets; const int32_t* d_pkt_bytes;
  int rounds;                  // plan rounds, of one hop at most each
  bool hops;                   // false: SetEncodedPacket alone (a uniform request of 0 samples): one plan and one slice, no hop starts
  // what a round's decode-stream half hands its noise-stream half, of this call's parity: the one-hop call's single-round
  // buffers in the context, or Dsa's (decode_samples_any_api.inc)
  int32_t* ids;                // [rounds][4 lists][cap]
  int32_t* info;               // [rounds][cap][4]
  int16_t* gan_new;            // [rounds][cap][320]
  size_t cap;
  int16_t* out16; int out_stride;   // ds_slice_kernel's rows: round r writes at out16 + 320 r
  bool tail;                   // the call ends in the resampler or a splice kernel, on the noise stream
  int32_t* d_is_noise; int32_t* d_is_cn;
  int32_t* ids_of(int r, int list) const { return ids + ((size_t)r * 4 + list) * cap; }
  int32_t* info_of(int r) const { return info + (size_t)r * 4 * cap; }
  int16_t* gan_of(int r) const { return gan_new + (size_t)r * 320 * cap; }
};

// The call: one unsplit decode-side call and ONE noise call.  plan(r) launches round r's plan kernel on sd[0]; tail() launches
// what ends the call on sn and returns a code.  The caller has allocated everything.
template <class Plan, class Tail>
int ds_run(lyra_hip_ctx* c, const DsCall& K, Plan plan, Tail tail) {
  const int B = K.B;
  // ---- decode stream: one unsplit decode-side call (on split contexts it stands for every chunk, dec_side_done) ----
  int rc = dec_side_begin(c, 0, 1);
  if (rc) return rc;
  { ProfScope ps(c, K_RVQ_DEC, c->sd[0]);
    hipLaunchKernelGGL(rvq_decode_mixed_kernel, dim3(cdiv(B, 4)), dim3(256), 0, c->sd[0], c->model.cb, K.d_packets, K.d_pkt_bytes, 0,
                       B, c->d_ds_feat); }
  HIPCHK(c, hipGetLastError());
  for (int r = 0; r < K.rounds; ++r) {
    plan(r);
    HIPCHK(c, hipGetLastError());
    if (K.hops && (rc = launch_generate(c, 0, 0, K.ids_of(r, 0), B, c->d_ds_feat, K.gan_of(r)))) return rc;
  }
  if ((rc = dec_side_done(c, 0, 1))) return rc;
  c->n_dec_calls++;
  // ---- noise stream: per round comfort noise, estimator, comfort noise, slices; then the tail, as ONE noise call ----
  if ((rc = noise_dev_begin(c))) return rc;
  for (int r = 0; r < K.rounds; ++r) {
    const int32_t* info = K.info_of(r);
    const int16_t* gan_new = K.gan_of(r);
    if (K.hops) {
      if ((rc = launch_cng(c, c->sn, K.ids_of(r, 1), B, nullptr, c->d_ds_cng_new))) return rc;
      hipLaunchKernelGGL(ds_est_gather_kernel, dim3(cdiv(B, 4)), dim3(256), 0, c->sn, K.d_ids, B, info, gan_new,
                         (const int16_t*)c->d_ds_gan, c->d_ds_est);
      HIPCHK(c, hipGetLastError());
      if ((rc = launch_noise_masked(c, K.ids_of(r, 3), B, c->d_ds_est, K.d_is_noise))) return rc;   // the rows whose received hop completes
      if ((rc = launch_cng(c, c->sn, K.ids_of(r, 2), B, nullptr, c->d_ds_cng_new))) return rc;
    }
    hipLaunchKernelGGL(ds_slice_kernel, dim3(cdiv(B, 4)), dim3(256), 0, c->sn, K.d_ids, B, info, gan_new,
                       (const int16_t*)c->d_ds_cng_new, c->d_ds_gan, c->d_ds_cng, (const float*)c->d_fade, K.out16 + 320 * r,
                       K.out_stride, (const uint8_t*)c->sm.base[st::R_NOISE_D], K.d_is_noise, K.d_is_cn);
    HIPCHK(c, hipGetLastError());
  }
  if (K.tail) {
    if ((rc = tail())) return rc;
    c->rs_sn_pending = true;
  }
  if ((rc = noise_dev_done(c))) return rc;
  c->n_ds_calls++;
  return serial_noise_half_done(c);
}

int ds_launch(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_packets, const int32_t* d_pkt_bytes, int n_ext,
              int n_int, int ext, int16_t* d_pcm_ext, int32_t* d_is_noise, int32_t* d_is_cn) {
  DEVSCOPE(c);
  int rc = ensure_scratch(c, B);
  if (rc) return rc;
  if ((rc = ds_ensure(c, B))) return rc;
  const int set = (int)(c->n_ds_calls & 1);
  const bool direct = ext == 16000;   // (n == 0 is SetEncodedPacket alone: no pass, so no hop starts)
  const DsCall K = {d_ids, B, d_packets, d_pkt_bytes, 1, n_int > 0, c->d_ds_ids[set], c->d_ds_info[set], c->d_ds_gan_new[set],
                    (size_t)c->ds_cap, direct ? d_pcm_ext : c->d_ds_pcm16, direct ? n_ext : 320, !direct && n_int > 0, d_is_noise,
                    d_is_cn};
  return ds_run(
      c, K,
      [&](int) {
        hipLaunchKernelGGL(ds_plan_kernel, dim3(cdiv(B, 256)), dim3(256), 0, c->sd[0], d_ids, B, d_pkt_bytes, n_int,
                           c->sm.base[st::R_CNG], K.ids_of(0, 0), K.ids_of(0, 1), K.ids_of(0, 2), K.ids_of(0, 3), K.info,
                           c->d_ds_feat, c->d_ds_ring, c->d_ds_err);
      },
      [&] { return launch_resample(c, 1, d_ids, B, c->d_ds_pcm16, n_int, 16000, ext, d_pcm_ext, nullptr, 320, n_ext, c->sn); });
}

int ds_check_size(lyra_hip_ctx* c, int num_samples, int sample_rate_hz) {
  int rc = check_rate(c, sample_rate_hz);
  if (rc) return rc;
  if (ds_internal_samples(num_samples, sample_rate_hz) < 0)
    return fail(c, LYRA_HIP_EINVAL, "decode_samples: %d samples at %d Hz: a request must be 0..%d samples and a whole number of "
                "16 kHz samples (other sizes: BatchLyraDecoder)", num_samples, sample_rate_hz, sample_rate_hz / 50);
  return 0;
}

// The two uniform calls with HOST buffers, in two halves (the form of lyra_hip_decode_begin / _end): begin() copies ids, sizes
// and packets into pinned staging, uploads them on the decode-side stream and enqueues the `_dev` call into the slot's row
// buffer; end() downloads the OLDEST begun request straight into the caller's memory -- on the (idle) quantizer stream
// while a younger request's kernels run, on the noise stream itself when there is none -- and synchronises that stream only.
// A request's slot: pinned staging for its arguments and a device row buffer for its result (host_staging::decode_samples).
struct DsHostForm {
  Pipeline pl;
  const char* who;
  size_t hops;                                         // hops of 960 samples per stream in a slot's row buffer
  int (*check_size)(lyra_hip_ctx*, int num_samples, int sample_rate_hz);
  int (*dev)(lyra_hip_ctx*, const int32_t*, int, const uint8_t*, const int32_t*, int, int, int16_t*, int32_t*, int32_t*);
};

int ds_host_begin(lyra_hip_ctx* c, const DsHostForm& F, const int32_t* ids, int B, const uint8_t* packets,
                  const int32_t* packet_bytes, int num_samples, int sample_rate_hz) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if ((rc = F.check_size(c, num_samples, sample_rate_hz))) return rc;
  if (!packets || !packet_bytes) return fail(c, LYRA_HIP_EINVAL, "%s_begin: null pointer", F.who);
  if ((rc = check_ids_host(c, ids, B))) return rc;
  DEVSCOPE(c);
  if ((rc = pl_admit(c, F.pl, F.who))) return rc;
  HostSlot& S = host_slot_begin(c, F.pl);
  const host_staging::DecodeSamples L = host_staging::decode_samples((size_t)c->max_streams, F.hops);
  if ((rc = host_slot_ensure(c, S, L.room))) return rc;
  std::memcpy(S.h_in + L.h_ids, ids, (size_t)B * 4);
  std::memcpy(S.h_in + L.h_packet_bytes, packet_bytes, (size_t)B * 4);
  std::memcpy(S.h_in + L.h_packets, packets, (size_t)B * LYRA_HIP_MAX_PACKET_BYTES);
  int32_t* d_ids = slot_at<int32_t>(S.d_in, L.d_ids);
  int32_t* d_nb = slot_at<int32_t>(S.d_in, L.d_packet_bytes);
  uint8_t* d_pk = S.d_in + L.d_packets;
  HIPCHK(c, hipMemcpyAsync(d_ids, S.h_in + L.h_ids, (size_t)B * 4, hipMemcpyHostToDevice, c->sd[0]));
  HIPCHK(c, hipMemcpyAsync(d_nb, S.h_in + L.h_packet_bytes, (size_t)B * 4, hipMemcpyHostToDevice, c->sd[0]));
  HIPCHK(c, hipMemcpyAsync(d_pk, S.h_in + L.h_packets, (size_t)B * LYRA_HIP_MAX_PACKET_BYTES, hipMemcpyHostToDevice, c->sd[0]));
  if ((rc = F.dev(c, d_ids, B, d_pk, d_nb, num_samples, sample_rate_hz, slot_at<int16_t>(S.d_out, L.d_pcm), nullptr, nullptr)))
    return rc;
  S.n = num_samples;
  return host_slot_begun(c, F.pl, S, B, c->sn);
}

int ds_host_end(lyra_hip_ctx* c, const DsHostForm& F, int16_t* pcm) {
  if (!c) return LYRA_HIP_EINVAL;
  HostSlot* oldest = host_slot_oldest(c, F.pl);
  if (!oldest) return LYRA_HIP_EINVAL;
  HostSlot& S = *oldest;
  if (S.n > 0 && !pcm) return fail(c, LYRA_HIP_EINVAL, "%s_end: null pointer", F.who);
  DEVSCOPE(c);
  const int rc = host_slot_ended(c, F.pl, S, S.n == 0);   // (a request of 0 samples has nothing to download: wait for its kernels)
  if (rc || S.n == 0) return rc;
  const bool overlap = pl_in_flight(c, F.pl) != 0;
  hipStream_t down = overlap ? c->sq[0] : c->sn;
  if (overlap) HIPCHK(c, hipStreamWaitEvent(down, S.ev_done, 0));
  HIPCHK(c, hipMemcpyAsync(pcm, S.d_out, (size_t)S.B * (size_t)S.n * 2, hipMemcpyDeviceToHost, down));
  HIPCHK(c, hipStreamSynchronize(down));
  return 0;
}

const DsHostForm kDsHostForm = {PL_DECODE_SAMPLES, "decode_samples", 1, ds_check_size, lyra_hip_decode_samples_dev};

}  // namespace

extern "C" {

int lyra_hip_decode_samples_dev(lyra_hip_ctx* c, const int32_t* d_ids, int B, const uint8_t* d_packets,
                                const int32_t* d_packet_bytes, int num_samples, int sample_rate_hz, int16_t* d_pcm_ext,
                                int32_t* d_is_noise, int32_t* d_is_comfort_noise) {
  int rc = check_batch(c, B);
  if (rc) return rc;
  if ((rc = ds_check_size(c, num_samples, sample_rate_hz))) return rc;
  if (!d_ids || !d_packets || !d_packet_bytes || (num_samples > 0 && !d_pcm_ext))
    return fail(c, LYRA_HIP_EINVAL, "decode_samples: null pointer");
  return ds_launch(c, d_ids, B, d_packets, d_packet_bytes, num_samples, ds_internal_samples(num_samples, sample_rate_hz),
                   sample_rate_hz, d_pcm_ext, d_is_noise, d_is_comfort_noise);
}

long lyra_hip_decode_samples_errors(lyra_hip_ctx* c, int clear) {
  return read_error_counter(c, &lyra_hip_ctx::d_ds_err, clear);
}

int lyra_hip_decode_samples_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets,
                                  const int32_t* packet_bytes, int num_samples, int sample_rate_hz) {
  return ds_host_begin(c, kDsHostForm, ids, B, packets, packet_bytes, num_samples, sample_rate_hz);
}

int lyra_hip_decode_samples_end(lyra_hip_ctx* c, int16_t* pcm) { return ds_host_end(c, kDsHostForm, pcm); }

}  // extern "C"
