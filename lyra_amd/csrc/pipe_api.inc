// pipe_api.inc -- part of api.hip: two-deep PIPELINED forms of the host-buffer codec calls (include/lyra_hip.h "Pipelined
// host-buffer calls").  The blocking calls (lyra_hip_encode, lyra_hip_twin_fetch, ...) copy from / to the caller's
// pageable memory on the stream that runs the kernels and synchronise: per hop the chain idles for the upload, the
// download and the host's turnaround (round-5 review, weak #8).  Here a call is split in two:
//   begin()  uploads the caller's audio on a copy stream (straight from the caller's memory; the call waits for the upload
//            only, so the buffer may be reused on return), enqueues the kernels through the `_dev` entry points and -- for
//            the encoder -- the small download of the packets into a pinned slot behind the quantizer, and records an event;
//   end()    waits for the oldest begun call's event and hands the result over (the decoder twin's rows: one download
//            straight into the caller's memory on the copy stream, while the next request's kernels run).
// With begin(n + 1) issued before end(n) the upload of hop n + 1 and the download of hop n run under the kernels: through
// BatchLyraEncoder / BatchLyraDecoder 11.1 -> 18.3 M and 10.4 -> 14.9 M frames/s at 4,096 streams.  Same kernels, same
// order per stream: results are bit-identical to the blocking calls (tests/test_gpu_pipelined.py).

namespace {

// What these three pipelines have beside their slots (HostSlot, api.hip; host_staging::encode / decode; a twin request's slot
// holds where its rows are and the event behind its last kernel).
// Copy streams: the uploads of the encode pipeline and the downloads of the decoder twin overlap the kernels.  They are
// BORROWED from the context -- the noise-estimator stream, idle in both twins (the decoder twin runs its estimator on the
// decode-side stream) -- rather than created:
// a process's streams share a handful of hardware queues (GPU_MAX_HW_QUEUES, 4 by default), and every additional stream
// lands on a queue that a busy stream of this or the other twin's context already uses (measured: both twins on two
// threads 7.5 -> 4.5 M frames/s with two created copy streams per context).
// (both on the noise stream: with the streams of two contexts on queues 0-3 in the same order -- lyra_hip_create -- an
// encoder twin then uses queues 0 (extractor), 2 (quantizer), 3 (uploads) and a decoder twin beside it queue 1 (decoder
// chain) and 3 (downloads): only the two copy streams share a queue)
// The events of all three pipelines' slots are created here, in front of every admission check.
int pipe_ensure(lyra_hip_ctx* c) {
  c->s_up = c->sn;
  c->s_down = c->sn;
  for (int i = 0; i < PL_DEPTH; ++i) {
    if (!c->ev_pipe_up[i]) HIPCHK(c, hipEventCreateWithFlags(&c->ev_pipe_up[i], hipEventDisableTiming));
    for (Pipeline p : {PL_ENCODE, PL_TWIN_FETCH, PL_DECODE})
      if (const int rc = host_slot_event(c, c->pl_slot[p][i])) return rc;
  }
  return 0;
}
void pipe_free(lyra_hip_ctx* c) {
  for (hipEvent_t& e : c->ev_pipe_up) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  dfree(c->d_twin_alt_out, c->d_twin_alt_ext);
  c->twin_alt_out_cap = c->twin_alt_ext_cap = 0;
}
}  // namespace

extern "C" {

int lyra_hip_encode_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const int16_t* pcm, int sample_rate_hz, int num_bits,
                          int dtx) {
  if (!c) return LYRA_HIP_EINVAL;
  int rc = check_batch(c, B);
  if (rc) return rc;
  if ((rc = check_bits(c, num_bits))) return rc;
  if (!pcm) return fail(c, LYRA_HIP_EINVAL, "null pointer");
  if (sample_rate_hz != 8000 && sample_rate_hz != 16000 && sample_rate_hz != 32000 && sample_rate_hz != 48000)
    return fail(c, LYRA_HIP_EINVAL, "encode_begin: sample rate %d", sample_rate_hz);
  if (dtx && c->enc_noise_rate != sample_rate_hz)
    return fail(c, LYRA_HIP_EINVAL, "encode_begin: DTX at %d Hz but the encoder-side noise estimator is set up for %d Hz "
                "(lyra_hip_set_encoder_sample_rate)", sample_rate_hz, c->enc_noise_rate);
  if ((rc = check_ids_host(c, ids, B))) return rc;
  DEVSCOPE(c);
  if ((rc = ensure_scratch(c, B))) return rc;
  if ((rc = pipe_ensure(c))) return rc;
  if ((rc = pl_admit(c, PL_ENCODE, "encode_begin"))) return rc;
  HostSlot& S = host_slot_begin(c, PL_ENCODE);
  const host_staging::Encode L = host_staging::encode((size_t)c->max_streams);
  if ((rc = host_slot_ensure(c, S, L.room))) return rc;
  int32_t* d_ids = slot_at<int32_t>(S.d_in, L.d_ids);
  int16_t* d_in = slot_at<int16_t>(S.d_in, L.d_pcm);
  int16_t* d_16k = slot_at<int16_t>(S.d_in, L.d_pcm16);
  uint8_t* d_pk = S.d_out + L.d_packets;
  int32_t* d_len = slot_at<int32_t>(S.d_out, L.d_packet_bytes);
  hipEvent_t ev_up = c->ev_pipe_up[c->pl_begun[PL_ENCODE] % PL_DEPTH];
  const int n_ext = sample_rate_hz / 50, nbytes = (num_bits + 7) / 8;
  const size_t pcm_b = (size_t)B * n_ext * 2;
  // The audio goes up straight from the caller's memory (the runtime copies pageable memory at the speed of pinned memory on
  // this platform, profiles/r05_batch_twins_host_time.txt; a staging copy would cost a core 0.1-0.2 ms per hop) on the copy
  // stream, which carries nothing else: waiting for it here -- so that the caller may reuse `pcm` on return -- waits for the
  // upload only, never for a kernel.
  // With no other call in flight there is nothing to overlap the upload with: it goes on the extractor's own stream and
  // the copy stream -- one more hardware queue of the few a process has (GPU_MAX_HW_QUEUES, 4 by default) -- stays unused,
  // so that a purely blocking caller (Encode = begin + end) runs exactly as lyra_hip_encode does.
  const bool overlap = c->pl_begun[PL_ENCODE] != c->pl_ended[PL_ENCODE];
  hipStream_t up = overlap ? c->s_up : c->se[0];
  std::memcpy(S.h_in + L.h_ids, ids, (size_t)B * 4);
  HIPCHK(c, hipMemcpyAsync(d_ids, S.h_in + L.h_ids, (size_t)B * 4, hipMemcpyHostToDevice, up));
  HIPCHK(c, hipMemcpyAsync(d_in, pcm, pcm_b, hipMemcpyHostToDevice, up));
  if (overlap) {
    HIPCHK(c, hipEventRecord(ev_up, c->s_up));
    HIPCHK(c, hipStreamSynchronize(c->s_up));
    for (int k = 0; k < c->nsub; ++k) {
      HIPCHK(c, hipStreamWaitEvent(c->se[k], ev_up, 0));
      HIPCHK(c, hipStreamWaitEvent(c->sq[k], ev_up, 0));
    }
  } else {
    // The upload is waited for HERE, on the host, whatever nsub is (nothing of this pipeline is in flight in this branch, so
    // nothing is lost), as the overlapped branch above does for the copy stream.  `pcm` is the caller's again on return: from
    // pinned memory the copy is asynchronous, and without this wait it would read what the caller has put there since
    // (tests/test_gpu_pinned_buffers.py).  With a split batch the other chunks' extractors run on se[1..] and read what
    // se[0] has just uploaded: a kernel enqueued after the copy has completed needs no cross-stream edge behind a copy (the
    // one place that had such an edge, lyra_hip_decode_begin's first form, misbehaved: profiles/EXPERIMENTS.md).
    HIPCHK(c, hipStreamSynchronize(c->se[0]));
  }
  const int16_t* d16 = d_in;
  if (sample_rate_hz != 16000) {   // lyra_encoder.cc:119-122: the encoder's own resampler
    if ((rc = lyra_hip_resample_dev(c, LYRA_HIP_SIDE_ENCODER, d_ids, B, d_in, n_ext, sample_rate_hz, 16000, d_16k))) return rc;
    d16 = d_16k;
  }
  if (dtx) {
    HIPCHK(c, hipMemsetAsync(d_pk, 0, (size_t)B * nbytes, c->se[0]));   // empty packets read back as zeros (lyra_hip_encode_dtx)
    rc = lyra_hip_encode_dtx_dev(c, d_ids, B, d16, num_bits, d_pk, d_len);
  } else {
    rc = lyra_hip_encode_dev(c, d_ids, B, d16, num_bits, d_pk);
  }
  if (rc) return rc;
  // the packets (and DTX's lengths) are written by the quantizer on sq[0]: their small download rides on that stream -- a
  // stream of its own would be one more hardware queue for a 94 KB copy, and a process holds only a few (GPU_MAX_HW_QUEUES)
  for (int k = 1; k < c->nsub; ++k)   // (a split batch: the chunks' quantizers run on sq[1..]; encq_done recorded their ends)
    HIPCHK(c, hipStreamWaitEvent(c->sq[0], c->ev_encs[c->sq_slot[k]][k], 0));
  HIPCHK(c, hipMemcpyAsync(S.h_out + L.h_packets, d_pk, (size_t)B * nbytes, hipMemcpyDeviceToHost, c->sq[0]));
  if (dtx) HIPCHK(c, hipMemcpyAsync(S.h_out + L.h_packet_bytes, d_len, (size_t)B * 4, hipMemcpyDeviceToHost, c->sq[0]));
  S.nbytes = nbytes; S.dtx = dtx;
  return host_slot_begun(c, PL_ENCODE, S, B, c->sq[0]);
}

int lyra_hip_encode_end(lyra_hip_ctx* c, uint8_t* packets, int32_t* packet_bytes) {
  if (!c) return LYRA_HIP_EINVAL;
  HostSlot* oldest = host_slot_oldest(c, PL_ENCODE);
  if (!oldest) return LYRA_HIP_EINVAL;
  if (!packets) return fail(c, LYRA_HIP_EINVAL, "null pointer");
  DEVSCOPE(c);
  HostSlot& S = *oldest;
  if (const int rc = host_slot_ended(c, PL_ENCODE, S, true)) return rc;
  const host_staging::Encode L = host_staging::encode((size_t)c->max_streams);
  std::memcpy(packets, S.h_out + L.h_packets, (size_t)S.B * S.nbytes);
  if (packet_bytes) {
    if (S.dtx) std::memcpy(packet_bytes, S.h_out + L.h_packet_bytes, (size_t)S.B * 4);
    else for (int i = 0; i < S.B; ++i) packet_bytes[i] = S.nbytes;
  }
  return 0;
}

// lyra_hip_decode in two halves (LyraDecoder::SetEncodedPacket + DecodeSamples(320) steady state for B streams): begin()
// uploads ids + packets (94 KB: on the decode-side streams themselves) and enqueues the kernels into the slot's PCM buffer;
// end() downloads the oldest begun call's PCM straight into the caller's memory -- on the copy stream while a younger call's
// kernels run, on the decode-side stream itself when there is none (then exactly lyra_hip_decode).
int lyra_hip_decode_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets, int num_bits) {
  if (!c) return LYRA_HIP_EINVAL;
  int rc = check_batch(c, B);
  if (rc) return rc;
  if ((rc = check_bits(c, num_bits))) return rc;
  if (!packets) return fail(c, LYRA_HIP_EINVAL, "null pointer");
  if ((rc = check_ids_host(c, ids, B))) return rc;
  DEVSCOPE(c);
  if ((rc = ensure_scratch(c, B))) return rc;
  if ((rc = pipe_ensure(c))) return rc;
  if ((rc = pl_admit(c, PL_DECODE, "decode_begin"))) return rc;
  HostSlot& S = host_slot_begin(c, PL_DECODE);
  const host_staging::Decode L = host_staging::decode((size_t)c->max_streams);
  if ((rc = host_slot_ensure(c, S, L.room))) return rc;
  int32_t* d_ids = slot_at<int32_t>(S.d_in, L.d_ids);
  uint8_t* d_pk = S.d_in + L.d_packets;
  const int nbytes = (num_bits + 7) / 8;
  std::memcpy(S.h_in + L.h_ids, ids, (size_t)B * 4);
  std::memcpy(S.h_in + L.h_packets, packets, (size_t)B * nbytes);
  // Each chunk of a split batch uploads its own rows on its own stream, so every kernel follows its inputs in stream
  // order.  (Round 6: with one upload on sd[0] and an event for the other chunks' streams, the second chunk of a call
  // begun while another was in flight decoded the packets the slot held two calls earlier.)
  const int nk = chunks_for(c, B);
  for (int k = 0; k < nk; ++k) {
    int lo = 0, cnt = B;
    if (nk > 1) chunk_of(c, B, k, &lo, &cnt);
    if (cnt <= 0) continue;
    HIPCHK(c, hipMemcpyAsync(d_ids + lo, S.h_in + L.h_ids + (size_t)lo * 4, (size_t)cnt * 4, hipMemcpyHostToDevice, c->sd[k]));
    HIPCHK(c, hipMemcpyAsync(d_pk + (size_t)lo * nbytes, S.h_in + L.h_packets + (size_t)lo * nbytes, (size_t)cnt * nbytes,
                             hipMemcpyHostToDevice, c->sd[k]));
  }
  if ((rc = lyra_hip_decode_dev(c, d_ids, B, d_pk, num_bits, slot_at<int16_t>(S.d_out, L.d_pcm)))) return rc;
  {   // the chunks of a split batch end on sd[1..]: their "done" records (dec_side_done) are this call's
    const int done_slot = (int)((c->n_dec_calls - 1) & 1);
    for (int k = 1; k < c->nsub; ++k) HIPCHK(c, hipStreamWaitEvent(c->sd[0], c->ev_dec[done_slot][k], 0));
  }
  return host_slot_begun(c, PL_DECODE, S, B, c->sd[0]);
}

int lyra_hip_decode_end(lyra_hip_ctx* c, int16_t* pcm) {
  if (!c) return LYRA_HIP_EINVAL;
  HostSlot* oldest = host_slot_oldest(c, PL_DECODE);
  if (!oldest) return LYRA_HIP_EINVAL;
  if (!pcm) return fail(c, LYRA_HIP_EINVAL, "null pointer");
  DEVSCOPE(c);
  HostSlot& S = *oldest;
  (void)host_slot_ended(c, PL_DECODE, S, false);
  const bool overlap = c->pl_ended[PL_DECODE] != c->pl_begun[PL_DECODE];
  hipStream_t down = overlap ? c->s_down : c->sd[0];
  if (overlap) HIPCHK(c, hipStreamWaitEvent(c->s_down, S.ev_done, 0));
  const host_staging::Decode L = host_staging::decode((size_t)c->max_streams);
  HIPCHK(c, hipMemcpyAsync(pcm, S.d_out + L.d_pcm, (size_t)S.B * 640, hipMemcpyDeviceToHost, down));
  HIPCHK(c, hipStreamSynchronize(down));
  return 0;
}

// lyra_hip_twin_fetch in two halves.  begin() ends the request being assembled: its resampling is enqueued, an event is
// recorded behind its last kernel, and the request's output buffers are parked (the next request assembles into the other
// pair), so the NEXT request's twin calls may follow at once.  end() brings the oldest begun request's rows to the caller:
// one device-to-host copy STRAIGHT into the caller's memory on the copy stream -- the runtime copies into pageable memory
// at the speed of pinned memory here (profiles/r05_batch_twins_host_time.txt), a pinned slot plus a host copy cost 0.15-0.25 ms
// per hop when tried -- while the kernels of the request begun after it run.
int lyra_hip_twin_fetch_begin(lyra_hip_ctx* c, int num_streams, int num_internal_samples, int out_rate) {
  if (!c) return LYRA_HIP_EINVAL;
  int rc = check_batch(c, num_streams);
  if (rc) return rc;
  DEVSCOPE(c);
  if ((rc = pipe_ensure(c))) return rc;
  const int n = num_internal_samples;
  auto abandon = [&](int code) {
    (void)hipStreamSynchronize(c->sd[0]);
    c->twin_args_used = 0;
    c->twin_out_n = 0;
    return code;
  };
  // (its own depth only, not pl_admit: a refusal here abandons the request being assembled, and no other pipeline refuses it)
  if (pl_in_flight(c, PL_TWIN_FETCH) >= PL_DEPTH) return abandon(fail(c, LYRA_HIP_EINVAL, "twin_fetch_begin: two requests are already in flight"));
  if (n < 0 || (n > 0 && c->twin_out_n != n)) {
    const int assembled = c->twin_out_n;
    return abandon(fail(c, LYRA_HIP_EINVAL, "twin_fetch: %d samples requested, %d assembled", n, assembled));
  }
  HostSlot& F = host_slot_begin(c, PL_TWIN_FETCH);   // (no staging: the rows stay where the twin calls assembled them)
  F.src_bytes = 0;
  F.src = nullptr;
  if (n > 0) {
    const int16_t* src = c->d_twin_out;
    size_t row = (size_t)n;
    if (out_rate != 16000) {
      ResampleP RP;
      if (!resample_design(16000, out_rate, &RP)) return abandon(fail(c, LYRA_HIP_EINVAL, "twin_fetch: unsupported rate %d", out_rate));
      if (n % RP.down != 0)
        return abandon(fail(c, LYRA_HIP_EINVAL, "twin_fetch: %d internal samples are not a multiple of %d", n, RP.down));
      const int n_ext = n * RP.up / RP.down;
      const size_t need = (size_t)c->max_streams * (size_t)n_ext;
      if (need > c->twin_ext_cap) {   // (this buffer's previous user, two requests back, has ended)
        if (c->d_twin_ext) (void)hipFree(c->d_twin_ext);
        c->d_twin_ext = nullptr;
        c->twin_ext_cap = 0;
        HIPCHK(c, dalloc(&c->d_twin_ext, need));
        c->twin_ext_cap = need;
      }
      const int step = 960 / RP.up;
      for (int s0 = 0; s0 < n; s0 += step) {
        const int n_in = n - s0 < step ? n - s0 : step;
        if ((rc = launch_resample(c, 1, c->d_twin_iota, num_streams, c->d_twin_out + s0, n_in, 16000, out_rate,
                                  c->d_twin_ext + (size_t)s0 * RP.up / RP.down, nullptr, n, n_ext)))
          return abandon(rc);
      }
      src = c->d_twin_ext;
      row = (size_t)n_ext;
    }
    F.src = src;
    F.src_bytes = (size_t)num_streams * row * 2;
  }
  if ((rc = host_slot_begun(c, PL_TWIN_FETCH, F, num_streams, c->sd[0]))) return rc;
  // The staged host arguments of this request stay where they are until the stream has consumed them: the next request
  // stages into the OTHER half of the arena (twin_stage), whose previous user has ended by then.  Likewise its rows: the
  // next request assembles into the other pair of buffers.
  std::swap(c->d_twin_out, c->d_twin_alt_out); std::swap(c->twin_out_cap, c->twin_alt_out_cap);
  std::swap(c->d_twin_ext, c->d_twin_alt_ext); std::swap(c->twin_ext_cap, c->twin_alt_ext_cap);
  c->twin_args_used = 0;
  c->twin_out_n = 0;
  return 0;
}

int lyra_hip_twin_fetch_end(lyra_hip_ctx* c, int16_t* out) {
  if (!c) return LYRA_HIP_EINVAL;
  HostSlot* oldest = host_slot_oldest(c, PL_TWIN_FETCH);
  if (!oldest) return LYRA_HIP_EINVAL;
  DEVSCOPE(c);
  HostSlot& F = *oldest;
  (void)host_slot_ended(c, PL_TWIN_FETCH, F, false);
  // Nothing begun after this request: no kernels to overlap the download with -- it rides on the decode-side stream itself,
  // as in lyra_hip_twin_fetch, and the copy stream (one more of the process's few hardware queues) stays unused.
  const bool overlap = c->pl_ended[PL_TWIN_FETCH] != c->pl_begun[PL_TWIN_FETCH] || c->twin_args_used != 0;
  hipStream_t down = overlap ? c->s_down : c->sd[0];
  if (overlap) HIPCHK(c, hipStreamWaitEvent(c->s_down, F.ev_done, 0));
  if (F.src_bytes) {
    if (!out) return fail(c, LYRA_HIP_EINVAL, "null pointer");
    HIPCHK(c, hipMemcpyAsync(out, F.src, F.src_bytes, hipMemcpyDeviceToHost, down));
  }
  HIPCHK(c, hipStreamSynchronize(down));
  return 0;
}

}  // extern "C"
