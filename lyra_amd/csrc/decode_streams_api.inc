// decode_streams_api.inc -- part of api.hip: decoders of any sample rate and packet size in one batch, the hop-synchronous
// receiver (include/lyra_hip_decode_streams.h).
//   lyra_hip_decode_streams_dev: lyra_hip_decode_lossy_rates_dev with each row's samples at an offset of its own inside one
//     buffer (resample_streams_out_kernel: a row that leaves the buffer writes nothing and leaves its resampler slot alone)
//     and with the 16 kHz hop optional (library scratch by call parity, as the tick's own buffers).  Nothing else of the
//     tick changes, so the packed form needs no state of its own.
//   lyra_hip_decode_streams_begin / _end: its two-deep host-buffer form, the input side as lyra_hip_decode_samples_begin
//     (pinned staging, uploaded on the decode-side stream, no synchronisation), the rest as lyra_hip_encode_streams_begin /
//     _end with slots of its own: one download behind the tick on the noise stream, end() waits for its event only.
#include "../../include/lyra_hip_decode_streams.h"

namespace {

struct DstrSlot {
  uint8_t* h_in = nullptr;     // pinned: [ids | packet_bytes | rates | offsets] int32, B each, then packets [B][23]
  uint8_t* h_out = nullptr;    // pinned: [is_noise | is_comfort_noise] int32, B each, then the packed samples
  uint8_t* d_in = nullptr;     // the same on the device (room for max_streams rows each)
  uint8_t* d_out = nullptr;
  hipEvent_t ev_done = nullptr;
  int B = 0;
  long total = 0;              // samples of the packed hop
};
struct DstrHost { DstrSlot slot[2]; };

constexpr size_t kDstrInRow = 4 * 4 + LYRA_HIP_MAX_PACKET_BYTES;          // bytes per stream going up
constexpr size_t kDstrOutRow = 2 * 4 + LYRA_HIP_MAX_EXT_HOP * 2;          // ... and at most coming down

void dstr_free(lyra_hip_ctx* c) {
  dfree(c->d_dstr16[0], c->d_dstr16[1]);
  c->dstr16_cap = 0;
  DstrHost* D = static_cast<DstrHost*>(c->dstr_host);
  if (!D) return;
  for (DstrSlot& S : D->slot) {
    if (S.h_in) (void)hipHostFree(S.h_in);
    if (S.h_out) (void)hipHostFree(S.h_out);
    dfree(S.d_in, S.d_out);
    if (S.ev_done) (void)hipEventDestroy(S.ev_done);
  }
  delete D;
  c->dstr_host = nullptr;
}

int dstr_slot_ensure(lyra_hip_ctx* c, DstrSlot* S) {
  const size_t n = (size_t)c->max_streams;
  if (!S->h_in) HIPCHK(c, hipHostMalloc((void**)&S->h_in, n * kDstrInRow, hipHostMallocDefault));
  if (!S->h_out) HIPCHK(c, hipHostMalloc((void**)&S->h_out, n * kDstrOutRow, hipHostMallocDefault));
  if (!S->d_in) HIPCHK(c, dalloc(&S->d_in, n * kDstrInRow));
  if (!S->d_out) HIPCHK(c, dalloc(&S->d_out, n * kDstrOutRow));
  if (!S->ev_done) HIPCHK(c, hipEventCreateWithFlags(&S->ev_done, hipEventDisableTiming));
  return 0;
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
  if (!c->dstr_host) c->dstr_host = new DstrHost();
  DstrSlot& S = static_cast<DstrHost*>(c->dstr_host)->slot[c->pl_begun[PL_DECODE_STREAMS] & 1];
  if ((rc = dstr_slot_ensure(c, &S))) return rc;
  // everything the tick allocates or builds on first use, BEFORE anything is enqueued: a failure here leaves the streams idle
  if ((rc = rates_ensure(c))) return rc;
  if ((rc = lossy_ensure(c, B))) return rc;
  if ((rc = dstr16_ensure(c, B))) return rc;
  // (the slot's previous user, two calls back, has ended: its kernels on both streams have read d_in, its download has left
  // d_out and h_out)
  const size_t n = (size_t)B;
  int32_t* h = reinterpret_cast<int32_t*>(S.h_in);
  long total = 0;
  for (int b = 0; b < B; ++b) {
    h[b] = ids[b];
    h[n + b] = packet_bytes[b];
    h[2 * n + b] = sample_rates[b];
    h[3 * n + b] = (int32_t)total;   // (at most max_streams * 960 < 2^31: lyra_hip_create's bound on max_streams)
    total += sample_rates[b] / 50;
  }
  std::memcpy(S.h_in + n * 16, packets, n * LYRA_HIP_MAX_PACKET_BYTES);
  // one upload from pinned staging on the decode-side stream, in front of the tick's first kernel: the caller's arrays are
  // free on return and nothing waits on the host
  HIPCHK(c, hipMemcpyAsync(S.d_in, S.h_in, n * kDstrInRow, hipMemcpyHostToDevice, c->sd[0]));
  const int32_t* m = reinterpret_cast<const int32_t*>(S.d_in);
  int32_t* flags = reinterpret_cast<int32_t*>(S.d_out);
  int16_t* pcm = reinterpret_cast<int16_t*>(S.d_out + n * 8);
  if ((rc = lyra_hip_decode_streams_dev(c, m, B, S.d_in + n * 16, m + n, m + 2 * n, pcm, total, m + 3 * n, nullptr, flags,
                                        flags + n)))
    return rc;
  // flags and samples are written by the noise-stream half: their download rides on that stream, behind the resampler
  HIPCHK(c, hipMemcpyAsync(S.h_out, S.d_out, n * 8 + (size_t)total * 2, hipMemcpyDeviceToHost, c->sn));
  HIPCHK(c, hipEventRecord(S.ev_done, c->sn));
  S.B = B;
  S.total = total;
  c->pl_begun[PL_DECODE_STREAMS]++;
  return 0;
}

int lyra_hip_decode_streams_end(lyra_hip_ctx* c, int16_t* pcm, int32_t* is_noise, int32_t* is_comfort_noise) {
  if (!c) return LYRA_HIP_EINVAL;
  if (!c->dstr_host || c->pl_ended[PL_DECODE_STREAMS] == c->pl_begun[PL_DECODE_STREAMS]) return fail(c, LYRA_HIP_EINVAL, "decode_streams_end: no call in flight");
  if (!pcm) return fail(c, LYRA_HIP_EINVAL, "decode_streams_end: null pointer");
  DEVSCOPE(c);
  DstrSlot& S = static_cast<DstrHost*>(c->dstr_host)->slot[c->pl_ended[PL_DECODE_STREAMS] & 1];
  c->pl_ended[PL_DECODE_STREAMS]++;                 // whatever happens below, the slot is given back
  HIPCHK(c, hipEventSynchronize(S.ev_done));
  const size_t n = (size_t)S.B;
  if (is_noise) std::memcpy(is_noise, S.h_out, n * 4);
  if (is_comfort_noise) std::memcpy(is_comfort_noise, S.h_out + n * 4, n * 4);
  std::memcpy(pcm, S.h_out + n * 8, (size_t)S.total * 2);
  return 0;
}

}  // extern "C"
