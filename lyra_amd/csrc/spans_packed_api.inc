// spans_packed_api.inc -- part of api.hip, behind spans_rates_api.inc: the span calls with a sample rate per span on a packed
// external-rate buffer, on device buffers and on host buffers (include/lyra_hip_spans_packed.h).  The `_dev` forms are the
// rates calls' bodies with a SpanExt that also holds each span's base: the rows of the resampler pass carry it and the pass is
// span_resample_packed_kernel (spans_packed_kernels.hip); no other kernel of a span call addresses the external-rate buffer.
// The layout and the offset check are host-only C++ (spans_packed_plan.h).  The host-buffer forms renumber the spans so that
// they lie back to back in every device buffer, stage exactly the spans' frames, and run the `_dev` form on that.
#include "../../include/lyra_hip_spans_packed.h"
#include "spans_packed_plan.h"

#include <initializer_list>
#include <memory>

namespace {

// The offsets of a packed call as the kernel takes them: the caller's, or the back-to-back layout; judged by spk::check.
int packed_resolve(lyra_hip_ctx* c, const char* what, const lyra_hip_span* spans, int n_spans, const int32_t* sample_rates,
                   const long long* ext_offsets, long long n_ext_samples, std::vector<long long>* base) {
  if (n_spans <= 0 || !spans) return fail(c, LYRA_HIP_EINVAL, "%s: no spans", what);
  base->assign((size_t)n_spans, 0);
  if (ext_offsets) std::copy(ext_offsets, ext_offsets + n_spans, base->begin());
  else if (spk::layout(spans, n_spans, sample_rates, base->data()) < 0)
    return fail(c, LYRA_HIP_EINVAL, "%s: the packed layout needs frame counts >= 0 and rates of 8000 / 16000 / 32000 / 48000", what);
  int bad = -1;
  const int e = spk::check(spans, n_spans, sample_rates, base->data(), n_ext_samples, &bad);
  if (e) return fail(c, LYRA_HIP_EINVAL, "%s: %s (span %d, %lld samples in the buffer)", what, spk::error_text(e), bad, n_ext_samples);
  return 0;
}

// ---- host buffers ----------------------------------------------------------------------------------------------------------
// What the host forms share.  The caller's spans name frames and samples anywhere in its buffers; on the device span s takes
// frames frame0[s] .. and samples dev_off[s] .., each the running sum over the spans in front of it, so the staging holds the
// spans' own frames and nothing else.  host_off: where the caller has the span's samples.
struct PackedStage {
  std::vector<lyra_hip_span> spans;     // renumbered: first_frame = the frames of the spans in front
  std::vector<long long> host_off, dev_off;
  long long frames = 0, samples = 0;
  uint8_t* d = nullptr;                 // one allocation: the parts below, each 256-byte aligned
  size_t bytes = 0;
  size_t part(size_t n) {               // reserves n bytes, returns their offset
    const size_t at = bytes;
    bytes += (n + 255) & ~(size_t)255;
    return at;
  }
  ~PackedStage() { if (d) (void)hipFree(d); }
};

// every check of a host form that needs no buffer contents, and the renumbering
int packed_stage_plan(lyra_hip_ctx* c, const char* what, int side, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                      int n_lanes, const int32_t* sample_rates, const long long* ext_offsets, long long n_ext_samples,
                      PackedStage* G) {
  int rc = span_rates_head(c, what, side, nullptr, sample_rates);
  if (rc) return rc;
  if (n_lanes < 0 || (n_lanes && !lane_ids)) return fail(c, LYRA_HIP_EINVAL, "%s: bad lane list", what);
  if ((rc = packed_resolve(c, what, spans, n_spans, sample_rates, ext_offsets, n_ext_samples, &G->host_off))) return rc;
  SpanPlan dry;   // the planner's rules on the spans as given: the renumbered ones could not overlap
  if ((rc = span_plan_checked(c, side, spans, n_spans, lane_ids, n_lanes, &dry, what))) return rc;
  G->spans.assign(spans, spans + n_spans);
  G->dev_off.assign((size_t)n_spans, 0);
  for (int s = 0; s < n_spans; ++s) {
    G->spans[(size_t)s].first_frame = G->frames;
    G->frames += spans[s].n_frames;
  }
  G->samples = spk::layout(spans, n_spans, sample_rates, G->dev_off.data());
  return 0;
}

int packed_stage_alloc(lyra_hip_ctx* c, const char* what, PackedStage* G) {
  if (hipMalloc((void**)&G->d, std::max<size_t>(G->bytes, 256)) != hipSuccess) {
    G->d = nullptr;
    (void)hipGetLastError();
    return fail(c, LYRA_HIP_ENOMEM, "%s: staging %lld frames failed", what, G->frames);
  }
  return 0;
}

// rows of `row` bytes per frame between the caller's frame-major buffer and the staging's dense one
void packed_rows_in(const PackedStage& G, const lyra_hip_span* spans, const void* host, size_t row, uint8_t* dense) {
  for (size_t s = 0; s < G.spans.size(); ++s)
    if (spans[s].n_frames)
      std::memcpy(dense + (size_t)G.spans[s].first_frame * row, (const uint8_t*)host + (size_t)spans[s].first_frame * row,
                  (size_t)spans[s].n_frames * row);
}
void packed_rows_out(const PackedStage& G, const lyra_hip_span* spans, const uint8_t* dense, size_t row, void* host) {
  for (size_t s = 0; host && s < G.spans.size(); ++s)
    if (spans[s].n_frames)
      std::memcpy((uint8_t*)host + (size_t)spans[s].first_frame * row, dense + (size_t)G.spans[s].first_frame * row,
                  (size_t)spans[s].n_frames * row);
}
// the spans' samples between the caller's flat buffer and the staging's back-to-back one
void packed_samples(const PackedStage& G, const int32_t* rates, int16_t* host, int16_t* dense, bool to_host) {
  for (size_t s = 0; s < G.spans.size(); ++s) {
    const size_t n = (size_t)G.spans[s].n_frames * (size_t)(rates[s] / 50) * sizeof(int16_t);
    if (!n) continue;
    if (to_host) std::memcpy(host + G.host_off[s], dense + G.dev_off[s], n);
    else std::memcpy(dense + G.dev_off[s], host + G.host_off[s], n);
  }
}

// the caller has the spans' samples where the staging has them: they travel straight from / to its buffer
bool packed_in_place(const PackedStage& G) {
  for (size_t s = 0; s < G.spans.size(); ++s)
    if (G.spans[s].n_frames && G.host_off[s] != G.dev_off[s]) return false;
  return true;
}

// upload `up` bytes from `src` to the front of the staging, clear the rest, run dev(), drain, then the downloads:
// staging [at, at + n) -> host, each
struct PackedDown { void* host; size_t at, n; };
template <class Dev>
int packed_stage_run(lyra_hip_ctx* c, const char* what, int side, PackedStage& G, const void* src, size_t up,
                     std::initializer_list<PackedDown> downs, Dev dev) {
  hipStream_t st_ = span_stream(c, side);
  int rc = 0;
  if (up && hipMemcpyAsync(G.d, src, up, hipMemcpyHostToDevice, st_) != hipSuccess)
    rc = fail(c, LYRA_HIP_EHIP, "%s: upload failed", what);
  if (!rc && G.bytes > up && hipMemsetAsync(G.d + up, 0, G.bytes - up, st_) != hipSuccess)
    rc = fail(c, LYRA_HIP_EHIP, "%s: upload failed", what);
  if (!rc) rc = dev();
  if (!rc && hipStreamSynchronize(st_) != hipSuccess) rc = fail(c, LYRA_HIP_EHIP, "%s: synchronise failed", what);
  for (const PackedDown& d : downs)
    if (!rc && d.n && hipMemcpy(d.host, G.d + d.at, d.n, hipMemcpyDeviceToHost) != hipSuccess)
      rc = fail(c, LYRA_HIP_EHIP, "%s: download failed", what);
  if (rc) (void)hipStreamSynchronize(st_);   // whatever failed, the side's stream has drained before the staging goes
  return rc;
}

// the decode forms: packets [frames][row] in; samples, optional 16 kHz rows and optional flags out.  lossy: sizes per frame.
int packed_decode_host(lyra_hip_ctx* c, const char* what, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                       int n_lanes, const uint8_t* packets, bool lossy, const int32_t* packet_bytes, int num_bits,
                       const int32_t* sample_rates, int16_t* pcm16, int16_t* pcm_ext, long long n_ext_samples,
                       const long long* ext_offsets, int32_t* is_noise, int32_t* is_cn) {
  PackedStage G;
  int rc = packed_stage_plan(c, what, sp::SIDE_DEC, spans, n_spans, lane_ids, n_lanes, sample_rates, ext_offsets, n_ext_samples, &G);
  if (rc) return rc;
  if (!lossy && (rc = check_bits(c, num_bits))) return rc;
  const size_t T = (size_t)G.frames, row = lossy ? (size_t)MAX_PACKET_BYTES : (size_t)(num_bits + 7) / 8;
  if (T && (!packets || !pcm_ext || (lossy && !packet_bytes))) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  std::vector<int32_t> sizes(lossy ? std::max<size_t>(T, 1) : 0, 0);
  for (int s = 0; lossy && s < n_spans; ++s)
    for (int64_t k = 0; k < spans[s].n_frames; ++k) {
      const int32_t b = packet_bytes[spans[s].first_frame + k];
      if (b != 0 && !mixed_received(b))
        return fail(c, LYRA_HIP_EINVAL, "%s: packet_bytes[%lld] = %d is neither 0 nor 8, 15 or %d", what,
                    (long long)(spans[s].first_frame + k), b, (int)MAX_PACKET_BYTES);
      sizes[(size_t)(G.spans[(size_t)s].first_frame + k)] = b;
    }
  // the staging: packets | noise flags | comfort-noise flags | 16 kHz rows (downloaded only if asked for) | samples
  const size_t o_pk = G.part(T * row), o_noise = G.part(is_noise ? T * 4 : 0), o_cn = G.part(is_cn ? T * 4 : 0), o_16 = G.part(T * 640),
               o_ext = G.part((size_t)G.samples * 2);
  const bool in_place = packed_in_place(G);
  const size_t small1 = pcm16 ? o_16 + T * 640 : o_16, h_bytes = in_place ? small1 : o_ext + (size_t)G.samples * 2;
  std::unique_ptr<uint8_t[]> h(new uint8_t[std::max<size_t>(h_bytes, 1)]);   // (not cleared: every byte read is written first)
  packed_rows_in(G, spans, packets, row, h.get() + o_pk);
  DEVSCOPE(c);
  if ((rc = packed_stage_alloc(c, what, &G))) return rc;
  const PackedDown small{h.get() + o_noise, o_noise, small1 - o_noise};
  const PackedDown samples{in_place ? (void*)pcm_ext : (void*)(h.get() + o_ext), o_ext, (size_t)G.samples * 2};
  rc = packed_stage_run(c, what, sp::SIDE_DEC, G, h.get(), T * row, {small, samples}, [&] {
    int16_t* d16 = (int16_t*)(G.d + o_16);
    int16_t* dext = (int16_t*)(G.d + o_ext);
    if (!lossy)
      return lyra_hip_decode_spans_packed_dev(c, G.spans.data(), n_spans, lane_ids, n_lanes, G.d + o_pk, num_bits, sample_rates, d16,
                                              dext, G.samples, nullptr);
    return lyra_hip_decode_spans_lossy_packed_dev(c, G.spans.data(), n_spans, lane_ids, n_lanes, G.d + o_pk, sizes.data(),
                                                  sample_rates, d16, dext, G.samples, nullptr,
                                                  is_noise ? (int32_t*)(G.d + o_noise) : nullptr,
                                                  is_cn ? (int32_t*)(G.d + o_cn) : nullptr);
  });
  if (rc) return rc;
  if (!in_place) packed_samples(G, sample_rates, pcm_ext, (int16_t*)(h.get() + o_ext), true);
  packed_rows_out(G, spans, h.get() + o_noise, 4, is_noise);
  packed_rows_out(G, spans, h.get() + o_cn, 4, is_cn);
  packed_rows_out(G, spans, h.get() + o_16, 640, pcm16);
  return 0;
}

}  // namespace

extern "C" {

long long lyra_hip_spans_packed_layout(const lyra_hip_span* spans, int n_spans, const int32_t* sample_rates, long long* ext_offsets) {
  if (n_spans < 0 || (n_spans && (!spans || !sample_rates))) return -1;
  return spk::layout(spans, n_spans, sample_rates, ext_offsets);
}

int lyra_hip_encode_spans_packed_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                     const int16_t* d_pcm_ext, long long n_ext_samples, const long long* ext_offsets,
                                     const int32_t* sample_rates, int16_t* d_pcm16, const int32_t* num_bits, int dtx,
                                     uint8_t* d_packets, int32_t* d_packet_bytes) {
  const char* what = "encode_spans_packed";
  int rc = span_rates_head(c, what, sp::SIDE_ENC, nullptr, sample_rates);
  if (rc) return rc;
  if (!num_bits) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  std::vector<long long> base;
  if ((rc = packed_resolve(c, what, spans, n_spans, sample_rates, ext_offsets, n_ext_samples, &base))) return rc;
  return encode_spans_planned_dev(c, what, spans, n_spans, lane_ids, n_lanes, d_pcm_ext, 0, d_pcm16, 0, num_bits, dtx != 0,
                                  d_packets, d_packet_bytes, sample_rates, base.data());
}

int lyra_hip_decode_spans_lossy_packed_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                           int n_lanes, const uint8_t* d_packets, const int32_t* packet_bytes,
                                           const int32_t* sample_rates, int16_t* d_pcm16, int16_t* d_pcm_ext,
                                           long long n_ext_samples, const long long* ext_offsets, int32_t* d_is_noise,
                                           int32_t* d_is_comfort_noise) {
  const char* what = "decode_spans_lossy_packed";
  int rc = span_rates_head(c, what, sp::SIDE_DEC, nullptr, sample_rates);
  if (rc) return rc;
  std::vector<long long> base;
  if ((rc = packed_resolve(c, what, spans, n_spans, sample_rates, ext_offsets, n_ext_samples, &base))) return rc;
  return decode_spans_lossy_sized_dev(c, what, spans, n_spans, lane_ids, n_lanes, d_packets, packet_bytes, 0, true, 0, d_pcm16,
                                      d_pcm_ext, d_is_noise, d_is_comfort_noise, sample_rates, base.data());
}

int lyra_hip_decode_spans_packed_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                     const uint8_t* d_packets, int num_bits, const int32_t* sample_rates, int16_t* d_pcm16,
                                     int16_t* d_pcm_ext, long long n_ext_samples, const long long* ext_offsets) {
  const char* what = "decode_spans_packed";
  int rc = span_rates_head(c, what, sp::SIDE_DEC, &num_bits, sample_rates);
  if (rc) return rc;
  std::vector<long long> base;
  if ((rc = packed_resolve(c, what, spans, n_spans, sample_rates, ext_offsets, n_ext_samples, &base))) return rc;
  return spans_call_dev(c, sp::SIDE_DEC, spans, n_spans, lane_ids, n_lanes, d_packets, num_bits, d_pcm_ext,
                        SpanExt{16000, d_pcm16, sample_rates, base.data()}, what);
}

int lyra_hip_encode_spans_packed(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                 const int16_t* pcm_ext, long long n_ext_samples, const long long* ext_offsets,
                                 const int32_t* sample_rates, const int32_t* num_bits, int dtx, uint8_t* packets,
                                 int32_t* packet_bytes) {
  const char* what = "encode_spans_packed";
  PackedStage G;
  int rc = packed_stage_plan(c, what, sp::SIDE_ENC, spans, n_spans, lane_ids, n_lanes, sample_rates, ext_offsets, n_ext_samples, &G);
  if (rc) return rc;
  const size_t T = (size_t)G.frames, row = (size_t)MAX_PACKET_BYTES;
  if (!num_bits || !packet_bytes || (T && (!pcm_ext || !packets))) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  std::vector<int32_t> bits(std::max<size_t>(T, 1), 4);   // (never empty: the `_dev` form wants the array itself)
  for (int s = 0; s < n_spans; ++s)
    for (int64_t k = 0; k < spans[s].n_frames; ++k) {
      const int32_t b = num_bits[spans[s].first_frame + k];
      if (b < 4 || b > 184 || (b & 3))
        return fail(c, LYRA_HIP_EINVAL, "%s: num_bits[%lld] = %d is not a multiple of 4 in 4..184", what,
                    (long long)(spans[s].first_frame + k), b);
      bits[(size_t)(G.spans[(size_t)s].first_frame + k)] = b;
    }
  // the staging: samples | packets | sizes | 16 kHz workspace
  const size_t o_ext = G.part((size_t)G.samples * 2), o_pk = G.part(T * row), o_sz = G.part(T * 4), o_16 = G.part(T * 640);
  const bool in_place = packed_in_place(G);
  std::unique_ptr<uint8_t[]> h(new uint8_t[in_place ? 1 : std::max<size_t>(o_pk, 1)]), out(new uint8_t[o_sz + T * 4 - o_pk + 1]);   // (out: packets and sizes, from o_pk on)
  if (!in_place) packed_samples(G, sample_rates, const_cast<int16_t*>(pcm_ext), (int16_t*)(h.get() + o_ext), false);
  DEVSCOPE(c);
  if ((rc = packed_stage_alloc(c, what, &G))) return rc;
  const PackedDown results{out.get(), o_pk, o_sz + T * 4 - o_pk};
  rc = packed_stage_run(c, what, sp::SIDE_ENC, G, in_place ? (const void*)pcm_ext : (const void*)h.get(), (size_t)G.samples * 2,
                        {results}, [&] {
    return lyra_hip_encode_spans_packed_dev(c, G.spans.data(), n_spans, lane_ids, n_lanes, (const int16_t*)(G.d + o_ext), G.samples,
                                            nullptr, sample_rates, (int16_t*)(G.d + o_16), bits.data(), dtx, G.d + o_pk,
                                            (int32_t*)(G.d + o_sz));
  });
  if (rc) return rc;
  packed_rows_out(G, spans, out.get(), row, packets);
  packed_rows_out(G, spans, out.get() + (o_sz - o_pk), 4, packet_bytes);
  return 0;
}

int lyra_hip_decode_spans_lossy_packed(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                       int n_lanes, const uint8_t* packets, const int32_t* packet_bytes,
                                       const int32_t* sample_rates, int16_t* pcm16, int16_t* pcm_ext, long long n_ext_samples,
                                       const long long* ext_offsets, int32_t* is_noise, int32_t* is_comfort_noise) {
  return packed_decode_host(c, "decode_spans_lossy_packed", spans, n_spans, lane_ids, n_lanes, packets, true, packet_bytes, 0,
                            sample_rates, pcm16, pcm_ext, n_ext_samples, ext_offsets, is_noise, is_comfort_noise);
}

int lyra_hip_decode_spans_packed(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                 const uint8_t* packets, int num_bits, const int32_t* sample_rates, int16_t* pcm16, int16_t* pcm_ext,
                                 long long n_ext_samples, const long long* ext_offsets) {
  return packed_decode_host(c, "decode_spans_packed", spans, n_spans, lane_ids, n_lanes, packets, false, nullptr, num_bits,
                            sample_rates, pcm16, pcm_ext, n_ext_samples, ext_offsets, nullptr, nullptr);
}

}  // extern "C"
