// spans_lossy_api.inc -- part of api.hip, behind spans_api.inc: lyra_hip_decode_spans_lossy[_dev], LyraDecoder's packet-loss path
// (SetEncodedPacket when a packet arrived + DecodeSamples(one hop), lossy_api.inc) over whole spans, time-parallel.
// The loss state machine depends on the receive pattern alone, and packet_bytes is a HOST array: once the span streams' control
// words are known -- the ONE host wait of the call, at its start, for 4 bytes per span -- the plan (spans_lossy_plan.h) names
// every tick's legs, and everything else is enqueued on the decode stream without synchronising:
//   1  the chunked decoder steps on the compacted run_gen list (span_run_steps with the map; concealed rows from zero features);
//      the generative hops land in d_pcm16
//   2  the estimator's log-mel of the received frames, one launch       3  the scan over the received lists, one wavefront per span
//   4 + 5  comfort noise of the run_cng ticks and the mix, in place      the flags, the control words
//   6  the span resampler at 8 / 32 / 48 kHz
// All of the hop-by-hop call's noise-stream half runs here on the decode stream, inside the call's one decode-side bracket.
#include "spans_lossy_plan.h"

namespace {

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// pinned + device bytes for the plan's lists, floats for the snapshots: grow-only, growing drains the stream first
int span_lossy_ensure(lyra_hip_ctx* c, SpanSide& S, hipStream_t st_, size_t list_bytes, size_t snap_floats, int n_ctl) {
  if (n_ctl > S.ctl_cap) {   // (never in flight: the call that enqueues its one reader waits for it)
    if (S.h_ctl) (void)hipHostFree(S.h_ctl);
    S.h_ctl = S.d_ctl = nullptr;
    S.ctl_cap = 0;
    HIPCHK(c, hipHostMalloc((void**)&S.h_ctl, (size_t)n_ctl * sizeof(int32_t), hipHostMallocDefault));
    HIPCHK(c, hipHostGetDevicePointer((void**)&S.d_ctl, S.h_ctl, 0));
    S.ctl_cap = n_ctl;
  }
  if (list_bytes > S.lists_cap) {
    HIPCHK(c, hipStreamSynchronize(st_));
    if (S.h_lists) (void)hipHostFree(S.h_lists);
    S.h_lists = nullptr;
    dfree(S.d_lists);
    S.lists_cap = 0;
    HIPCHK(c, hipHostMalloc((void**)&S.h_lists, list_bytes, hipHostMallocDefault));
    if (dalloc(&S.d_lists, list_bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, LYRA_HIP_ENOMEM, "decode_spans_lossy: %zu bytes of plan lists failed", list_bytes);
    }
    S.lists_cap = list_bytes;
  }
  if (snap_floats > S.snap_cap) {
    HIPCHK(c, hipStreamSynchronize(st_));
    dfree(S.d_snap);
    S.snap_cap = 0;
    if (dalloc(&S.d_snap, snap_floats) != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, LYRA_HIP_ENOMEM, "decode_spans_lossy: %zu estimate snapshots failed", snap_floats / 160);
    }
    S.snap_cap = snap_floats;
  }
  return 0;
}

// lyra_hip_spans_lossy_plan, and with packet_size == slp::SIZE_PER_FRAME lyra_hip_spans_lossy_plan_mixed (spans_mixed_api.inc)
int spans_lossy_plan_sized(const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes, int max_streams,
                           const int32_t* packet_bytes, int packet_size, const uint32_t* ctl_in, lyra_hip_span_lossy_counts* counts,
                           int64_t* gen_frames, uint8_t* gen_received, int64_t* rx_frames, int64_t* cng_frames,
                           int32_t* cng_versions, int32_t* versions, int32_t* info, lyra_hip_span_chunk* chunks, int cap,
                           int* n_steps) {
  const sp::Span* in = reinterpret_cast<const sp::Span*>(spans);
  std::vector<sp::Chunk> dry;
  if (sp::plan(sp::SIDE_DEC, in, n_spans, lane_ids, n_lanes, max_streams, &dry, nullptr) < 0) return LYRA_HIP_EINVAL;
  std::vector<slp::SpanLists> lists;
  if (slp::plan_sized(in, n_spans, packet_bytes, packet_size, ctl_in, &lists) < 0 || (n_spans && !counts)) return LYRA_HIP_EINVAL;
  size_t g = 0, r = 0, k = 0, v = 0, f = 0;
  for (int s = 0; s < n_spans; ++s) {
    const slp::SpanLists& L = lists[(size_t)s];
    counts[s] = lyra_hip_span_lossy_counts{(int64_t)L.gen_frame.size(), (int64_t)L.rx_frame.size(), (int64_t)L.cng_frame.size(),
                                           (int64_t)L.versions.size(), L.ctl_out, 0};
    auto put = [](auto* dst, size_t at, const auto& src) {
      if (dst && !src.empty()) std::memcpy(dst + at, src.data(), src.size() * sizeof(src[0]));
    };
    put(gen_frames, g, L.gen_frame); put(gen_received, g, L.gen_received); put(rx_frames, r, L.rx_frame);
    put(cng_frames, k, L.cng_frame); put(cng_versions, k, L.cng_version); put(versions, v, L.versions); put(info, f, L.info);
    g += L.gen_frame.size(); r += L.rx_frame.size(); k += L.cng_frame.size(); v += L.versions.size(); f += L.info.size();
  }
  const std::vector<sp::Span> compact = slp::compact_gen_spans(in, lists);
  std::vector<sp::Chunk> out;
  const int n = sp::plan(sp::SIDE_DEC, compact.data(), n_spans, lane_ids, n_lanes, max_streams, &out, n_steps);
  if (n < 0 || n > cap || (n && !chunks)) return LYRA_HIP_EINVAL;
  if (n) std::memcpy(chunks, out.data(), (size_t)n * sizeof(sp::Chunk));
  return n;
}

// lyra_hip_decode_spans_lossy_dev, and with `mixed` lyra_hip_decode_spans_lossy_mixed_dev (spans_mixed_api.inc): num_bits is not
// read, a packet has any size of the codec (8 / 15 / 23, chosen per frame), packet rows are MAX_PACKET_BYTES apart, and the list
// uploaded as gen_received holds every tick's size, from which the steps' gather hands it to rvq_decode_mixed_kernel row by row.
// span_rates (spans_rates_api.inc): a HOST array [n_spans], a rate per span; sample_rate_hz is not read, d_pcm_ext rows are
// MAX_EXT_HOP apart and required, and the output resampler is the per-row one.  ext_base (spans_packed_api.inc): with
// span_rates, d_pcm_ext is flat and HOST [n_spans] holds each span's first sample.
int decode_spans_lossy_sized_dev(lyra_hip_ctx* c, const char* what, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                                 int n_lanes, const uint8_t* d_packets, const int32_t* packet_bytes, int num_bits, bool mixed,
                                 int sample_rate_hz, int16_t* d_pcm16, int16_t* d_pcm_ext, int32_t* d_is_noise,
                                 int32_t* d_is_comfort_noise, const int32_t* span_rates = nullptr,
                                 const long long* ext_base = nullptr) {
  const int rate = span_rates ? 16000 : sample_rate_hz;
  const bool ext = span_rates || rate != 16000;
  const SpanExt X{rate, ext ? d_pcm16 : nullptr, span_rates, span_rates ? ext_base : nullptr};
  SpanPlan dry;   // ids, lanes and frame ranges: the planner's rules, on the spans as given
  int rc = span_check(c, what, sp::SIDE_DEC, mixed ? nullptr : &num_bits, spans, n_spans, lane_ids, n_lanes,
                      ext ? d_pcm_ext : d_pcm16, d_packets, X, &dry);
  if (rc) return rc;
  const int nbytes = mixed ? slp::SIZE_PER_FRAME : (num_bits + 7) / 8;
  if (dry.end_frame && !packet_bytes) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  long long total = 0;
  int n_l = 0;   // spans with frames
  for (int s = 0; s < n_spans; ++s) {
    for (int64_t f = spans[s].first_frame; f < spans[s].first_frame + spans[s].n_frames; ++f)
      if (packet_bytes[f] != 0 && (mixed ? !mixed_received(packet_bytes[f]) : packet_bytes[f] != nbytes))
        return fail(c, LYRA_HIP_EINVAL, "%s: packet_bytes[%lld] = %d is neither 0 nor %s%d", what, (long long)f, packet_bytes[f],
                    mixed ? "8, 15 or " : "", mixed ? (int)MAX_PACKET_BYTES : nbytes);
    total += spans[s].n_frames;
    n_l += spans[s].n_frames > 0;
  }
  const SpanPass rs = ext ? span_pass_rows<SpanRsRow>(spans, n_spans, nullptr) : SpanPass();
  if (rs.wgs < 0 || total > INT32_MAX / 2) return fail(c, LYRA_HIP_EINVAL, "%s: too many frames for one pass", what);
  DEVSCOPE(c);
  if (span_rates && (rc = rates_ensure(c))) return rc;
  hipStream_t st_;
  SpanSide& S = span_side_open(c, sp::SIDE_DEC, &st_);
  // the scratch whose size does not depend on the plan, before anything is enqueued: at most one chunk per span and per lane
  const int rows_max = n_spans + n_lanes, n_fix = n_lanes + rs.n + 2 * n_l;
  if ((rc = span_side_ensure(c, S, st_, rows_max, n_fix))) return rc;
  if ((rc = ensure_scratch(c, rows_max))) return rc;
  if ((rc = fade_ensure(c))) return rc;
  if ((rc = span_dtx_ensure(c, S, st_, std::max<long long>(total, 1), n_spans))) return rc;
  const size_t T = (size_t)total;
  // worst case of the lists, every frame in every list: 49 bytes per frame and some alignment
  const size_t lists_max = up16(T * 8) + T * sizeof(SpanLossyRx) + T * sizeof(SpanLossyCng) + up16(T * sizeof(SpanLossyFrame)) + up16(T);
  if ((rc = span_lossy_ensure(c, S, st_, std::max<size_t>(lists_max, 16), 0, n_spans))) return rc;
  if ((rc = span_side_begin(c, sp::SIDE_DEC))) return rc;
  // everything from here on ends in span_side_close, whatever fails: a kernel may already be on the stream
  long long rx_wgs = 0, cng_wgs = 0;
  size_t n_snap = 0;
  SpanPlan P;
  const SpanRow* d_fix = S.d_rows + rows_max;
  const SpanRsRow* d_rs_rows = reinterpret_cast<const SpanRsRow*>(d_fix + n_lanes);
  const SpanLossyRow* d_lrows = reinterpret_cast<const SpanLossyRow*>(d_fix + n_lanes + rs.n);
  const long long* d_gen = nullptr;
  const SpanLossyRx* d_rx = nullptr;
  const SpanLossyCng* d_cng = nullptr;
  const SpanLossyFrame* d_frame = nullptr;
  const uint8_t* d_grx = nullptr;
  auto prepare = [&]() -> int {
    int rc = wait_noise_stream(c);   // the slots of the hop-by-hop call's noise-stream half
    if (rc) return rc;
    c->rs_sn_pending = false;
    // ---- the one host wait: the span streams' control words ----
    std::vector<uint32_t> ctl((size_t)n_spans, 0u);
    if (n_l) {
      for (int s = 0; s < n_spans; ++s) S.h_ctl[s] = spans[s].stream_id;
      hipLaunchKernelGGL(span_lossy_ctl_read_kernel, dim3(cdiv(n_spans, 256)), dim3(256), 0, st_, S.d_ctl, n_spans, c->max_streams,
                         (const uint8_t*)c->sm.base[st::R_CNG]);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipStreamSynchronize(st_));
      S.up_pending = false;
      for (int s = 0; s < n_spans; ++s) ctl[(size_t)s] = (uint32_t)S.h_ctl[s];
    }
    // ---- the plan ----
    std::vector<slp::SpanLists> lists;
    if (slp::plan_sized(reinterpret_cast<const sp::Span*>(spans), n_spans, packet_bytes, nbytes, ctl.data(), &lists) < 0)
      return fail(c, LYRA_HIP_EINVAL, "%s: the plan refused the packet sizes", what);
    const std::vector<sp::Span> compact = slp::compact_gen_spans(reinterpret_cast<const sp::Span*>(spans), lists);
    if ((rc = span_plan_checked(c, sp::SIDE_DEC, reinterpret_cast<const lyra_hip_span*>(compact.data()), n_spans, lane_ids,
                                n_lanes, &P, what)))
      return rc;
    size_t n_gen = 0, n_rx = 0, n_cng = 0;
    for (const slp::SpanLists& L : lists) {
      n_snap += L.versions.size(); n_gen += L.gen_frame.size(); n_rx += L.rx_frame.size(); n_cng += L.cng_frame.size();
    }
    // snapshots: one row per version that some tick reads -- at most one per comfort-noise stretch
    if ((rc = span_lossy_ensure(c, S, st_, 0, n_snap * 160 + (size_t)std::max(n_l, 1), 0))) return rc;
    // ---- rows and lists of the upload; the lists dense, one behind the other, so that one copy moves what is used ----
    const size_t o_gen = 0, o_rx = o_gen + up16(n_gen * 8), o_cng = o_rx + n_rx * sizeof(SpanLossyRx),
                 o_frame = o_cng + n_cng * sizeof(SpanLossyCng), o_grx = o_frame + up16(T * sizeof(SpanLossyFrame)),
                 list_bytes = o_grx + up16(n_gen);
    const int rows = (int)P.chunks.size();
    span_fill_rows(P, reinterpret_cast<const lyra_hip_span*>(compact.data()), lane_ids, 0, S.h_rows);
    SpanRow* h_fix = S.h_rows + rows_max;
    for (int l = 0; l < n_lanes; ++l) h_fix[l] = SpanRow{lane_ids[l], 0, 0, -1, 0, 0, 0};
    if (rs.n) span_pass_rows(spans, n_spans, reinterpret_cast<SpanRsRow*>(h_fix + n_lanes), span_rates, X.base);
    SpanLossyRow* h_lrows = reinterpret_cast<SpanLossyRow*>(h_fix + n_lanes + rs.n);
    long long* h_gen = reinterpret_cast<long long*>(S.h_lists + o_gen);
    SpanLossyRx* h_rx = reinterpret_cast<SpanLossyRx*>(S.h_lists + o_rx);
    SpanLossyCng* h_cng = reinterpret_cast<SpanLossyCng*>(S.h_lists + o_cng);
    SpanLossyFrame* h_frame = reinterpret_cast<SpanLossyFrame*>(S.h_lists + o_frame);
    uint8_t* h_grx = S.h_lists + o_grx;
    size_t g = 0, r = 0, k = 0, f = 0, snap = 0;
    int lr = 0;
    for (int s = 0; s < n_spans; ++s) {
      const slp::SpanLists& L = lists[(size_t)s];
      if (!spans[s].n_frames) continue;
      const size_t snap0 = snap;   // the span's versions take rows snap0 ..., in rising order
      auto row_of_version = [&](int32_t v) {
        return (int32_t)(snap0 + (size_t)(std::lower_bound(L.versions.begin(), L.versions.end(), v) - L.versions.begin()));
      };
      auto snapped = [&](int32_t v) { return std::binary_search(L.versions.begin(), L.versions.end(), v); };
      h_lrows[lr++] = SpanLossyRow{spans[s].first_frame, spans[s].n_frames, (long long)f, spans[s].stream_id,
                                   (int32_t)r, (int32_t)L.rx_frame.size(), (int32_t)rx_wgs,
                                   (int32_t)k, (int32_t)L.cng_frame.size(), (int32_t)cng_wgs,
                                   snapped(0) ? row_of_version(0) : -1, L.ctl_out, 0};
      for (size_t i = 0; i < L.gen_frame.size(); ++i) { h_gen[g] = L.gen_frame[i]; h_grx[g++] = L.gen_received[i]; }
      for (size_t i = 0; i < L.rx_frame.size(); ++i)   // after received frame i the estimate is version i + 1
        h_rx[r++] = SpanLossyRx{L.rx_frame[i], snapped((int32_t)i + 1) ? row_of_version((int32_t)i + 1) : -1, 0};
      for (size_t i = 0; i < L.cng_frame.size(); ++i)
        h_cng[k++] = SpanLossyCng{L.cng_frame[i], row_of_version(L.cng_version[i]),
                                  L.info[(size_t)(L.cng_frame[i] - spans[s].first_frame)]};
      int64_t last_rx = -1;
      for (size_t i = 0; i < L.info.size(); ++i) {
        if (L.info[i] & LOSSY_RX) last_rx = (int64_t)i;
        h_frame[f++] = SpanLossyFrame{L.info[i], last_rx < 0 ? 0 : (int32_t)((int64_t)i - last_rx)};
      }
      rx_wgs += ((long long)L.rx_frame.size() + 1) / 2;
      cng_wgs += (long long)L.cng_frame.size();
      snap += L.versions.size();
    }
    // three uploads: the batch rows; behind their place for the worst case, the fixed rows; the used part of the lists
    if ((rc = span_upload_rows(c, S, st_, 0, rows))) return rc;
    if ((rc = span_upload_rows(c, S, st_, rows_max, n_fix))) return rc;
    if (T) {
      HIPCHK(c, hipMemcpyAsync(S.d_lists, S.h_lists, list_bytes, hipMemcpyHostToDevice, st_));
      HIPCHK(c, hipEventRecord(S.ev_up, st_));
      S.up_pending = true;
    }
    d_gen = reinterpret_cast<const long long*>(S.d_lists + o_gen);
    d_rx = reinterpret_cast<const SpanLossyRx*>(S.d_lists + o_rx);
    d_cng = reinterpret_cast<const SpanLossyCng*>(S.d_lists + o_cng);
    d_frame = reinterpret_cast<const SpanLossyFrame*>(S.d_lists + o_frame);
    d_grx = S.d_lists + o_grx;
    return 0;
  };
  auto passes = [&]() -> int {   // behind the steps
    int32_t* d_entry = reinterpret_cast<int32_t*>(S.d_snap + n_snap * 160);
    uint8_t* est_region = c->sm.base[st::R_NOISE_D];
    uint8_t* cng_region = c->sm.base[st::R_CNG];
    // ---- 2, 3: the estimator over the received frames ----
    if (rx_wgs) {
      hipLaunchKernelGGL(span_logmel_map_kernel, dim3((unsigned)rx_wgs), dim3(256), logmel_lds_bytes(), st_, c->model.d_mel_rate[1],
                         d_lrows, n_l, est_region, d_rx, (const int16_t*)d_pcm16, S.d_mel);
      HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(span_lossy_scan_kernel, dim3(n_l), dim3(64), 0, st_, noise_params(16000), d_lrows, n_l, est_region,
                       (const float*)S.d_mel, d_rx, d_is_noise, S.d_snap, d_entry);
    HIPCHK(c, hipGetLastError());
    // ---- 4, 5: comfort noise and mix, then the accumulators and hop counters ----
    if (cng_wgs) {
      for (int final = 0; final < 2; ++final) {
        hipLaunchKernelGGL(span_cng_kernel, dim3(final ? (unsigned)n_l : (unsigned)cng_wgs), dim3(256), cng_lds_bytes(), st_,
                           c->model.d_mel, c->cng_seed, d_lrows, n_l, final, cng_region, d_cng, (const float*)S.d_snap,
                           (const float*)c->d_fade, d_pcm16);
        HIPCHK(c, hipGetLastError());
      }
    }
    hipLaunchKernelGGL(span_lossy_finish_kernel, dim3((unsigned)cdiv((int)total, 256)), dim3(256), 0, st_, d_lrows, n_l, total,
                       d_frame, cng_region, (const int32_t*)d_entry, d_is_noise, d_is_comfort_noise);
    HIPCHK(c, hipGetLastError());
    // ---- 6: the output resampler ----
    if (ext && rs.n) return launch_span_resample(c, false, st_, d_rs_rows, rs.n, rs.wgs, X, d_pcm16, d_pcm_ext);
    return 0;
  };
  rc = prepare();
  // ---- 1: the steps; the generative hops of the run_gen ticks -> d_pcm16 ----
  const SpanMixed M;
  if (!rc)
    rc = span_run_steps(c, false, S, st_, P, S.h_rows, S.d_rows, d_fix, n_lanes, d_packets, num_bits, d_pcm16, d_gen, d_grx,
                        mixed ? &M : nullptr);
  if (!rc && n_l) rc = passes();
  return span_side_close(c, sp::SIDE_DEC, rc);
}

}  // namespace

extern "C" {

int lyra_hip_spans_lossy_plan(const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes, int max_streams,
                              const int32_t* packet_bytes, int packet_size, const uint32_t* ctl_in,
                              lyra_hip_span_lossy_counts* counts, int64_t* gen_frames, uint8_t* gen_received, int64_t* rx_frames,
                              int64_t* cng_frames, int32_t* cng_versions, int32_t* versions, int32_t* info,
                              lyra_hip_span_chunk* chunks, int cap, int* n_steps) {
  if (packet_size <= 0) return LYRA_HIP_EINVAL;
  return spans_lossy_plan_sized(spans, n_spans, lane_ids, n_lanes, max_streams, packet_bytes, packet_size, ctl_in, counts,
                                gen_frames, gen_received, rx_frames, cng_frames, cng_versions, versions, info, chunks, cap, n_steps);
}

int lyra_hip_decode_spans_lossy_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                    const uint8_t* d_packets, const int32_t* packet_bytes, int num_bits, int sample_rate_hz,
                                    int16_t* d_pcm16, int16_t* d_pcm_ext, int32_t* d_is_noise, int32_t* d_is_comfort_noise) {
  return decode_spans_lossy_sized_dev(c, "decode_spans_lossy", spans, n_spans, lane_ids, n_lanes, d_packets, packet_bytes, num_bits,
                                      false, sample_rate_hz, d_pcm16, d_pcm_ext, d_is_noise, d_is_comfort_noise);
}

// host-buffer form: is_noise / is_comfort_noise may be null, pcm_ext at 16000 too
int lyra_hip_decode_spans_lossy(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                const uint8_t* packets, const int32_t* packet_bytes, int num_bits, int sample_rate_hz,
                                int16_t* pcm16, int16_t* pcm_ext, int32_t* is_noise, int32_t* is_comfort_noise) {
  const char* what = "decode_spans_lossy";
  const int rc = span_check_head(c, what, sp::SIDE_DEC, &num_bits, sample_rate_hz);
  if (rc) return rc;
  const bool ext = sample_rate_hz != 16000;
  auto opt = [](void* host, size_t bytes) { return SpanBuf{host ? SPAN_OUT : SPAN_WORK, host, host ? bytes : 0}; };
  SpanBuf B[] = {{SPAN_IN, (void*)packets, (size_t)(num_bits + 7) / 8}, {SPAN_OUT, pcm16, 640},
                 ext ? SpanBuf{SPAN_OUT, pcm_ext, (size_t)sample_rate_hz / 50 * 2} : SpanBuf{SPAN_WORK, nullptr, 0},
                 opt(is_noise, sizeof(int32_t)), opt(is_comfort_noise, sizeof(int32_t))};
  return span_staged(c, what, sp::SIDE_DEC, spans, n_spans, B, [&] {
    return lyra_hip_decode_spans_lossy_dev(c, spans, n_spans, lane_ids, n_lanes, B[0].d, packet_bytes, num_bits, sample_rate_hz,
                                           (int16_t*)B[1].d, (int16_t*)B[2].d, (int32_t*)B[3].d, (int32_t*)B[4].d);
  });
}

}  // extern "C"
