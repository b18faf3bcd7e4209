// spans_api.inc -- part of api.hip: lyra_hip_encode_spans[_ext][_dev] / lyra_hip_decode_spans[_ext][_dev], one long recording (or a
// few) through the batched stage kernels time-parallel (spans_plan.h: the warm-up bound and the planner; spans_kernels.hip: the row
// movement and the hand-over).  A call is ONE call of its side for the ordering rules of include/lyra_hip.h "Streams": the
// whole of it runs on the side's first stream (se[0] with the quantizer behind the extractor, as the host form of
// lyra_hip_encode runs it; sd[0]) between enc_side_begin / _done or dec_side_begin / _done, and works on scratch of its own --
// the feature buffers of the `_dev` encode calls may still be read by a quantizer on sq[0].
// Per call: the plan (host), one upload of the rows, lane preparation, T steps of {gather, stages, [quantizer, scatter]},
// hand-over, lane reset.  Nothing is read back and no step waits for the host.
// The `_ext` calls at 8 / 32 / 48 kHz add ONE launch of span_resample_kernel on the same stream inside the same bracket: over all
// frames of the spans in front of the steps (encode: external rate -> the caller's [frames][320] workspace, which the steps
// then read) or behind them (decode: the steps write the workspace).  The resampler needs no lanes: its state is the 34 input
// samples in front of a frame, and those are in the buffer.
// lyra_hip_encode_spans_dtx[_dev] puts the DTX encoder's NoiseEstimator in front of the steps (spans_dtx_kernels.hip: the log-mel
// of all frames in one launch, then one wavefront per span for the recurrence), waits ONCE on the host for the spans' counts of
// non-noise hops, and runs the unchanged steps on the compacted frame list: under DTX the encoder advances on non-noise hops
// only, so what it sees is again a stream whose state is convolution history.  lyra_hip_noise_spans[_dev] is the estimator alone.
// Per-frame bitrates (spans_mixed_api.inc) ride the same steps: span_run_steps with a SpanMixed, encode_spans_planned_dev with
// frame_bits.
// Per-span sample rates (spans_rates_api.inc) ride the same bodies: a SpanExt that holds the caller's array of rates, and the
// passes over every frame are the per-row kernels of spans_rates_kernels.hip.
#include <type_traits>

#include "spans_plan.h"

static_assert(sizeof(lyra_hip_span) == sizeof(sp::Span) && sizeof(lyra_hip_span_chunk) == sizeof(sp::Chunk) &&
                  offsetof(lyra_hip_span_chunk, last) == offsetof(sp::Chunk, last) &&
                  offsetof(lyra_hip_span, n_frames) == offsetof(sp::Span, n_frames),
              "the ABI structs are the planner's");
static_assert(LYRA_HIP_SIDE_ENCODER == sp::SIDE_ENC && LYRA_HIP_SIDE_DECODER == sp::SIDE_DEC, "side numbers");

namespace {

struct SpanSide {
  SpanRow* h_rows = nullptr;        // pinned: the upload of the call in flight
  SpanRow* d_rows = nullptr;        // [rows_cap]: the batch rows, then one row per lane for the final reset, then (`_ext`
                                    // calls) one SpanRsRow per span with frames
  int rows_cap = 0;
  hipEvent_t ev_up = nullptr;       // end of that upload: h_rows may be rewritten
  bool up_pending = false;
  int cap = 0;                      // dense scratch, rows
  uint8_t* d_in = nullptr;          // [cap][640]  gathered PCM (encode) / packets (decode, 23-byte rows at most)
  uint8_t* d_out = nullptr;         // [cap][640]  packets (encode) / PCM (decode) in front of the scatter
  float* d_feat = nullptr;          // [cap][64]   encode: features between extractor and quantizer
  int32_t* d_step_ids = nullptr;    // [cap]       the step's id list (-1: the row has ended)
  int32_t* d_step_size = nullptr;   // [cap]       per-frame bitrates: the step's bit counts (encode) / packet sizes (decode)
  // DTX (encode_spans_dtx, noise_spans): grow-only like the above
  long long dtx_cap = 0;            // frames
  float* d_mel = nullptr;           // [dtx_cap][SPAN_MEL_ROW]  mel rows of the call's frames, span after span
  long long* d_map = nullptr;       // [dtx_cap]   buffer frame of every non-noise frame, a region per span
  int counts_cap = 0;
  int32_t* h_counts = nullptr;      // pinned [counts_cap]: non-noise frames per span with frames, written by the scan
  int32_t* d_counts = nullptr;      // the device's view of h_counts
  // packet loss (decode_spans_lossy, spans_lossy_api.inc): grow-only like the above
  size_t lists_cap = 0;             // bytes
  uint8_t* h_lists = nullptr;       // pinned: the plan's lists of the call in flight (uploaded with the rows: ev_up covers both)
  uint8_t* d_lists = nullptr;
  int ctl_cap = 0;
  int32_t* h_ctl = nullptr;         // pinned [ctl_cap]: span stream ids in, their control words out.  This call's alone, and it
  int32_t* d_ctl = nullptr;         // waits for its read kernel before it goes on: no kernel in flight ever names the buffer
  size_t snap_cap = 0;              // floats
  float* d_snap = nullptr;          // estimate snapshots [versions][160], then one int32 per span: is_noise() on entry
};
struct SpanCalls { SpanSide side[2]; };

SpanCalls* span_calls_of(lyra_hip_ctx* c) { return static_cast<SpanCalls*>(c->span_calls); }

void span_side_free(SpanSide& S) {
  if (S.h_rows) (void)hipHostFree(S.h_rows);
  S.h_rows = nullptr;
  dfree(S.d_rows, S.d_in, S.d_out, S.d_feat, S.d_step_ids, S.d_step_size, S.d_mel, S.d_map);
  if (S.h_counts) (void)hipHostFree(S.h_counts);
  S.h_counts = S.d_counts = nullptr;
  if (S.h_lists) (void)hipHostFree(S.h_lists);
  S.h_lists = nullptr;
  if (S.h_ctl) (void)hipHostFree(S.h_ctl);
  S.h_ctl = S.d_ctl = nullptr;
  S.ctl_cap = 0;
  dfree(S.d_lists, S.d_snap);
  S.lists_cap = S.snap_cap = 0;
  if (S.ev_up) (void)hipEventDestroy(S.ev_up);
  S.ev_up = nullptr;
  S.rows_cap = S.cap = S.counts_cap = 0;
  S.dtx_cap = 0;
}

void spans_free(lyra_hip_ctx* c) {
  SpanCalls* P = span_calls_of(c);
  if (!P) return;
  for (SpanSide& S : P->side) span_side_free(S);
  delete P;
  c->span_calls = nullptr;
}

// buffers of one side for `rows` batch rows + `n_lanes` reset and resampler rows; growing drains the side's stream first
int span_side_ensure(lyra_hip_ctx* c, SpanSide& S, hipStream_t st_, int rows, int n_lanes) {
  if (!S.ev_up) HIPCHK(c, hipEventCreateWithFlags(&S.ev_up, hipEventDisableTiming));
  if (S.up_pending) {   // the previous call's upload has to have left the pinned rows
    HIPCHK(c, hipEventSynchronize(S.ev_up));
    S.up_pending = false;
  }
  if (rows + n_lanes > S.rows_cap) {
    HIPCHK(c, hipStreamSynchronize(st_));
    if (S.h_rows) (void)hipHostFree(S.h_rows);
    S.h_rows = nullptr;
    dfree(S.d_rows);
    S.rows_cap = 0;
    HIPCHK(c, hipHostMalloc((void**)&S.h_rows, (size_t)(rows + n_lanes) * sizeof(SpanRow), hipHostMallocDefault));
    HIPCHK(c, dalloc(&S.d_rows, (size_t)(rows + n_lanes)));
    S.rows_cap = rows + n_lanes;
  }
  if (rows > S.cap) {
    HIPCHK(c, hipStreamSynchronize(st_));
    dfree(S.d_in, S.d_out, S.d_feat, S.d_step_ids, S.d_step_size);
    S.cap = 0;
    HIPCHK(c, dalloc(&S.d_in, (size_t)rows * 640));
    HIPCHK(c, dalloc(&S.d_out, (size_t)rows * 640));
    HIPCHK(c, dalloc(&S.d_feat, (size_t)rows * 64));
    HIPCHK(c, dalloc(&S.d_step_ids, (size_t)rows));
    HIPCHK(c, dalloc(&S.d_step_size, (size_t)rows));
    S.cap = rows;
  }
  return 0;
}

struct SpanPlan {
  std::vector<sp::Chunk> chunks;
  int n_own = 0, n_steps = 0;
  int64_t end_frame = 0;   // one past the last buffer frame any span names
};

// one past the last buffer frame a span names -- a span without frames names its first (spans the planner refuses name none)
int64_t span_end_frame(const lyra_hip_span* spans, int n_spans) {
  int64_t end = 0;
  for (int s = 0; spans && s < n_spans; ++s)
    if (spans[s].first_frame >= 0 && spans[s].n_frames >= 0) end = std::max<int64_t>(end, spans[s].first_frame + spans[s].n_frames);
  return end;
}

int span_plan_checked(lyra_hip_ctx* c, int side, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                      SpanPlan* P, const char* what) {
  if (n_spans <= 0 || !spans) return fail(c, LYRA_HIP_EINVAL, "%s: no spans", what);
  const int n = sp::plan(side, reinterpret_cast<const sp::Span*>(spans), n_spans, lane_ids, n_lanes, c->max_streams, &P->chunks,
                         &P->n_steps);
  if (n < 0)
    return fail(c, LYRA_HIP_EINVAL,
                "%s: span and lane ids must be distinct streams of the context (0..%d), frame ranges non-negative and disjoint",
                what, c->max_streams - 1);
  for (const sp::Chunk& ch : P->chunks) P->n_own += ch.n_warmup == 0;
  P->end_frame = span_end_frame(spans, n_spans);
  return 0;
}

void span_fill_rows(const SpanPlan& P, const lyra_hip_span* spans, const int32_t* lane_ids, int n_lanes, SpanRow* rows) {
  int r = 0;
  for (const sp::Chunk& ch : P.chunks) {
    const bool lane = ch.n_warmup > 0;
    rows[r++] = SpanRow{ch.stream_id, ch.n_warmup + ch.n_frames, ch.n_warmup, lane ? spans[ch.span].stream_id : -1,
                        ch.phase_offset, ch.last, (long long)(ch.first_frame - ch.n_warmup)};
  }
  for (int l = 0; l < n_lanes; ++l) rows[r++] = SpanRow{lane_ids[l], 0, 0, -1, 0, 0, 0};
}

// rows of the batch that still run at step i: own rows and lane rows are each sorted by falling step count
int span_batch_at(const SpanPlan& P, const SpanRow* rows, int step, int* own_running) {
  const int n = (int)P.chunks.size();
  int own = 0, lanes = 0;
  while (own < P.n_own && rows[own].n_steps > step) ++own;
  while (P.n_own + lanes < n && rows[P.n_own + lanes].n_steps > step) ++lanes;
  *own_running = own;
  return lanes ? P.n_own + lanes : own;
}

inline int span_grid(int B, int units) { return (int)(((long long)B * units + 255) / 256); }

// The external-rate side of an `_ext` call: ONE rate (16000 = none, the call is the plain one), or a rate per span
// (spans_rates_api.inc): `rates` is the caller's HOST array [n_spans], `rate` is not read, rows of the external-rate buffer are
// MAX_EXT_HOP samples apart whatever the span's rate, the 16 kHz buffer is always needed (a 16 kHz span is copied through), and
// the passes over every frame are the kernels of spans_rates_kernels.hip.
struct SpanExt {
  int rate = 16000;
  int16_t* d_pcm16 = nullptr;   // [frames][320], the caller's: resampled input (encode) / the steps' output (decode)
  const int32_t* rates = nullptr;
  const long long* base = nullptr;   // with rates (spans_packed_api.inc): the external-rate buffer is flat, HOST [n_spans] = each
                                     // span's first sample, checked by the caller (spans_packed_plan.h); n_ext() is not used
  int n_ext() const { return rates ? (int)LYRA_HIP_MAX_EXT_HOP : rate / 50; }   // samples between rows of the external-rate buffer
  bool on() const { return rates || rate != 16000; }
};

// Rows of the kernels that pass once over every frame of a call, one row per span with frames.  Row = SpanRsRow:
// span_resample_kernel, four frames per workgroup; SpanDtxRow: span_logmel_kernel / span_noise_scan_kernel, two frames per
// log-mel workgroup, region = the frames of the rows in front.  rows == nullptr only counts.  wgs < 0: too many for one launch.
// rates (SpanRsRow, a rate per span): the row carries its span's rate, for the estimator's rows of the same index too.
struct SpanPass {
  int n = 0;                      // rows
  long long wgs = 0, frames = 0;  // workgroups and frames of all rows
};
template <class Row>
SpanPass span_pass_rows(const lyra_hip_span* spans, int n_spans, Row* rows, const int32_t* rates = nullptr,
                        const long long* base = nullptr) {
  constexpr bool dtx = std::is_same<Row, SpanDtxRow>::value;
  SpanPass p;
  for (int s = 0; s < n_spans; ++s) {
    if (!spans[s].n_frames) continue;
    if (rows) {
      rows[p.n] = Row{spans[s].first_frame, spans[s].n_frames, spans[s].stream_id, (int32_t)p.wgs};
      if constexpr (dtx) rows[p.n].region = p.frames;
      else {
        rows[p.n].pad[0] = rates ? rates[s] : 0;
        rows[p.n].pad[1] = base ? (int32_t)(base[s] / 8) : 0;   // (packed: span_resample_packed_kernel)
      }
    }
    ++p.n;
    p.wgs += dtx ? (spans[s].n_frames + 1) / 2 : (spans[s].n_frames + 3) / 4;
    p.frames += spans[s].n_frames;
    if (p.wgs > INT32_MAX) {
      p.wgs = -1;
      break;
    }
  }
  return p;
}

// one launch over every frame of every span on st_: enc: d_in [frames][X.n_ext()] at the external rate -> d_out [frames][320];
// else d_in [frames][320] -> d_out [frames][X.n_ext()] (slots: see launch_resample -- behind run_steps' launches ahead on the
// quantizer stream / on the noise stream).  X.rates: the rows carry their rates and c->d_rs_tab is there (rates_ensure).
int launch_span_resample(lyra_hip_ctx* c, bool enc, hipStream_t st_, const SpanRsRow* d_rows, int n_rows, long long wgs,
                         const SpanExt& X, const int16_t* d_in, int16_t* d_out) {
  const int from = enc ? X.rate : 16000, to = enc ? 16000 : X.rate;
  ResampleP P;
  if (!X.rates && !resample_design(from, to, &P))
    return fail(c, LYRA_HIP_EINVAL, "spans: unsupported resampling %d -> %d Hz", from, to);
  int rc = 0;
  if (enc) {
    if ((rc = wait_ahead(c))) return rc;
  } else if (c->rs_sn_pending) {
    if ((rc = wait_noise_stream(c))) return rc;
    c->rs_sn_pending = false;
  }
  if (X.base) {   // the flat external-rate buffer: the rows carry their bases too
    ProfScope ps(c, K_SPAN_RS_PACKED, st_);
    hipLaunchKernelGGL(span_resample_packed_kernel, dim3((unsigned)wgs), dim3(256), resample_rates_lds_bytes(), st_,
                       (const ResampleP*)c->d_rs_tab, enc ? 0 : 1, d_rows, n_rows, c->sm.base[enc ? st::R_RS_E : st::R_RS_D], d_in,
                       d_out);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  if (X.rates) {
    ProfScope ps(c, K_SPAN_RS_RATES, st_);
    hipLaunchKernelGGL(span_resample_rates_kernel, dim3((unsigned)wgs), dim3(256), resample_rates_lds_bytes(), st_,
                       (const ResampleP*)c->d_rs_tab, enc ? 0 : 1, d_rows, n_rows, c->sm.base[enc ? st::R_RS_E : st::R_RS_D], d_in,
                       enc ? X.n_ext() : 320, d_out, enc ? 320 : X.n_ext());
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  const int n_in = from / 50, n_out = to / 50;
  hipLaunchKernelGGL(span_resample_kernel, dim3((unsigned)wgs), dim3(256), resample_lds_bytes(n_in), st_, P, d_rows, n_rows,
                     c->sm.base[enc ? st::R_RS_E : st::R_RS_D], d_in, n_in, d_out, n_out);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// Lane preparation, the T steps, hand-over and lane reset of one call on st_.  h_batch / d_batch: the plan's rows (host copy
// and device), d_reset: one row per lane.  enc: d_src PCM [frames][320], d_dst packets [frames][nbytes]; else the reverse.
// d_map (encode_spans_dtx, decode_spans_lossy): the plan counts frames in the compacted list, index c is buffer frame d_map[c].
// d_gen_received (decode_spans_lossy): entry c of that list came with a packet; the others decode from zero features.
// M (spans_mixed_api.inc): per-frame bitrates.  num_bits is not read, packet rows are MAX_PACKET_BYTES long, the gather leaves
// every row's bit count (encode: M->d_frame_bits by buffer frame) or packet size (decode: d_gen_received holds the sizes) in
// S.d_step_size and the mixed quantizer kernels take it from there: launch for launch the uniform step.
struct SpanMixed {
  const int32_t* d_frame_bits = nullptr;   // encode: [frames], the device copy of the caller's num_bits
  int32_t* d_packet_bytes = nullptr;       // encode: [frames], the caller's
};
int span_run_steps(lyra_hip_ctx* c, bool enc, SpanSide& S, hipStream_t st_, const SpanPlan& P, const SpanRow* h_batch,
                   const SpanRow* d_batch, const SpanRow* d_reset, int n_lanes, const void* d_src, int num_bits, void* d_dst,
                   const long long* d_map, const uint8_t* d_gen_received = nullptr, const SpanMixed* M = nullptr) {
  const int rows = (int)P.chunks.size(), nbytes = M ? (int)MAX_PACKET_BYTES : (num_bits + 7) / 8, r0 = enc ? st::R_E0 : st::R_D0;
  int rc = 0;
  const int n_lane_rows = rows - P.n_own;
  if (n_lane_rows) {
    hipLaunchKernelGGL(span_lane_init_kernel, dim3(n_lane_rows), dim3(256), 0, st_, c->model.d_reset, d_batch + P.n_own,
                       n_lane_rows, r0, c->sm);
    HIPCHK(c, hipGetLastError());
  }
  const int W = sp::warmup(enc ? sp::SIDE_ENC : sp::SIDE_DEC);
  const int in_bytes = enc ? 640 : nbytes, out_bytes = enc ? nbytes : 640;
  for (int i = 0; i < P.n_steps && !rc; ++i) {
    int own = 0;
    const int B = span_batch_at(P, h_batch, i, &own);
    if (M)
      hipLaunchKernelGGL(span_gather_mixed_kernel, dim3(span_grid(B, enc ? 40 : in_bytes)), dim3(256), 0, st_, d_batch, B, i,
                         (const uint8_t*)d_src, enc ? M->d_frame_bits : nullptr, enc ? nullptr : d_gen_received, S.d_in,
                         S.d_step_ids, S.d_step_size, d_map);
    else
      hipLaunchKernelGGL(span_gather_kernel, dim3(span_grid(B, enc ? 40 : in_bytes)), dim3(256), 0, st_, d_batch, B, i,
                         (const uint8_t*)d_src, in_bytes, enc ? 1 : 0, S.d_in, S.d_step_ids, d_map);
    HIPCHK(c, hipGetLastError());
    if (enc) {
      rc = launch_extract(c, 0, 0, S.d_step_ids, B, (const int16_t*)S.d_in, S.d_feat);
      // warm-up steps of the lanes skip the quantizer: before step W only the spans' own rows produce
      const int Bq = i < W ? own : B;
      if (!rc && Bq && !M) rc = launch_rvq_encode(c, 0, Bq, S.d_feat, num_bits / 4, nullptr, S.d_out, S.d_step_ids);
      if (rc || !Bq) continue;
      if (M) {   // (rows that have ended carry a valid count: the kernel's error word judges every row < Bq)
        { ProfScope ps(c, K_RVQ_ENC, st_);
          hipLaunchKernelGGL(rvq_encode_mixed_kernel, dim3(cdiv(Bq, 16)), dim3(64), 0, st_, c->model.cb, c->model.cbn, S.d_feat, Bq,
                             S.d_step_size, S.d_out, S.d_step_ids, (int32_t*)nullptr, c->d_rvq_stats, c->d_mixed_err); }
        HIPCHK(c, hipGetLastError());
        hipLaunchKernelGGL(span_scatter_mixed_kernel, dim3(span_grid(Bq, out_bytes)), dim3(256), 0, st_, d_batch, Bq, i, S.d_out,
                           S.d_step_size, (uint8_t*)d_dst, M->d_packet_bytes, d_map);
      } else
        hipLaunchKernelGGL(span_scatter_kernel, dim3(span_grid(Bq, out_bytes)), dim3(256), 0, st_, d_batch, Bq, i, S.d_out,
                           out_bytes, 0, (uint8_t*)d_dst, d_map);
    } else {
      if (d_gen_received) {   // as a lossy tick: the RVQ decode of every row, zero features where the tick conceals
        if (M) {
          { ProfScope ps(c, K_RVQ_DEC, st_);
            hipLaunchKernelGGL(rvq_decode_mixed_kernel, dim3(cdiv(B, 4)), dim3(256), 0, st_, c->model.cb, S.d_in, S.d_step_size, 0, B,
                               S.d_feat); }
          HIPCHK(c, hipGetLastError());
        } else if ((rc = launch_rvq_decode(c, 0, B, nullptr, S.d_in, num_bits / 4, S.d_feat))) continue;
        hipLaunchKernelGGL(span_lossy_feat_kernel, dim3(span_grid(B, 64)), dim3(256), 0, st_, d_batch, B, i, d_gen_received,
                           S.d_feat);
        HIPCHK(c, hipGetLastError());
        if ((rc = launch_generate(c, 0, 0, S.d_step_ids, B, S.d_feat, (int16_t*)S.d_out))) continue;
      } else if ((rc = launch_generate(c, 0, 0, S.d_step_ids, B, nullptr, (int16_t*)S.d_out, S.d_in, num_bits / 4))) continue;
      const int Bs = i < W ? own : B;
      if (!Bs) continue;
      hipLaunchKernelGGL(span_scatter_kernel, dim3(span_grid(Bs, 40)), dim3(256), 0, st_, d_batch, Bs, i, S.d_out, out_bytes,
                         1, (uint8_t*)d_dst, d_map);
    }
    HIPCHK(c, hipGetLastError());
  }
  if (!rc && n_lane_rows) {
    hipLaunchKernelGGL(span_handover_kernel, dim3(n_lane_rows), dim3(256), 0, st_, d_batch + P.n_own, n_lane_rows, r0, c->sm);
    HIPCHK(c, hipGetLastError());
  }
  if (!rc && n_lanes) {   // every lane the caller lent, used or not, comes back reset
    hipLaunchKernelGGL(span_lane_init_kernel, dim3(n_lanes), dim3(256), 0, st_, c->model.d_reset, d_reset, n_lanes, r0, c->sm);
    HIPCHK(c, hipGetLastError());
  }
  return rc;
}

// ---- what the calls share ------------------------------------------------------------------------------------------------
bool span_rate_ok(int rate) { return rate == 8000 || rate == 16000 || rate == 32000 || rate == 48000; }
hipStream_t span_stream(lyra_hip_ctx* c, int side) { return side == sp::SIDE_ENC ? c->se[0] : c->sd[0]; }

// the side's state of the span calls (created on first use) and its stream
SpanSide& span_side_open(lyra_hip_ctx* c, int side, hipStream_t* st_) {
  if (!c->span_calls) c->span_calls = new SpanCalls();
  *st_ = span_stream(c, side);
  return span_calls_of(c)->side[side];
}

int span_side_begin(lyra_hip_ctx* c, int side) { return side == sp::SIDE_ENC ? enc_side_begin(c, 0) : dec_side_begin(c, 0); }

// the end of the call's bracket, rc: what the enqueue gave; a decoder-side call counts as one whether or not it failed
int span_side_close(lyra_hip_ctx* c, int side, int rc) {
  if (side == sp::SIDE_ENC) return rc ? rc : enc_side_done(c, 0);
  if (!rc) rc = dec_side_done(c, 0, 1);
  c->n_dec_calls++;
  return rc;
}

// pinned rows [first, first + n) -> the device's rows on st_; ev_up: the end of the side's last upload
int span_upload_rows(lyra_hip_ctx* c, SpanSide& S, hipStream_t st_, int first, int n) {
  if (!n) return 0;
  HIPCHK(c, hipMemcpyAsync(S.d_rows + first, S.h_rows + first, (size_t)n * sizeof(SpanRow), hipMemcpyHostToDevice, st_));
  HIPCHK(c, hipEventRecord(S.ev_up, st_));
  S.up_pending = true;
  return 0;
}

// In front of the encoder's steps at another rate: ONE resampler pass, *d_pcm [frames][X.n_ext()] -> the 16 kHz workspace, which
// the steps then read: *d_pcm becomes the workspace.
int span_encode_front(lyra_hip_ctx* c, hipStream_t st_, const SpanExt& X, const SpanRsRow* d_rs_rows, const SpanPass& rs,
                      const int16_t** d_pcm) {
  if (!X.on()) return 0;
  const int rc = rs.n ? launch_span_resample(c, true, st_, d_rs_rows, rs.n, rs.wgs, X, *d_pcm, X.d_pcm16) : 0;
  if (!rc) *d_pcm = X.d_pcm16;
  return rc;
}

// What every form checks first: the context, the side, the bit count (num_bits == nullptr: the call has none), the rate.
int span_check_head(lyra_hip_ctx* c, const char* what, int side, const int* num_bits, int rate) {
  if (!c) return LYRA_HIP_EINVAL;
  if (sp::warmup(side) < 0) return fail(c, LYRA_HIP_EINVAL, "%s: bad side", what);
  const int rc = num_bits ? check_bits(c, *num_bits) : 0;
  if (rc) return rc;
  if (!span_rate_ok(rate)) return fail(c, LYRA_HIP_EINVAL, "%s: sample rate %d Hz (8000 / 16000 / 32000 / 48000)", what, rate);
  return 0;
}

// The argument check of the `_dev` forms, before anything of the context is touched: span_check_head, the lane list, the
// planner's rules on the spans as given (*P: that plan), with a rate per span every span's rate, d_pcm and d_other non-null once
// a span names a frame, d_pcm 16-byte aligned, and at another rate (always, with a rate per span) the 16 kHz workspace.
int span_check(lyra_hip_ctx* c, const char* what, int side, const int* num_bits, const lyra_hip_span* spans, int n_spans,
               const int32_t* lane_ids, int n_lanes, const void* d_pcm, const void* d_other, const SpanExt& X, SpanPlan* P) {
  int rc = span_check_head(c, what, side, num_bits, X.rate);
  if (rc) return rc;
  if (n_lanes < 0 || (n_lanes && !lane_ids)) return fail(c, LYRA_HIP_EINVAL, "%s: bad lane list", what);
  if ((rc = span_plan_checked(c, side, spans, n_spans, lane_ids, n_lanes, P, what))) return rc;
  for (int s = 0; X.rates && s < n_spans; ++s)
    if (!span_rate_ok(X.rates[s]))
      return fail(c, LYRA_HIP_EINVAL, "%s: sample_rates[%d] = %d Hz (8000 / 16000 / 32000 / 48000)", what, s, X.rates[s]);
  if (P->end_frame && (!d_pcm || !d_other)) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  if (reinterpret_cast<uintptr_t>(d_pcm) & 15) return fail(c, LYRA_HIP_EINVAL, "%s: the PCM buffer must be 16-byte aligned", what);
  if (X.on() && ((P->end_frame && !X.d_pcm16) || (reinterpret_cast<uintptr_t>(X.d_pcm16) & 15))) {
    if (X.rates) return fail(c, LYRA_HIP_EINVAL, "%s: with a rate per span the 16 kHz buffer must be given, 16-byte aligned", what);
    return fail(c, LYRA_HIP_EINVAL, "%s: at %d Hz the 16 kHz buffer must be given, 16-byte aligned", what, X.rate);
  }
  return 0;
}

// One buffer of a blocking host-buffer form, `bytes` per frame: frames 0 .. end - 1 are staged on the device.
enum SpanDir { SPAN_IN, SPAN_OUT, SPAN_WORK };   // uploaded | the spans' own frames read back | neither: the call's workspace
struct SpanBuf {
  SpanDir dir;
  void* host;
  size_t bytes;         // 0: the call does without the buffer, d stays null
  bool zero = false;    // the device copy starts as zeros: rows of a span that the call does not write read back as zeros
  uint8_t* d = nullptr;
};

// The blocking host-buffer forms: allocate, upload, run the `_dev` form (dev(), on B[k].d), synchronise, read back the spans'
// own frames, free.  Whatever fails, the side's stream has drained before the staging buffers go.
template <size_t N, class Dev>
int span_staged(lyra_hip_ctx* c, const char* what, int side, const lyra_hip_span* spans, int n_spans, SpanBuf (&B)[N], Dev dev) {
  const size_t end = (size_t)span_end_frame(spans, n_spans);
  for (const SpanBuf& b : B)
    if (end && b.dir != SPAN_WORK && !b.host) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  DEVSCOPE(c);
  hipStream_t st_ = span_stream(c, side);
  int rc = 0;
  for (SpanBuf& b : B) {
    const size_t bytes = end * b.bytes;
    if (rc || !b.bytes) continue;
    if (hipMalloc((void**)&b.d, std::max<size_t>(bytes, 1)) != hipSuccess)
      rc = fail(c, LYRA_HIP_ENOMEM, "%s: staging %zu frames failed", what, end);
    else if (bytes && (b.dir == SPAN_IN ? hipMemcpy(b.d, b.host, bytes, hipMemcpyHostToDevice)
                       : b.zero         ? hipMemset(b.d, 0, bytes)
                                        : hipSuccess) != hipSuccess)
      rc = fail(c, LYRA_HIP_EHIP, "%s: upload failed", what);
  }
  if (!rc) rc = dev();
  if (!rc && hipStreamSynchronize(st_) != hipSuccess) rc = fail(c, LYRA_HIP_EHIP, "%s: synchronise failed", what);
  for (int s = 0; !rc && s < n_spans; ++s)
    for (const SpanBuf& b : B) {
      const size_t at = (size_t)spans[s].first_frame * b.bytes, n = (size_t)spans[s].n_frames * b.bytes;
      if (!rc && b.dir == SPAN_OUT && n && hipMemcpy((uint8_t*)b.host + at, b.d + at, n, hipMemcpyDeviceToHost) != hipSuccess)
        rc = fail(c, LYRA_HIP_EHIP, "%s: download failed", what);
    }
  if (rc) (void)hipStreamSynchronize(st_);
  for (SpanBuf& b : B) dfree(b.d);
  return rc;
}

// ---- the plain and `_ext` calls ----------------------------------------------------------------------------------------------
// side SIDE_ENC: d_src PCM [frames][320], d_dst packets [frames][nbytes]; SIDE_DEC the reverse.  X.on(): the PCM of d_src /
// d_dst is [frames][X.n_ext()] and the steps work on X.d_pcm16.  what: the call's name in error texts (null: that of the side).
int spans_call_dev(lyra_hip_ctx* c, int side, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                   const void* d_src, int num_bits, void* d_dst, const SpanExt& X = SpanExt(), const char* what = nullptr) {
  const bool enc = side == sp::SIDE_ENC;
  if (!what) what = enc ? "encode_spans" : "decode_spans";
  SpanPlan P;
  int rc = span_check(c, what, side, &num_bits, spans, n_spans, lane_ids, n_lanes, enc ? d_src : d_dst, enc ? d_dst : d_src, X, &P);
  if (rc) return rc;
  const SpanPass rs = X.on() ? span_pass_rows<SpanRsRow>(spans, n_spans, nullptr) : SpanPass();
  if (rs.wgs < 0) return fail(c, LYRA_HIP_EINVAL, "%s: too many frames for one pass", what);
  DEVSCOPE(c);
  if (X.rates && (rc = rates_ensure(c))) return rc;
  hipStream_t st_;
  SpanSide& S = span_side_open(c, side, &st_);
  const int rows = (int)P.chunks.size();
  if ((rc = span_side_ensure(c, S, st_, std::max(rows, 1), n_lanes + rs.n))) return rc;
  if (rows && (rc = ensure_scratch(c, rows))) return rc;   // the stage kernels' own boundary buffers
  span_fill_rows(P, spans, lane_ids, n_lanes, S.h_rows);
  const int rs0 = rows + n_lanes;   // the resampler's rows lie behind the lanes' reset rows
  if (rs.n) span_pass_rows(spans, n_spans, reinterpret_cast<SpanRsRow*>(S.h_rows + rs0), X.rates, X.base);
  if ((rc = span_side_begin(c, side))) return rc;
  if ((rc = span_upload_rows(c, S, st_, 0, rs0 + rs.n))) return rc;
  const SpanRsRow* d_rs_rows = reinterpret_cast<const SpanRsRow*>(S.d_rows + rs0);
  void* d_ext_out = nullptr;
  if (enc) {   // the steps read the 16 kHz workspace ...
    const int16_t* d_pcm = static_cast<const int16_t*>(d_src);
    if ((rc = span_encode_front(c, st_, X, d_rs_rows, rs, &d_pcm))) return rc;
    d_src = d_pcm;
  } else if (X.on()) {   // ... or write it
    d_ext_out = d_dst;
    d_dst = X.d_pcm16;
  }
  rc = span_run_steps(c, enc, S, st_, P, S.h_rows, S.d_rows, S.d_rows + rows, n_lanes, d_src, num_bits, d_dst, nullptr);
  if (!rc && d_ext_out && rs.n)
    rc = launch_span_resample(c, false, st_, d_rs_rows, rs.n, rs.wgs, X, X.d_pcm16, (int16_t*)d_ext_out);
  return span_side_close(c, side, rc);
}

// host-buffer form: PCM rows of rate / 50 samples, and at a rate other than 16000 the 16 kHz workspace lives next to the
// staging buffers
int spans_call_host(lyra_hip_ctx* c, int side, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                    const void* src, int num_bits, void* dst, int rate = 16000) {
  const bool enc = side == sp::SIDE_ENC;
  const char* what = enc ? "encode_spans" : "decode_spans";
  const int rc = span_check_head(c, what, side, &num_bits, rate);
  if (rc) return rc;
  const size_t nbytes = (size_t)(num_bits + 7) / 8, pcm_b = (size_t)rate / 50 * 2;
  SpanBuf B[] = {{SPAN_IN, (void*)src, enc ? pcm_b : nbytes}, {SPAN_OUT, dst, enc ? nbytes : pcm_b},
                 {SPAN_WORK, nullptr, rate != 16000 ? (size_t)640 : 0}};
  return span_staged(c, what, side, spans, n_spans, B, [&] {
    return spans_call_dev(c, side, spans, n_spans, lane_ids, n_lanes, B[0].d, num_bits, B[1].d, SpanExt{rate, (int16_t*)B[2].d});
  });
}

// ---- DTX on spans ---------------------------------------------------------------------------------------------------------
// mel rows and map for `frames` frames, counts for n_rows spans -- the worst case of a call, before anything is enqueued
int span_dtx_ensure(lyra_hip_ctx* c, SpanSide& S, hipStream_t st_, long long frames, int n_rows) {
  if (frames > S.dtx_cap) {
    HIPCHK(c, hipStreamSynchronize(st_));
    dfree(S.d_mel, S.d_map);
    S.dtx_cap = 0;
    if (dalloc(&S.d_mel, (size_t)frames * SPAN_MEL_ROW) != hipSuccess || dalloc(&S.d_map, (size_t)frames) != hipSuccess) {
      dfree(S.d_mel, S.d_map);
      (void)hipGetLastError();
      return fail(c, LYRA_HIP_ENOMEM, "spans: %lld mel rows of scratch failed", frames);
    }
    S.dtx_cap = frames;
  }
  if (n_rows > S.counts_cap) {
    HIPCHK(c, hipStreamSynchronize(st_));
    if (S.h_counts) (void)hipHostFree(S.h_counts);
    S.h_counts = S.d_counts = nullptr;
    S.counts_cap = 0;
    HIPCHK(c, hipHostMalloc((void**)&S.h_counts, (size_t)n_rows * sizeof(int32_t), hipHostMallocDefault));
    HIPCHK(c, hipHostGetDevicePointer((void**)&S.d_counts, S.h_counts, 0));
    S.counts_cap = n_rows;
  }
  return 0;
}

// NoiseEstimator::ReceiveSamples over every frame of the rows' spans on st_: the log-mel pass, then the scan.  side picks the
// region, the filterbank and the constants as launch_noise does.  flag_out[frame] = v_noise / v_active.
// d_rate_rows (a rate per span, encoder side): row i's filterbank and constants are those of d_rate_rows[i]'s rate.
int launch_span_noise(lyra_hip_ctx* c, int side, hipStream_t st_, SpanSide& S, const SpanDtxRow* d_rows, int n_rows, long long wgs,
                      const int16_t* d_pcm16, int32_t* d_flag_out, int v_noise, int v_active, long long* d_map,
                      const SpanRsRow* d_rate_rows = nullptr) {
  uint8_t* region = c->sm.base[side == 0 ? st::R_NOISE_E : st::R_NOISE_D];
  if (d_rate_rows) {
    hipLaunchKernelGGL(span_logmel_rates_kernel, dim3((unsigned)wgs), dim3(256), logmel_lds_bytes(), st_, c->model.d_mel_rate[0],
                       d_rows, d_rate_rows, n_rows, region, d_pcm16, S.d_mel);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(span_noise_scan_rates_kernel, dim3(n_rows), dim3(64), 0, st_, (const NoiseP*)c->d_noise_tab, d_rows,
                       d_rate_rows, n_rows, region, (const float*)S.d_mel, d_flag_out, v_noise, v_active, d_map, S.d_counts);
    HIPCHK(c, hipGetLastError());
    return 0;
  }
  const int rate = side == 0 ? c->enc_noise_rate : 16000;
  const MelP* melp = c->model.d_mel_rate[rate == 8000 ? 0 : rate == 32000 ? 2 : rate == 48000 ? 3 : 1];
  hipLaunchKernelGGL(span_logmel_kernel, dim3((unsigned)wgs), dim3(256), logmel_lds_bytes(), st_, melp, d_rows, n_rows, region,
                     d_pcm16, S.d_mel);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(span_noise_scan_kernel, dim3(n_rows), dim3(64), 0, st_, noise_params(rate), d_rows, n_rows, region,
                     (const float*)S.d_mel, d_flag_out, v_noise, v_active, d_map, S.d_counts);
  HIPCHK(c, hipGetLastError());
  return 0;
}

// The encode calls that report packet_bytes: DTX (lyra_hip_encode_spans_dtx_dev) and per-frame bitrates
// (lyra_hip_encode_spans_mixed_dev, spans_mixed_api.inc), alone or together.
//   dtx         the estimator in front of the steps, the one host wait, the steps on the compacted map; else the steps run on
//               the spans as given and the host does not wait;
//   frame_bits  null: every frame at num_bits.  Else a HOST array [frames], a bit count per frame (num_bits is not read):
//               judged for every span frame before anything is enqueued, uploaded by buffer frame with the rows, and
//               d_packet_bytes is written by the scatter.
//   span_rates  null: every span at sample_rate_hz.  Else a HOST array [n_spans], a rate per span (spans_rates_api.inc;
//               sample_rate_hz is not read): d_pcm_ext rows are MAX_EXT_HOP apart, d_pcm16 is required, and with dtx each span's
//               estimator is that of its own rate, whatever lyra_hip_set_encoder_sample_rate says.
//   ext_base    with span_rates (spans_packed_api.inc): d_pcm_ext is flat, HOST [n_spans] = each span's first sample.
int span_lossy_ensure(lyra_hip_ctx* c, SpanSide& S, hipStream_t st_, size_t list_bytes, size_t snap_floats, int n_ctl);   // spans_lossy_api.inc
int encode_spans_planned_dev(lyra_hip_ctx* c, const char* what, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids,
                             int n_lanes, const int16_t* d_pcm_ext, int sample_rate_hz, int16_t* d_pcm16, int num_bits,
                             const int32_t* frame_bits, bool dtx, uint8_t* d_packets, int32_t* d_packet_bytes,
                             const int32_t* span_rates = nullptr, const long long* ext_base = nullptr) {
  const int rate = span_rates ? 16000 : sample_rate_hz;
  const SpanExt X{rate, span_rates || rate != 16000 ? d_pcm16 : nullptr, span_rates, span_rates ? ext_base : nullptr};
  SpanPlan dry;   // ids, lanes and frame ranges: the planner's rules, on the spans as given
  int rc = span_check(c, what, sp::SIDE_ENC, frame_bits ? nullptr : &num_bits, spans, n_spans, lane_ids, n_lanes, d_pcm_ext,
                      d_packets, X, &dry);
  if (rc) return rc;
  if (!d_packet_bytes) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  for (int s = 0; frame_bits && s < n_spans; ++s)
    for (int64_t f = spans[s].first_frame; f < spans[s].first_frame + spans[s].n_frames; ++f)
      if (frame_bits[f] < 4 || frame_bits[f] > 184 || (frame_bits[f] & 3))
        return fail(c, LYRA_HIP_EINVAL, "%s: num_bits[%lld] = %d is not a multiple of 4 in 4..184", what, (long long)f,
                    frame_bits[f]);
  if (dtx && !span_rates && c->enc_noise_rate != rate)   // as lyra_hip_encode_ext_dev: the DTX estimator is created at the encoder's external rate
    return fail(c, LYRA_HIP_EINVAL, "%s: DTX at %d Hz but the encoder-side noise estimator is set up for %d Hz "
                "(call lyra_hip_set_encoder_sample_rate(%d) first)", what, rate, c->enc_noise_rate, rate);
  const SpanPass rs = X.on() ? span_pass_rows<SpanRsRow>(spans, n_spans, nullptr) : SpanPass();
  const SpanPass dx = dtx ? span_pass_rows<SpanDtxRow>(spans, n_spans, nullptr) : SpanPass();
  if (rs.wgs < 0 || dx.wgs < 0) return fail(c, LYRA_HIP_EINVAL, "%s: too many frames for one pass", what);
  DEVSCOPE(c);
  if (span_rates && (rc = rates_ensure(c))) return rc;
  hipStream_t st_;
  SpanSide& S = span_side_open(c, sp::SIDE_ENC, &st_);
  // all scratch for the worst case -- every frame active: at most one chunk per span and per lane -- before the first launch
  const int rows_max = n_spans + n_lanes;
  if ((rc = span_side_ensure(c, S, st_, rows_max, n_lanes + rs.n + dx.n))) return rc;
  if ((rc = ensure_scratch(c, rows_max))) return rc;
  if (dtx && (rc = span_dtx_ensure(c, S, st_, std::max<long long>(dx.frames, 1), std::max(dx.n, 1)))) return rc;
  const size_t bits_bytes = frame_bits ? (size_t)dry.end_frame * sizeof(int32_t) : 0;
  if (bits_bytes) {
    if ((rc = span_lossy_ensure(c, S, st_, bits_bytes, 0, 0))) return rc;
    if ((rc = err_word_ensure(c, &c->d_mixed_err))) return rc;   // the mixed quantizer's error word (mixed_api.inc)
    for (int s = 0; s < n_spans; ++s)   // frames outside the spans are not read: their entries are never looked at either
      if (spans[s].n_frames)
        std::memcpy(S.h_lists + (size_t)spans[s].first_frame * sizeof(int32_t), frame_bits + spans[s].first_frame,
                    (size_t)spans[s].n_frames * sizeof(int32_t));
  }
  // upload 1, behind the batch rows' place: the lanes' reset rows, the resampler's rows, the estimator's rows
  SpanRow* h_fix = S.h_rows + rows_max;
  for (int l = 0; l < n_lanes; ++l) h_fix[l] = SpanRow{lane_ids[l], 0, 0, -1, 0, 0, 0};
  if (rs.n) span_pass_rows(spans, n_spans, reinterpret_cast<SpanRsRow*>(h_fix + n_lanes), span_rates, X.base);
  if (dx.n) span_pass_rows(spans, n_spans, reinterpret_cast<SpanDtxRow*>(h_fix + n_lanes + rs.n));
  const SpanRow* d_fix = S.d_rows + rows_max;
  const SpanRsRow* d_rs_rows = reinterpret_cast<const SpanRsRow*>(d_fix + n_lanes);
  const SpanDtxRow* d_dx_rows = reinterpret_cast<const SpanDtxRow*>(d_fix + n_lanes + rs.n);
  if ((rc = span_side_begin(c, sp::SIDE_ENC))) return rc;
  if ((rc = span_upload_rows(c, S, st_, rows_max, n_lanes + rs.n + dx.n))) return rc;
  if (bits_bytes) {
    HIPCHK(c, hipMemcpyAsync(S.d_lists, S.h_lists, bits_bytes, hipMemcpyHostToDevice, st_));
    HIPCHK(c, hipEventRecord(S.ev_up, st_));
    S.up_pending = true;
  }
  const int16_t* d_src16 = d_pcm_ext;
  if ((rc = span_encode_front(c, st_, X, d_rs_rows, rs, &d_src16))) return rc;
  SpanPlan P;
  std::vector<lyra_hip_span> compact((size_t)n_spans);
  if (dx.n) {
    // (per-frame bitrates: the scatter stores the size of every frame that has a packet)
    if ((rc = launch_span_noise(c, 0, st_, S, d_dx_rows, dx.n, dx.wgs, d_src16, d_packet_bytes, 0,
                                frame_bits ? (int)MAX_PACKET_BYTES : (num_bits + 7) / 8, S.d_map, span_rates ? d_rs_rows : nullptr)))
      return rc;
    // the one host wait of the call: the plan depends on the decisions
    HIPCHK(c, hipStreamSynchronize(st_));
    S.up_pending = false;
  }
  if (!dtx) {
    std::copy(spans, spans + n_spans, compact.begin());
  } else {   // what the encoder sees of span s: its non-noise hops, at the start of its region of the map
    long long region = 0;
    int r = 0;
    for (int s = 0; s < n_spans; ++s) {
      compact[s] = lyra_hip_span{spans[s].stream_id, region, spans[s].n_frames ? (int64_t)S.h_counts[r++] : 0};
      if (compact[s].n_frames < 0 || compact[s].n_frames > spans[s].n_frames)
        return fail(c, LYRA_HIP_EHIP, "%s: the scan's count of span %d is out of range", what, s);
      region += spans[s].n_frames;
    }
  }
  if ((rc = span_plan_checked(c, sp::SIDE_ENC, compact.data(), n_spans, lane_ids, n_lanes, &P, what))) return rc;
  // upload 2: the batch rows (the pinned rows in front of upload 1's, so neither waits for the other)
  span_fill_rows(P, compact.data(), lane_ids, 0, S.h_rows);
  if ((rc = span_upload_rows(c, S, st_, 0, (int)P.chunks.size()))) return rc;
  const SpanMixed M{reinterpret_cast<const int32_t*>(S.d_lists), d_packet_bytes};
  rc = span_run_steps(c, true, S, st_, P, S.h_rows, S.d_rows, d_fix, n_lanes, d_src16, num_bits, d_packets, dtx ? S.d_map : nullptr,
                      nullptr, frame_bits ? &M : nullptr);
  return span_side_close(c, sp::SIDE_ENC, rc);
}

}  // namespace

extern "C" {

int lyra_hip_span_warmup_frames(int side) { return sp::warmup(side) < 0 ? LYRA_HIP_EINVAL : sp::warmup(side); }

int lyra_hip_spans_plan(int side, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes, int max_streams,
                        lyra_hip_span_chunk* chunks, int cap, int* n_steps) {
  std::vector<sp::Chunk> out;
  const int n = sp::plan(side, reinterpret_cast<const sp::Span*>(spans), n_spans, lane_ids, n_lanes, max_streams, &out, n_steps);
  if (n < 0 || n > cap || (n && !chunks)) return LYRA_HIP_EINVAL;
  if (n) std::memcpy(chunks, out.data(), (size_t)n * sizeof(sp::Chunk));
  return n;
}

int lyra_hip_encode_spans_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                              const int16_t* d_pcm, int num_bits, uint8_t* d_packets) {
  return spans_call_dev(c, sp::SIDE_ENC, spans, n_spans, lane_ids, n_lanes, d_pcm, num_bits, d_packets);
}

int lyra_hip_decode_spans_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                              const uint8_t* d_packets, int num_bits, int16_t* d_pcm) {
  return spans_call_dev(c, sp::SIDE_DEC, spans, n_spans, lane_ids, n_lanes, d_packets, num_bits, d_pcm);
}

int lyra_hip_encode_spans(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                          const int16_t* pcm, int num_bits, uint8_t* packets) {
  return spans_call_host(c, sp::SIDE_ENC, spans, n_spans, lane_ids, n_lanes, pcm, num_bits, packets);
}

int lyra_hip_decode_spans(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                          const uint8_t* packets, int num_bits, int16_t* pcm) {
  return spans_call_host(c, sp::SIDE_DEC, spans, n_spans, lane_ids, n_lanes, packets, num_bits, pcm);
}

int lyra_hip_encode_spans_ext_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                  const int16_t* d_pcm_ext, int sample_rate_hz, int16_t* d_pcm16, int num_bits,
                                  uint8_t* d_packets) {
  return spans_call_dev(c, sp::SIDE_ENC, spans, n_spans, lane_ids, n_lanes, d_pcm_ext, num_bits, d_packets,
                        SpanExt{sample_rate_hz, d_pcm16});
}

int lyra_hip_decode_spans_ext_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                  const uint8_t* d_packets, int num_bits, int sample_rate_hz, int16_t* d_pcm16,
                                  int16_t* d_pcm_ext) {
  return spans_call_dev(c, sp::SIDE_DEC, spans, n_spans, lane_ids, n_lanes, d_packets, num_bits, d_pcm_ext,
                        SpanExt{sample_rate_hz, d_pcm16});
}

int lyra_hip_encode_spans_ext(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                              const int16_t* pcm_ext, int sample_rate_hz, int num_bits, uint8_t* packets) {
  return spans_call_host(c, sp::SIDE_ENC, spans, n_spans, lane_ids, n_lanes, pcm_ext, num_bits, packets, sample_rate_hz);
}

int lyra_hip_decode_spans_ext(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                              const uint8_t* packets, int num_bits, int sample_rate_hz, int16_t* pcm_ext) {
  return spans_call_host(c, sp::SIDE_DEC, spans, n_spans, lane_ids, n_lanes, packets, num_bits, pcm_ext, sample_rate_hz);
}

int lyra_hip_encode_spans_dtx_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                                  const int16_t* d_pcm_ext, int sample_rate_hz, int16_t* d_pcm16, int num_bits,
                                  uint8_t* d_packets, int32_t* d_packet_bytes) {
  return encode_spans_planned_dev(c, "encode_spans_dtx", spans, n_spans, lane_ids, n_lanes, d_pcm_ext, sample_rate_hz, d_pcm16,
                                  num_bits, nullptr, true, d_packets, d_packet_bytes);
}

// host-buffer form: packet rows of noise frames read back as zeros
int lyra_hip_encode_spans_dtx(lyra_hip_ctx* c, const lyra_hip_span* spans, int n_spans, const int32_t* lane_ids, int n_lanes,
                              const int16_t* pcm_ext, int sample_rate_hz, int num_bits, uint8_t* packets, int32_t* packet_bytes) {
  const char* what = "encode_spans_dtx";
  const int rc = span_check_head(c, what, sp::SIDE_ENC, &num_bits, sample_rate_hz);
  if (rc) return rc;
  if (!packet_bytes) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  SpanBuf B[] = {{SPAN_IN, (void*)pcm_ext, (size_t)sample_rate_hz / 50 * 2}, {SPAN_OUT, packets, (size_t)(num_bits + 7) / 8, true},
                 {SPAN_OUT, packet_bytes, sizeof(int32_t)}, {SPAN_WORK, nullptr, sample_rate_hz != 16000 ? (size_t)640 : 0}};
  return span_staged(c, what, sp::SIDE_ENC, spans, n_spans, B, [&] {
    return lyra_hip_encode_spans_dtx_dev(c, spans, n_spans, lane_ids, n_lanes, (const int16_t*)B[0].d, sample_rate_hz,
                                         (int16_t*)B[3].d, num_bits, B[1].d, (int32_t*)B[2].d);
  });
}

int lyra_hip_noise_spans_dev(lyra_hip_ctx* c, int side, const lyra_hip_span* spans, int n_spans, const int16_t* d_pcm16,
                             int32_t* d_is_noise) {
  const char* what = "noise_spans";
  SpanPlan dry;
  int rc = span_check(c, what, side, nullptr, spans, n_spans, nullptr, 0, d_pcm16, d_is_noise, SpanExt(), &dry);
  if (rc) return rc;
  const SpanPass dx = span_pass_rows<SpanDtxRow>(spans, n_spans, nullptr);
  if (dx.wgs < 0) return fail(c, LYRA_HIP_EINVAL, "%s: too many frames for one pass", what);
  if (!dx.n) return 0;
  DEVSCOPE(c);
  hipStream_t st_;
  SpanSide& S = span_side_open(c, side, &st_);
  if ((rc = span_side_ensure(c, S, st_, 1, dx.n))) return rc;
  if ((rc = span_dtx_ensure(c, S, st_, dx.frames, dx.n))) return rc;
  span_pass_rows(spans, n_spans, reinterpret_cast<SpanDtxRow*>(S.h_rows));
  if ((rc = span_side_begin(c, side))) return rc;
  if (side == sp::SIDE_DEC && (rc = wait_noise_stream(c))) return rc;   // the decoder-side slots may have been touched on the noise stream
  if ((rc = span_upload_rows(c, S, st_, 0, dx.n))) return rc;
  rc = launch_span_noise(c, side, st_, S, reinterpret_cast<const SpanDtxRow*>(S.d_rows), dx.n, dx.wgs, d_pcm16, d_is_noise, 1, 0,
                         nullptr);
  return span_side_close(c, side, rc);
}

int lyra_hip_noise_spans(lyra_hip_ctx* c, int side, const lyra_hip_span* spans, int n_spans, const int16_t* pcm16,
                         int32_t* is_noise) {
  const char* what = "noise_spans";
  const int rc = span_check_head(c, what, side, nullptr, 16000);
  if (rc) return rc;
  SpanBuf B[] = {{SPAN_IN, (void*)pcm16, 640}, {SPAN_OUT, is_noise, sizeof(int32_t)}};
  return span_staged(c, what, side, spans, n_spans, B, [&] {
    return lyra_hip_noise_spans_dev(c, side, spans, n_spans, (const int16_t*)B[0].d, (int32_t*)B[1].d);
  });
}

}  // extern "C"
