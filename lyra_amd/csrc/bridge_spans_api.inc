// bridge_spans_api.inc -- part of api.hip, behind the span calls: a recording through the conference bridge in one call
// (include/lyra_hip_bridge_spans.h).
//   lyra_hip_spans_bridge_plan: bridge_spans_plan.h, no context.
//   lyra_hip_spans_bridge_mix_dev: the pass alone (bridge_spans_kernels.hip), a stateless encode-side call on se[0]: one upload of
//     the index over participant numbers, then per slab of ticks the full mix and the zeros of participants in no room, or the
//     three stages of the loudest-N selection.
//   lyra_hip_spans_bridge_dev: decode_spans_lossy_sized_dev (the decode leg, on sd[0]) -> the pass on se[0], behind the event
//     that the decode leg's dec_side_done records -> encode_spans_planned_dev straight from the mix, once per kind of DTX flag.
//     Everything either leg or the pass would refuse is refused here first, so that nothing has run when the call says no; all
//     scratch of the pass is allocated before the decode leg is enqueued.
//   lyra_hip_spans_bridge: span_staged around the `_dev` form.
#include "../../include/lyra_hip_bridge_spans.h"
#include "bridge_spans_kernels.h"
#include "bridge_spans_plan.h"

static_assert(sizeof(lyra_hip_span) == sizeof(bridge_spans::Span) &&
                  offsetof(lyra_hip_span, n_frames) == offsetof(bridge_spans::Span, n_frames),
              "the ABI struct is the planner's");
static_assert(bridge_spans::MAX_FRAMES == INT32_MAX / 2, "the lossy span decode's bound on the frames of a call");

namespace {

constexpr size_t kBspSelCap = (size_t)256 << 20;   // bytes of selection scratch a slab of ticks may take
// wavefronts of one launch: a quarter as many workgroups of 256 threads, 2^31 threads in x -- under the 2^32 - 1 threads a
// launch may be refused above.  Longer calls run as more slabs.
constexpr long long kBspMaxWaves = 1ll << 25;

struct BspState {
  uint8_t* h_idx = nullptr;    // pinned: first [P] int64 | order [P] | room_start [P + 1] | pos_room [P] | part_room [P] | lone [P]
  uint8_t* d_idx = nullptr;
  int idx_cap = 0;             // participants
  hipEvent_t ev_up = nullptr;  // end of the latest upload: h_idx may be rewritten
  bool up_pending = false;
  uint8_t* d_sel = nullptr;    // one slab of the selection: levels [ticks][P] int64 | lists [ticks][n_rooms][8] | keys [ticks][n_members]
  size_t sel_cap = 0;          // bytes
  int32_t* d_cn = nullptr;     // [cn_cap] is_comfort_noise of a call that skips comfort noise but was given no array
  int64_t cn_cap = 0;          // frames
};

size_t bsp_idx_bytes(size_t P) { return P * 8 + (5 * P + 1) * 4; }

void bsp_free(lyra_hip_ctx* c) {
  BspState* S = static_cast<BspState*>(c->bsp);
  if (!S) return;
  if (S->h_idx) (void)hipHostFree(S->h_idx);
  dfree(S->d_idx, S->d_sel, S->d_cn);
  if (S->ev_up) (void)hipEventDestroy(S->ev_up);
  delete S;
  c->bsp = nullptr;
}

// what the pass needs to know of a call, from the host arrays alone
struct BspPlan {
  int P = 0;
  int64_t T = 0;
  int n_rooms = 0, n_members = 0, n_lone = 0;
  bool big = false;            // a room above 64 members: the selection parks its keys
  std::vector<int32_t> order, room_start;
  size_t sel_per_tick(int max_speakers) const {
    return max_speakers ? (size_t)P * 8 + (size_t)n_rooms * LYRA_HIP_SPEAKERS_MAX * 4 + (big ? (size_t)n_members * 8 : 0) : 0;
  }
  // ticks per launch: the launch arithmetic (P is the largest unit count per tick) and, for the selection, the scratch cap
  int64_t slab(int max_speakers) const {
    int64_t n = std::min<int64_t>(std::max<int64_t>(T, 1), kBspMaxWaves / std::max(P, 1));
    if (max_speakers) n = std::min<int64_t>(n, (int64_t)(kBspSelCap / sel_per_tick(max_speakers)));
    return std::max<int64_t>(n, 1);
  }
};

int bsp_plan_checked(lyra_hip_ctx* c, const char* what, const lyra_hip_span* spans, int P, const int32_t* rooms, BspPlan* pl) {
  if (P < 1 || P > c->max_streams) return fail(c, LYRA_HIP_EINVAL, "%s: P %d outside 1..%d", what, P, c->max_streams);
  if (!spans || !rooms) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  pl->P = P;
  pl->order.assign((size_t)P, 0);
  pl->room_start.assign((size_t)P + 1, 0);
  if (bridge_spans::check(reinterpret_cast<const bridge_spans::Span*>(spans), P, &pl->T))
    return fail(c, LYRA_HIP_EINVAL,
                "%s: every span needs the same n_frames, a distinct stream id, and a non-negative frame range that overlaps no "
                "other; at most %lld span frames in all", what, (long long)bridge_spans::MAX_FRAMES);
  for (int p = 0; p < P; ++p)
    if (spans[p].stream_id >= c->max_streams)
      return fail(c, LYRA_HIP_EINVAL, "%s: stream id %d outside 0..%d", what, spans[p].stream_id, c->max_streams - 1);
  if (bridge::plan(rooms, P, pl->order.data(), pl->room_start.data(), &pl->n_rooms, &pl->n_members))
    return fail(c, LYRA_HIP_EINVAL, "%s: a room of more than %d members", what, LYRA_HIP_BRIDGE_MAX_ROOM);
  pl->n_lone = P - pl->n_members;
  for (int r = 0; r < pl->n_rooms; ++r) pl->big = pl->big || pl->room_start[(size_t)r + 1] - pl->room_start[(size_t)r] > 64;
  return 0;
}

// the buffer checks the pass shares with the ticks' mix calls (brg_check_buffers, bridge_api.inc), and its own range of N
int bsp_check_buffers(lyra_hip_ctx* c, const char* what, const int16_t* d_pcm16, const int16_t* d_mix, const int64_t* d_levels,
                      int max_speakers) {
  if (!d_pcm16 || !d_mix) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  if (const int rc = brg_check_buffers(c, what, d_pcm16, d_mix, "d_mix", d_levels)) return rc;
  if (max_speakers < 0 || max_speakers > LYRA_HIP_SPEAKERS_MAX)
    return fail(c, LYRA_HIP_EINVAL, "%s: max_speakers %d outside 0..%d", what, max_speakers, LYRA_HIP_SPEAKERS_MAX);
  return 0;
}

// Everything the pass allocates, before anything is enqueued: it fills nothing.  cn_frames > 0: the call needs comfort-noise
// flags of its own for that many frames.  Growing drains se[0], the only stream the pass's buffers are used on.
int bsp_ensure(lyra_hip_ctx* c, const BspPlan& pl, int max_speakers, int64_t cn_frames) {
  if (!c->bsp) c->bsp = new BspState();
  BspState& S = *static_cast<BspState*>(c->bsp);
  if (!S.ev_up) HIPCHK(c, hipEventCreateWithFlags(&S.ev_up, hipEventDisableTiming));
  const size_t P = (size_t)pl.P;
  if (pl.P > S.idx_cap) {
    HIPCHK(c, hipStreamSynchronize(c->se[0]));
    if (S.h_idx) (void)hipHostFree(S.h_idx);
    S.h_idx = nullptr;
    dfree(S.d_idx);
    S.idx_cap = 0;
    HIPCHK(c, hipHostMalloc((void**)&S.h_idx, bsp_idx_bytes(P), hipHostMallocDefault));
    HIPCHK(c, dalloc(&S.d_idx, bsp_idx_bytes(P)));
    S.idx_cap = pl.P;
  }
  const size_t sel = pl.sel_per_tick(max_speakers) * (size_t)pl.slab(max_speakers);
  if (sel > S.sel_cap) {
    HIPCHK(c, hipStreamSynchronize(c->se[0]));
    dfree(S.d_sel);
    S.sel_cap = 0;
    if (dalloc(&S.d_sel, sel) != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, LYRA_HIP_ENOMEM, "bridge_spans: %zu bytes of selection scratch failed", sel);
    }
    S.sel_cap = sel;
  }
  if (cn_frames > S.cn_cap) {
    const int rc = sync_all(c);   // (written on sd[0], read on se[0])
    if (rc) return rc;
    dfree(S.d_cn);
    S.cn_cap = 0;
    if (dalloc(&S.d_cn, (size_t)cn_frames) != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, LYRA_HIP_ENOMEM, "bridge_spans: comfort-noise flags for %lld frames failed", (long long)cn_frames);
    }
    S.cn_cap = cn_frames;
  }
  return 0;
}

// The index of a call into the pinned staging bsp_ensure sized, in the order of bsp_idx_bytes: called right in front of its
// upload, once the previous call's upload has left the staging.
int bsp_fill_index(lyra_hip_ctx* c, BspState& S, const BspPlan& pl, const lyra_hip_span* spans) {
  if (S.up_pending) {
    HIPCHK(c, hipEventSynchronize(S.ev_up));
    S.up_pending = false;
  }
  const size_t P = (size_t)pl.P;
  long long* first = reinterpret_cast<long long*>(S.h_idx);
  int32_t* order = reinterpret_cast<int32_t*>(S.h_idx + P * 8);
  int32_t *room_start = order + P, *pos_room = room_start + P + 1, *part_room = pos_room + P, *lone = part_room + P;
  for (size_t p = 0; p < P; ++p) {
    first[p] = spans[p].first_frame;
    order[p] = p < (size_t)pl.n_members ? pl.order[p] : 0;
    pos_room[p] = -1;
    part_room[p] = -1;
  }
  for (int r = 0; r <= pl.n_rooms; ++r) room_start[r] = pl.room_start[(size_t)r];
  for (int r = 0; r < pl.n_rooms; ++r)
    for (int i = pl.room_start[(size_t)r]; i < pl.room_start[(size_t)r + 1]; ++i) {
      pos_room[i] = r;
      part_room[pl.order[(size_t)i]] = r;
    }
  int n_lone = 0;
  for (size_t p = 0; p < P; ++p)
    if (part_room[p] < 0) lone[n_lone++] = (int32_t)p;
  return 0;
}

inline unsigned bsp_grid(long long units, long long n_ticks) { return (unsigned)((units * n_ticks + 3) / 4); }

// The pass on se[0], after bsp_ensure: the index of the call and its upload, then slab after slab of ticks.
int bsp_pass_launch(lyra_hip_ctx* c, const BspPlan& pl, const lyra_hip_span* spans, const int16_t* d_pcm16,
                    const int32_t* d_muted, const int32_t* d_is_cn, int max_speakers, int16_t* d_mix, int64_t* d_levels, int32_t* d_is_speaker) {
  if (pl.T == 0) return 0;
  BspState& S = *static_cast<BspState*>(c->bsp);
  hipStream_t st_ = c->se[0];
  const size_t P = (size_t)pl.P;
  const int rc = bsp_fill_index(c, S, pl, spans);
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(S.d_idx, S.h_idx, bsp_idx_bytes(P), hipMemcpyHostToDevice, st_));
  HIPCHK(c, hipEventRecord(S.ev_up, st_));
  S.up_pending = true;
  const long long* first = reinterpret_cast<const long long*>(S.d_idx);
  const int32_t* order = reinterpret_cast<const int32_t*>(S.d_idx + P * 8);
  const int32_t *room_start = order + P, *pos_room = room_start + P + 1, *part_room = pos_room + P, *lone = part_room + P;
  const int64_t slab = pl.slab(max_speakers);
  for (int64_t t0 = 0; t0 < pl.T; t0 += slab) {
    const int n = (int)std::min<int64_t>(slab, pl.T - t0);
    if (!max_speakers) {
      if (pl.n_rooms) {
        hipLaunchKernelGGL(bridge_spans_mix_kernel, dim3(bsp_grid(pl.n_rooms, n)), dim3(256), 0, st_, d_pcm16, first, order,
                           room_start, pl.n_rooms, (long long)t0, n, d_muted, d_is_cn, d_mix);
        HIPCHK(c, hipGetLastError());
      }
      if (pl.n_lone) {
        hipLaunchKernelGGL(bridge_spans_zero_kernel, dim3(bsp_grid(pl.n_lone, n)), dim3(256), 0, st_, first, lone, pl.n_lone,
                           (long long)t0, n, d_mix);
        HIPCHK(c, hipGetLastError());
      }
      continue;
    }
    long long* lv = reinterpret_cast<long long*>(S.d_sel);
    int32_t* spk = reinterpret_cast<int32_t*>(S.d_sel + (size_t)slab * P * 8);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(S.d_sel + (size_t)slab * (P * 8 + (size_t)pl.n_rooms * LYRA_HIP_SPEAKERS_MAX * 4));
    hipLaunchKernelGGL(bridge_spans_level_kernel, dim3(bsp_grid(pl.P, n)), dim3(256), 0, st_, d_pcm16, first, part_room, pl.P,
                       (long long)t0, n, lv, reinterpret_cast<long long*>(d_levels), d_mix, d_is_speaker);
    HIPCHK(c, hipGetLastError());
    if (!pl.n_rooms) continue;
    hipLaunchKernelGGL(bridge_spans_select_kernel, dim3(bsp_grid(pl.n_rooms, n)), dim3(256), 0, st_, (const long long*)lv, first,
                       order, room_start, pl.n_rooms, pl.n_members, pl.P, (long long)t0, n, d_muted, d_is_cn, max_speakers, keys, spk,
                       d_is_speaker);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(bridge_spans_speakers_mix_kernel, dim3(bsp_grid(cdiv(pl.n_members, 8), n)), dim3(256), 0, st_, d_pcm16,
                       first, order, pl.n_members, pos_room, pl.n_rooms, (long long)t0, n, (const int32_t*)spk, d_mix);
    HIPCHK(c, hipGetLastError());
  }
  return 0;
}

int bridge_spans_dev_impl(lyra_hip_ctx* c, const lyra_hip_spans_bridge_call* A) {
  const char* what = "bridge_spans";
  BspPlan pl;
  int rc = bsp_plan_checked(c, what, A->spans, A->P, A->rooms, &pl);
  if (rc) return rc;
  const int P = A->P;
  if (A->n_lanes < 0 || (A->n_lanes && !A->lane_ids)) return fail(c, LYRA_HIP_EINVAL, "%s: bad lane list", what);
  if (!A->d_packets || !A->packet_bytes || !A->num_bits || !A->d_out_packets || !A->d_out_packet_bytes)
    return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  if (A->flags & ~LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE) return fail(c, LYRA_HIP_EINVAL, "%s: unknown flags 0x%x", what, A->flags);
  if ((rc = bsp_check_buffers(c, what, A->d_pcm16, A->d_mix, A->d_levels, A->max_speakers))) return rc;
  // the planner's rules on ids and lanes, for both legs (the encode leg runs on subsets of the spans, which say less)
  for (int side = 0; side < 2; ++side) {
    SpanPlan dry;
    if ((rc = span_plan_checked(c, side, A->spans, P, A->lane_ids, A->n_lanes, &dry, what))) return rc;
  }
  bool any_dtx = false, any_plain = false;
  for (int p = 0; p < P; ++p) (A->dtx && A->dtx[p] ? any_dtx : any_plain) = true;
  if (any_dtx && c->enc_noise_rate != 16000)
    return fail(c, LYRA_HIP_EINVAL, "%s: DTX needs the encoder-side noise estimator at 16000 Hz, it is set up for %d Hz "
                "(call lyra_hip_set_encoder_sample_rate(16000) first)", what, c->enc_noise_rate);
  for (int p = 0; p < P; ++p)
    for (int64_t f = A->spans[p].first_frame; f < A->spans[p].first_frame + pl.T; ++f) {
      const int pb = A->packet_bytes[f], nb = A->num_bits[f];
      if (pb != 0 && !mixed_received(pb))
        return fail(c, LYRA_HIP_EINVAL, "%s: packet_bytes[%lld] = %d is neither 0 nor 8, 15 or %d", what, (long long)f, pb,
                    (int)MAX_PACKET_BYTES);
      if (nb < 4 || nb > 184 || (nb & 3))
        return fail(c, LYRA_HIP_EINVAL, "%s: num_bits[%lld] = %d is not a multiple of 4 in 4..184", what, (long long)f, nb);
    }
  const bool skip_cn = (A->flags & LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE) != 0;
  const int64_t end = span_end_frame(A->spans, P);
  {
    DEVSCOPE(c);
    if ((rc = bsp_ensure(c, pl, A->max_speakers, skip_cn && !A->d_is_comfort_noise ? std::max<int64_t>(end, 1) : 0)))
      return rc;
  }
  BspState& S = *static_cast<BspState*>(c->bsp);
  int32_t* is_cn = A->d_is_comfort_noise ? A->d_is_comfort_noise : skip_cn ? S.d_cn : nullptr;
  // ---- decode leg: lyra_hip_decode_spans_lossy_mixed_dev at 16 kHz ----
  if ((rc = decode_spans_lossy_sized_dev(c, what, A->spans, P, A->lane_ids, A->n_lanes, A->d_packets, A->packet_bytes, 0, true, 16000,
                                         A->d_pcm16, nullptr, A->d_is_noise, is_cn)))
    return rc;
  // ---- the edge and the pass: se[0] behind the decode leg's end ----
  {
    DEVSCOPE(c);
    if ((rc = enc_side_begin(c, 0))) return rc;
    HIPCHK(c, hipStreamWaitEvent(c->se[0], c->ev_dec[(c->n_dec_calls - 1) & 1][0], 0));
    rc = bsp_pass_launch(c, pl, A->spans, A->d_pcm16, A->d_muted, skip_cn ? is_cn : nullptr, A->max_speakers, A->d_mix, A->d_levels,
                         A->d_is_speaker);
    if (!rc) rc = enc_side_done(c, 0);
    if (rc) return rc;
  }
  // ---- encode leg: lyra_hip_encode_spans_mixed_dev at 16000 on the mix, the DTX participants' pass and then the others' ----
  std::vector<lyra_hip_span> part;
  for (int kind = 1; kind >= 0; --kind) {
    if (!(kind ? any_dtx : any_plain)) continue;
    part.clear();
    for (int p = 0; p < P; ++p)
      if ((A->dtx && A->dtx[p] != 0) == (kind != 0)) part.push_back(A->spans[p]);
    if ((rc = encode_spans_planned_dev(c, what, part.data(), (int)part.size(), A->lane_ids, A->n_lanes, A->d_mix, 16000, nullptr, 0,
                                       A->num_bits, kind != 0, A->d_out_packets, A->d_out_packet_bytes)))
      return rc;
  }
  return 0;
}

}  // namespace

extern "C" {

int lyra_hip_spans_bridge_plan(const lyra_hip_span* spans, int P, const int32_t* rooms, int32_t* order, int32_t* room_start,
                               int* n_rooms, int* n_members, int64_t* n_ticks) {
  return bridge_spans::plan(reinterpret_cast<const bridge_spans::Span*>(spans), P, rooms, order, room_start, n_rooms, n_members,
                            n_ticks)
             ? LYRA_HIP_EINVAL
             : 0;
}

int lyra_hip_spans_bridge_mix_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int P, const int32_t* rooms, const int16_t* d_pcm16,
                                  const int32_t* d_muted, const int32_t* d_is_comfort_noise, int max_speakers, int16_t* d_mix,
                                  int64_t* d_levels, int32_t* d_is_speaker) {
  if (!c) return LYRA_HIP_EINVAL;
  const char* what = "bridge_spans_mix";
  BspPlan pl;
  int rc = bsp_plan_checked(c, what, spans, P, rooms, &pl);
  if (rc) return rc;
  if ((rc = bsp_check_buffers(c, what, d_pcm16, d_mix, d_levels, max_speakers))) return rc;
  DEVSCOPE(c);
  if ((rc = bsp_ensure(c, pl, max_speakers, 0))) return rc;
  if ((rc = enc_side_begin(c, 0))) return rc;
  rc = bsp_pass_launch(c, pl, spans, d_pcm16, d_muted, d_is_comfort_noise, max_speakers, d_mix, d_levels, d_is_speaker);
  if (!rc) rc = enc_side_done(c, 0);
  return rc;
}

int lyra_hip_spans_bridge_dev(lyra_hip_ctx* c, const lyra_hip_spans_bridge_call* call) {
  if (!c) return LYRA_HIP_EINVAL;
  if (!call) return fail(c, LYRA_HIP_EINVAL, "bridge_spans: null pointer");
  return bridge_spans_dev_impl(c, call);
}

// host-buffer form: bytes past a packet's size, and the rows of DTX noise frames, read back as zeros
int lyra_hip_spans_bridge(lyra_hip_ctx* c, const lyra_hip_span* spans, int P, const int32_t* lane_ids, int n_lanes,
                          const int32_t* rooms, const uint8_t* packets, const int32_t* packet_bytes, const int32_t* muted,
                          unsigned flags, const int32_t* num_bits, const int32_t* dtx, int max_speakers, uint8_t* out_packets,
                          int32_t* out_packet_bytes, int16_t* pcm16, int16_t* mix, int32_t* is_noise, int32_t* is_comfort_noise,
                          int64_t* levels, int32_t* is_speaker) {
  if (!c) return LYRA_HIP_EINVAL;
  const char* what = "bridge_spans";
  BspPlan pl;   // (the staging is sized by the spans: judge them first)
  const int rc = bsp_plan_checked(c, what, spans, P, rooms, &pl);
  if (rc) return rc;
  if (!packets || !packet_bytes || !num_bits || !out_packets || !out_packet_bytes)
    return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  auto opt = [](void* host, size_t bytes) { return SpanBuf{host ? SPAN_OUT : SPAN_WORK, host, host ? bytes : 0}; };
  auto work = [](void* host, size_t bytes) { return SpanBuf{host ? SPAN_OUT : SPAN_WORK, host, bytes}; };
  const bool sel = max_speakers != 0;
  SpanBuf B[] = {{SPAN_IN, (void*)packets, (size_t)MAX_PACKET_BYTES},
                 muted ? SpanBuf{SPAN_IN, (void*)muted, sizeof(int32_t)} : SpanBuf{SPAN_WORK, nullptr, 0},
                 {SPAN_OUT, out_packets, (size_t)MAX_PACKET_BYTES, true},
                 {SPAN_OUT, out_packet_bytes, sizeof(int32_t)},
                 work(pcm16, 640),
                 work(mix, 640),
                 opt(is_noise, sizeof(int32_t)),
                 opt(is_comfort_noise, sizeof(int32_t)),
                 opt(sel ? levels : nullptr, sizeof(int64_t)),
                 opt(sel ? is_speaker : nullptr, sizeof(int32_t))};
  return span_staged(c, what, sp::SIDE_ENC, spans, P, B, [&] {
    lyra_hip_spans_bridge_call A = {};
    A.spans = spans;
    A.P = P;
    A.lane_ids = lane_ids;
    A.n_lanes = n_lanes;
    A.rooms = rooms;
    A.d_packets = B[0].d;
    A.packet_bytes = packet_bytes;
    A.d_muted = (const int32_t*)B[1].d;
    A.flags = flags;
    A.num_bits = num_bits;
    A.dtx = dtx;
    A.d_out_packets = B[2].d;
    A.d_out_packet_bytes = (int32_t*)B[3].d;
    A.d_pcm16 = (int16_t*)B[4].d;
    A.d_mix = (int16_t*)B[5].d;
    A.d_is_noise = (int32_t*)B[6].d;
    A.d_is_comfort_noise = (int32_t*)B[7].d;
    A.max_speakers = max_speakers;
    A.d_levels = (int64_t*)B[8].d;
    A.d_is_speaker = (int32_t*)B[9].d;
    return bridge_spans_dev_impl(c, &A);
  });
}

}  // extern "C"
