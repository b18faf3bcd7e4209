// meeting_api.inc -- part of api.hip, behind bridge_spans_api.inc: a recorded meeting with a schedule through the conference
// bridge in one call (include/lyra_hip_spans_meeting.h).
//   lyra_hip_spans_meeting_plan: meeting_plan.h, no context.
//   lyra_hip_spans_meeting_mix_dev: the pass alone (meeting_kernels.hip), a stateless encode-side call on se[0]: the epoch
//     table of the schedule is cut into pieces that fit a launch, the pieces into slabs; one upload of table and index, then
//     per slab the full mix and the zeros of participants in no room, or the three stages of the loudest-N selection -- one
//     launch each, however many epochs the slab holds.
//   lyra_hip_spans_meeting_dev: decode_spans_lossy_sized_dev over the participants with frames (the decode leg, on sd[0]) ->
//     the pass on se[0], behind the event that the decode leg's dec_side_done records -> encode_spans_planned_dev straight
//     from the mix, once per kind of DTX flag.  Everything either leg or the pass would refuse is refused here first; all
//     scratch of the pass is allocated before the decode leg is enqueued.
//   lyra_hip_spans_meeting: span_staged around the `_dev` form.
#include "../../include/lyra_hip_spans_meeting.h"
#include "meeting_kernels.h"
#include "meeting_plan.h"

static_assert(sizeof(lyra_hip_span) == sizeof(meeting::Span) && offsetof(lyra_hip_span, n_frames) == offsetof(meeting::Span, n_frames),
              "the ABI struct is the planner's");
static_assert(sizeof(lyra_hip_meeting_stay) == sizeof(meeting::Stay) &&
                  offsetof(lyra_hip_meeting_stay, room) == offsetof(meeting::Stay, room) &&
                  offsetof(lyra_hip_meeting_stay, first_tick) == offsetof(meeting::Stay, first_tick) &&
                  offsetof(lyra_hip_meeting_stay, n_ticks) == offsetof(meeting::Stay, n_ticks),
              "the ABI struct is the planner's");
static_assert(meeting::MAX_ENTRIES == LYRA_HIP_MEETING_MAX_ENTRIES && meeting::MAX_FRAMES == bridge_spans::MAX_FRAMES, "one bound each");
static_assert(sizeof(MeetEpoch) == 80, "the table row the header's index bytes are counted with");

namespace {

struct MeetState {
  uint8_t* h_idx = nullptr;    // pinned: table [pieces + 1] | base [entries] int64 | room [entries, even] | room_start
  uint8_t* d_idx = nullptr;
  size_t idx_cap = 0;          // bytes
  hipEvent_t ev_up = nullptr;  // end of the latest upload: h_idx may be rewritten
  bool up_pending = false;
  uint8_t* d_sel = nullptr;    // one slab of the selection
  size_t sel_cap = 0;          // bytes
  int32_t* d_cn = nullptr;     // [cn_cap] is_comfort_noise of a call that skips comfort noise but was given no array
  int64_t cn_cap = 0;          // frames
};

void meet_free(lyra_hip_ctx* c) {
  MeetState* S = static_cast<MeetState*>(c->meet);
  if (!S) return;
  if (S->h_idx) (void)hipHostFree(S->h_idx);
  dfree(S->d_idx, S->d_sel, S->d_cn);
  if (S->ev_up) (void)hipEventDestroy(S->ev_up);
  delete S;
  c->meet = nullptr;
}

// what the pass needs to know of a call, from the host arrays alone
struct MeetPass {
  meeting::Plan pl;
  std::vector<MeetEpoch> tab;     // the pieces and one row behind them that holds the totals
  std::vector<int> slab;          // slab s is pieces slab[s] .. slab[s + 1] - 1
  size_t sel_bytes = 0;           // of the largest slab
  std::vector<lyra_hip_span> with_frames;   // the participants either leg sees
  size_t n_entries() const { return (size_t)pl.n_entries(); }
  size_t off_base() const { return tab.size() * sizeof(MeetEpoch); }
  size_t off_room() const { return off_base() + n_entries() * 8; }
  size_t off_room_start() const { return off_room() + ((n_entries() + 1) & ~(size_t)1) * 4; }
  size_t idx_bytes() const { return off_room_start() + pl.room_start.size() * 4; }
};

// The epochs as pieces that fit a launch (2^25 wavefronts in the largest count, the entries') and, with a selection, the
// scratch cap; the pieces as slabs under the same two bounds.  Epochs in which nobody is present make no piece.
void meet_cut(MeetPass* mp, int max_speakers) {
  const meeting::Plan& pl = mp->pl;
  MeetEpoch run = {};              // the prefix sums so far
  long long slab_waves = 0;
  size_t slab_sel = 0;
  mp->slab.assign(1, 0);
  for (int64_t e = 0; e < pl.n_epochs(); ++e) {
    const long long n_entries = pl.epoch_entry[(size_t)e + 1] - pl.epoch_entry[(size_t)e];
    if (!n_entries) continue;
    const int n_rooms = pl.n_rooms(e), n_members = pl.epoch_members[(size_t)e];
    const bool big = pl.epoch_big[(size_t)e] != 0;
    const size_t per_tick = max_speakers ? (size_t)n_entries * 8 + (size_t)n_rooms * LYRA_HIP_SPEAKERS_MAX * 4 + (big ? (size_t)n_members * 8 : 0) : 0;
    long long most = kBspMaxWaves / n_entries;
    if (per_tick) most = std::min<long long>(most, (long long)(kBspSelCap / per_tick));
    most = std::max<long long>(most, 1);
    for (long long t = pl.epoch_tick[(size_t)e]; t < pl.epoch_tick[(size_t)e + 1]; t += most) {
      const long long n = std::min<long long>(most, pl.epoch_tick[(size_t)e + 1] - t);
      if (slab_waves + n * n_entries > kBspMaxWaves || slab_sel + (size_t)n * per_tick > kBspSelCap) {
        mp->slab.push_back((int)mp->tab.size());
        slab_waves = 0;
        slab_sel = 0;
      }
      MeetEpoch E = run;
      E.tick0 = t;
      E.sel = (long long)slab_sel;
      E.n_ticks = (int)n;
      E.entry0 = (int)pl.epoch_entry[(size_t)e];
      E.n_entries = (int)n_entries;
      E.n_members = n_members;
      E.room0 = (int)pl.epoch_room[(size_t)e];
      E.n_rooms = n_rooms;
      E.big = big;
      mp->tab.push_back(E);
      run.wave0[MEET_ROOMS] += n * n_rooms;
      run.wave0[MEET_LONE] += n * (n_entries - n_members);
      run.wave0[MEET_ENTRIES] += n * n_entries;
      run.wave0[MEET_CHUNKS] += n * cdiv(n_members, 8);
      slab_waves += n * n_entries;
      slab_sel += (size_t)n * per_tick;
      mp->sel_bytes = std::max(mp->sel_bytes, slab_sel);
    }
  }
  mp->slab.push_back((int)mp->tab.size());
  MeetEpoch end = run;
  end.tick0 = pl.n_ticks;
  mp->tab.push_back(end);
}

int meet_plan_checked(lyra_hip_ctx* c, const char* what, const lyra_hip_span* spans, int P, const lyra_hip_meeting_stay* stays,
                      int n_stays, int max_speakers, MeetPass* mp) {
  if (P < 1 || P > c->max_streams) return fail(c, LYRA_HIP_EINVAL, "%s: P %d outside 1..%d", what, P, c->max_streams);
  if (!spans || n_stays < 0 || (n_stays && !stays)) return fail(c, LYRA_HIP_EINVAL, "%s: null pointer or a negative count", what);
  if (meeting::plan(reinterpret_cast<const meeting::Span*>(spans), P, reinterpret_cast<const meeting::Stay*>(stays), n_stays, &mp->pl))
    return fail(c, LYRA_HIP_EINVAL,
                "%s: every span needs a distinct stream id and a non-negative frame range that overlaps no other, at most %lld "
                "span frames in all; stays sorted by (participant, first_tick), not overlapping, n_ticks >= 1, their sum the "
                "span's n_frames; at most %d entries; no room of more than %d members", what, (long long)meeting::MAX_FRAMES,
                LYRA_HIP_MEETING_MAX_ENTRIES, LYRA_HIP_BRIDGE_MAX_ROOM);
  for (int p = 0; p < P; ++p) {
    if (spans[p].stream_id >= c->max_streams)
      return fail(c, LYRA_HIP_EINVAL, "%s: stream id %d outside 0..%d", what, spans[p].stream_id, c->max_streams - 1);
    if (spans[p].n_frames) mp->with_frames.push_back(spans[p]);
  }
  meet_cut(mp, max_speakers < 0 || max_speakers > LYRA_HIP_SPEAKERS_MAX ? 0 : max_speakers);
  return 0;
}

// Everything the pass allocates, before anything is enqueued: it fills nothing.  Growing drains se[0], the only stream the
// pass's buffers are used on (the comfort-noise flags are written on sd[0]: every stream then).
int meet_ensure(lyra_hip_ctx* c, const MeetPass& mp, int64_t cn_frames) {
  if (!c->meet) c->meet = new MeetState();
  MeetState& S = *static_cast<MeetState*>(c->meet);
  if (!S.ev_up) HIPCHK(c, hipEventCreateWithFlags(&S.ev_up, hipEventDisableTiming));
  const size_t idx = mp.idx_bytes();
  if (idx > S.idx_cap) {
    HIPCHK(c, hipStreamSynchronize(c->se[0]));
    if (S.h_idx) (void)hipHostFree(S.h_idx);
    S.h_idx = nullptr;
    dfree(S.d_idx);
    S.idx_cap = 0;
    S.up_pending = false;
    if (hipHostMalloc((void**)&S.h_idx, idx, hipHostMallocDefault) != hipSuccess || dalloc(&S.d_idx, idx) != hipSuccess) {
      (void)hipGetLastError();
      if (S.h_idx) (void)hipHostFree(S.h_idx);
      S.h_idx = nullptr;
      dfree(S.d_idx);
      return fail(c, LYRA_HIP_ENOMEM, "meeting: %zu bytes of index failed", idx);
    }
    S.idx_cap = idx;
  }
  if (mp.sel_bytes > S.sel_cap) {
    HIPCHK(c, hipStreamSynchronize(c->se[0]));
    dfree(S.d_sel);
    S.sel_cap = 0;
    if (dalloc(&S.d_sel, mp.sel_bytes) != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, LYRA_HIP_ENOMEM, "meeting: %zu bytes of selection scratch failed", mp.sel_bytes);
    }
    S.sel_cap = mp.sel_bytes;
  }
  if (cn_frames > S.cn_cap) {
    const int rc = sync_all(c);
    if (rc) return rc;
    dfree(S.d_cn);
    S.cn_cap = 0;
    if (dalloc(&S.d_cn, (size_t)cn_frames) != hipSuccess) {
      (void)hipGetLastError();
      return fail(c, LYRA_HIP_ENOMEM, "meeting: comfort-noise flags for %lld frames failed", (long long)cn_frames);
    }
    S.cn_cap = cn_frames;
  }
  return 0;
}

inline unsigned meet_grid(long long waves) { return (unsigned)((waves + 3) / 4); }

// The pass on se[0], after meet_ensure: the table and index of the call and their upload, then slab after slab.
int meet_pass_launch(lyra_hip_ctx* c, const MeetPass& mp, const int16_t* d_pcm16, const int32_t* d_muted, const int32_t* d_is_cn,
                     int max_speakers, int16_t* d_mix, int64_t* d_levels, int32_t* d_is_speaker) {
  if (mp.tab.size() < 2) return 0;   // nobody is ever present
  MeetState& S = *static_cast<MeetState*>(c->meet);
  hipStream_t st_ = c->se[0];
  if (S.up_pending) {
    HIPCHK(c, hipEventSynchronize(S.ev_up));
    S.up_pending = false;
  }
  const meeting::Plan& pl = mp.pl;
  memcpy(S.h_idx, mp.tab.data(), mp.tab.size() * sizeof(MeetEpoch));
  memcpy(S.h_idx + mp.off_base(), pl.entry_base.data(), mp.n_entries() * 8);
  memcpy(S.h_idx + mp.off_room(), pl.entry_room.data(), mp.n_entries() * 4);
  memcpy(S.h_idx + mp.off_room_start(), pl.room_start.data(), pl.room_start.size() * 4);
  HIPCHK(c, hipMemcpyAsync(S.d_idx, S.h_idx, mp.idx_bytes(), hipMemcpyHostToDevice, st_));
  HIPCHK(c, hipEventRecord(S.ev_up, st_));
  S.up_pending = true;
  const MeetEpoch* tab = reinterpret_cast<const MeetEpoch*>(S.d_idx);
  const long long* base = reinterpret_cast<const long long*>(S.d_idx + mp.off_base());
  const int32_t* room = reinterpret_cast<const int32_t*>(S.d_idx + mp.off_room());
  const int32_t* room_start = reinterpret_cast<const int32_t*>(S.d_idx + mp.off_room_start());
  for (size_t s = 0; s + 1 < mp.slab.size(); ++s) {
    const int lo = mp.slab[s], hi = mp.slab[s + 1];
    if (hi <= lo) continue;
    long long n[4];
    for (int k = 0; k < 4; ++k) n[k] = mp.tab[(size_t)hi].wave0[k] - mp.tab[(size_t)lo].wave0[k];
    if (!max_speakers) {
      if (n[MEET_ROOMS]) {
        hipLaunchKernelGGL(meeting_mix_kernel, dim3(meet_grid(n[MEET_ROOMS])), dim3(256), 0, st_, tab, lo, hi, n[MEET_ROOMS], d_pcm16,
                           base, room_start, d_muted, d_is_cn, d_mix);
        HIPCHK(c, hipGetLastError());
      }
      if (n[MEET_LONE]) {
        hipLaunchKernelGGL(meeting_zero_kernel, dim3(meet_grid(n[MEET_LONE])), dim3(256), 0, st_, tab, lo, hi, n[MEET_LONE], base,
                           d_mix);
        HIPCHK(c, hipGetLastError());
      }
      continue;
    }
    hipLaunchKernelGGL(meeting_level_kernel, dim3(meet_grid(n[MEET_ENTRIES])), dim3(256), 0, st_, tab, lo, hi, n[MEET_ENTRIES], d_pcm16,
                       base, room, S.d_sel, reinterpret_cast<long long*>(d_levels), d_mix, d_is_speaker);
    HIPCHK(c, hipGetLastError());
    if (!n[MEET_ROOMS]) continue;
    hipLaunchKernelGGL(meeting_select_kernel, dim3(meet_grid(n[MEET_ROOMS])), dim3(256), 0, st_, tab, lo, hi, n[MEET_ROOMS], base,
                       room_start, d_muted, d_is_cn, max_speakers, S.d_sel, d_is_speaker);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(meeting_speakers_mix_kernel, dim3(meet_grid(n[MEET_CHUNKS])), dim3(256), 0, st_, tab, lo, hi, n[MEET_CHUNKS],
                       d_pcm16, base, room, (const unsigned char*)S.d_sel, d_mix);
    HIPCHK(c, hipGetLastError());
  }
  return 0;
}

int meeting_dev_impl(lyra_hip_ctx* c, const lyra_hip_spans_meeting_call* A) {
  const char* what = "meeting";
  MeetPass mp;
  int rc = meet_plan_checked(c, what, A->spans, A->P, A->stays, A->n_stays, A->max_speakers, &mp);
  if (rc) return rc;
  const int P = A->P;
  if (A->n_lanes < 0 || (A->n_lanes && !A->lane_ids)) return fail(c, LYRA_HIP_EINVAL, "%s: bad lane list", what);
  if (!A->d_packets || !A->packet_bytes || !A->num_bits || !A->d_out_packets || !A->d_out_packet_bytes)
    return fail(c, LYRA_HIP_EINVAL, "%s: null pointer", what);
  if (A->flags & ~LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE) return fail(c, LYRA_HIP_EINVAL, "%s: unknown flags 0x%x", what, A->flags);
  if ((rc = bsp_check_buffers(c, what, A->d_pcm16, A->d_mix, A->d_levels, A->max_speakers))) return rc;
  const std::vector<lyra_hip_span>& live = mp.with_frames;
  // the planner's rules on ids and lanes, for both legs (the encode leg runs on subsets of the spans, which say less)
  for (int side = 0; side < 2 && !live.empty(); ++side) {
    SpanPlan dry;
    if ((rc = span_plan_checked(c, side, live.data(), (int)live.size(), A->lane_ids, A->n_lanes, &dry, what))) return rc;
  }
  bool any_dtx = false, any_plain = false;
  for (int p = 0; p < P; ++p)
    if (A->spans[p].n_frames) (A->dtx && A->dtx[p] ? any_dtx : any_plain) = true;
  if (any_dtx && c->enc_noise_rate != 16000)
    return fail(c, LYRA_HIP_EINVAL, "%s: DTX needs the encoder-side noise estimator at 16000 Hz, it is set up for %d Hz "
                "(call lyra_hip_set_encoder_sample_rate(16000) first)", what, c->enc_noise_rate);
  for (const lyra_hip_span& s : live)
    for (int64_t f = s.first_frame; f < s.first_frame + s.n_frames; ++f) {
      const int pb = A->packet_bytes[f], nb = A->num_bits[f];
      if (pb != 0 && !mixed_received(pb))
        return fail(c, LYRA_HIP_EINVAL, "%s: packet_bytes[%lld] = %d is neither 0 nor 8, 15 or %d", what, (long long)f, pb,
                    (int)MAX_PACKET_BYTES);
      if (nb < 4 || nb > 184 || (nb & 3))
        return fail(c, LYRA_HIP_EINVAL, "%s: num_bits[%lld] = %d is not a multiple of 4 in 4..184", what, (long long)f, nb);
    }
  if (live.empty()) return 0;   // nobody is ever present: nothing to enqueue
  const bool skip_cn = (A->flags & LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE) != 0;
  const int64_t end = span_end_frame(live.data(), (int)live.size());
  {
    DEVSCOPE(c);
    if ((rc = meet_ensure(c, mp, skip_cn && !A->d_is_comfort_noise ? std::max<int64_t>(end, 1) : 0))) return rc;
  }
  MeetState& S = *static_cast<MeetState*>(c->meet);
  int32_t* is_cn = A->d_is_comfort_noise ? A->d_is_comfort_noise : skip_cn ? S.d_cn : nullptr;
  // ---- decode leg: lyra_hip_decode_spans_lossy_mixed_dev at 16 kHz ----
  if ((rc = decode_spans_lossy_sized_dev(c, what, live.data(), (int)live.size(), A->lane_ids, A->n_lanes, A->d_packets, A->packet_bytes,
                                         0, true, 16000, A->d_pcm16, nullptr, A->d_is_noise, is_cn)))
    return rc;
  // ---- the edge and the pass: se[0] behind the decode leg's end ----
  {
    DEVSCOPE(c);
    if ((rc = enc_side_begin(c, 0))) return rc;
    HIPCHK(c, hipStreamWaitEvent(c->se[0], c->ev_dec[(c->n_dec_calls - 1) & 1][0], 0));
    rc = meet_pass_launch(c, mp, A->d_pcm16, A->d_muted, skip_cn ? is_cn : nullptr, A->max_speakers, A->d_mix, A->d_levels,
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
      if (A->spans[p].n_frames && (A->dtx && A->dtx[p] != 0) == (kind != 0)) part.push_back(A->spans[p]);
    if ((rc = encode_spans_planned_dev(c, what, part.data(), (int)part.size(), A->lane_ids, A->n_lanes, A->d_mix, 16000, nullptr, 0,
                                       A->num_bits, kind != 0, A->d_out_packets, A->d_out_packet_bytes)))
      return rc;
  }
  return 0;
}

}  // namespace

extern "C" {

int lyra_hip_spans_meeting_plan(const lyra_hip_span* spans, int P, const lyra_hip_meeting_stay* stays, int n_stays, int64_t* n_epochs,
                                int64_t* n_entries, int64_t* n_ticks, int64_t* epoch_tick, int64_t* epoch_entry,
                                int32_t* entry_participant, int32_t* entry_room) {
  if (!n_epochs || !n_entries || !n_ticks) return LYRA_HIP_EINVAL;
  meeting::Plan pl;
  if (meeting::plan(reinterpret_cast<const meeting::Span*>(spans), P, reinterpret_cast<const meeting::Stay*>(stays), n_stays, &pl))
    return LYRA_HIP_EINVAL;
  *n_epochs = pl.n_epochs();
  *n_entries = pl.n_entries();
  *n_ticks = pl.n_ticks;
  if (epoch_tick) std::copy(pl.epoch_tick.begin(), pl.epoch_tick.end(), epoch_tick);
  if (epoch_entry) std::copy(pl.epoch_entry.begin(), pl.epoch_entry.end(), epoch_entry);
  if (entry_participant) std::copy(pl.entry_participant.begin(), pl.entry_participant.end(), entry_participant);
  if (entry_room) std::copy(pl.entry_room.begin(), pl.entry_room.end(), entry_room);
  return 0;
}

int lyra_hip_spans_meeting_mix_dev(lyra_hip_ctx* c, const lyra_hip_span* spans, int P, const lyra_hip_meeting_stay* stays, int n_stays,
                                   const int16_t* d_pcm16, const int32_t* d_muted, const int32_t* d_is_comfort_noise, int max_speakers,
                                   int16_t* d_mix, int64_t* d_levels, int32_t* d_is_speaker) {
  if (!c) return LYRA_HIP_EINVAL;
  const char* what = "meeting_mix";
  MeetPass mp;
  int rc = meet_plan_checked(c, what, spans, P, stays, n_stays, max_speakers, &mp);
  if (rc) return rc;
  if ((rc = bsp_check_buffers(c, what, d_pcm16, d_mix, d_levels, max_speakers))) return rc;
  DEVSCOPE(c);
  if ((rc = meet_ensure(c, mp, 0))) return rc;
  if ((rc = enc_side_begin(c, 0))) return rc;
  rc = meet_pass_launch(c, mp, d_pcm16, d_muted, d_is_comfort_noise, max_speakers, d_mix, d_levels, d_is_speaker);
  if (!rc) rc = enc_side_done(c, 0);
  return rc;
}

int lyra_hip_spans_meeting_dev(lyra_hip_ctx* c, const lyra_hip_spans_meeting_call* call) {
  if (!c) return LYRA_HIP_EINVAL;
  if (!call) return fail(c, LYRA_HIP_EINVAL, "meeting: null pointer");
  return meeting_dev_impl(c, call);
}

// host-buffer form: bytes past a packet's size, and the rows of DTX noise frames, read back as zeros
int lyra_hip_spans_meeting(lyra_hip_ctx* c, const lyra_hip_span* spans, int P, const int32_t* lane_ids, int n_lanes,
                           const lyra_hip_meeting_stay* stays, int n_stays, const uint8_t* packets, const int32_t* packet_bytes,
                           const int32_t* muted, unsigned flags, const int32_t* num_bits, const int32_t* dtx, int max_speakers,
                           uint8_t* out_packets, int32_t* out_packet_bytes, int16_t* pcm16, int16_t* mix, int32_t* is_noise,
                           int32_t* is_comfort_noise, int64_t* levels, int32_t* is_speaker) {
  if (!c) return LYRA_HIP_EINVAL;
  const char* what = "meeting";
  {
    MeetPass mp;   // (the staging is sized by the spans: judge them first)
    const int rc = meet_plan_checked(c, what, spans, P, stays, n_stays, 0, &mp);
    if (rc) return rc;
  }
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
    lyra_hip_spans_meeting_call A = {};
    A.spans = spans;
    A.P = P;
    A.lane_ids = lane_ids;
    A.n_lanes = n_lanes;
    A.stays = stays;
    A.n_stays = n_stays;
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
    return meeting_dev_impl(c, &A);
  });
}

}  // extern "C"
