// meeting_plan.h -- host-only: the data model of a meeting with a schedule (include/lyra_hip_spans_meeting.h), shared by
// api.hip and a plain compiler (tests/meeting/meeting_plan_test.cc).  P participants, spans[p].n_frames = the ticks on which
// p is present; stays say when and where.  plan() holds every rule that needs no context and builds the epoch table: the
// boundaries are the distinct values of {first_tick, first_tick + n_ticks}, an epoch is the run between two consecutive
// ones, an entry is one participant present in one epoch.  Inside an epoch the entries of rooms come first, rooms in ascending
// label order and participants ascending inside a room (the row order of the tick call over the present participants), then
// the present participants in no room.  Each entry carries a frame base: on meeting tick t its frame is base + t.
#ifndef LYRA_MEETING_PLAN_H_
#define LYRA_MEETING_PLAN_H_

#include <algorithm>
#include <cstdint>
#include <set>
#include <utility>
#include <vector>

#include "bridge_plan.h"

namespace meeting {

struct Span { int32_t stream_id; int64_t first_frame; int64_t n_frames; };                 // = lyra_hip_span
struct Stay { int32_t participant; int32_t room; int64_t first_tick; int64_t n_ticks; };   // = lyra_hip_meeting_stay

constexpr int64_t MAX_FRAMES = INT32_MAX / 2;   // span frames of a call, as the recording call
constexpr int64_t MAX_ENTRIES = 1 << 22;        // LYRA_HIP_MEETING_MAX_ENTRIES
constexpr int64_t MAX_TICK = (int64_t)1 << 40;  // the largest first_tick

struct Plan {
  int64_t n_ticks = 0;
  std::vector<int64_t> epoch_tick;          // [n_epochs + 1]
  std::vector<int64_t> epoch_entry;         // [n_epochs + 1] offsets into the entry arrays
  std::vector<int64_t> epoch_room;          // [n_epochs + 1] offsets into room_start: epoch e owns its rooms + 1 values
  std::vector<int32_t> epoch_members;       // [n_epochs] entries in rooms (they come first)
  std::vector<uint8_t> epoch_big;           // [n_epochs] a room above 64 members
  std::vector<int32_t> entry_participant;   // [n_entries]
  std::vector<int32_t> entry_room;          // [n_entries] dense room number inside the epoch, -1: in no room
  std::vector<int64_t> entry_base;          // [n_entries] frame on meeting tick t = base + t
  std::vector<int32_t> room_start;          // positions inside the epoch
  int64_t n_epochs() const { return (int64_t)epoch_tick.size() - 1; }
  int64_t n_entries() const { return epoch_entry.back(); }
  int n_rooms(int64_t e) const { return (int)(epoch_room[(size_t)e + 1] - epoch_room[(size_t)e] - 1); }
};

// the rules on spans alone: 0, or -1 for a null pointer, P < 1, a negative id, first_frame or n_frames, an id named twice,
// overlapping ranges (of spans with frames), or more than MAX_FRAMES span frames in all
inline int check_spans(const Span* spans, int P) {
  if (!spans || P < 1) return -1;
  std::vector<int32_t> ids((size_t)P);
  std::vector<std::pair<int64_t, int64_t>> ranges;
  int64_t total = 0;
  for (int p = 0; p < P; ++p) {
    const Span& s = spans[p];
    if (s.stream_id < 0 || s.first_frame < 0 || s.n_frames < 0 || s.n_frames > MAX_FRAMES - total) return -1;
    if (s.first_frame > INT64_MAX / 1024 - s.n_frames) return -1;   // (frame * 640 bytes stays inside 64 bits)
    total += s.n_frames;
    ids[(size_t)p] = s.stream_id;
    if (s.n_frames) ranges.emplace_back(s.first_frame, s.n_frames);
  }
  std::sort(ids.begin(), ids.end());
  if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return -1;
  std::sort(ranges.begin(), ranges.end());
  for (size_t i = 1; i < ranges.size(); ++i)
    if (ranges[i - 1].first + ranges[i - 1].second > ranges[i].first) return -1;
  return 0;
}

// 0 and *out, or -1: check_spans, a stay rule broken (null with n_stays > 0, n_stays < 0, participant outside 0 .. P-1,
// n_ticks < 1, first_tick outside 0 .. MAX_TICK, not sorted by (participant, first_tick), overlapping stays of one participant,
// sums that differ from n_frames), more than MAX_ENTRIES entries, or a room of more than bridge::MAX_ROOM members in an epoch
inline int plan(const Span* spans, int P, const Stay* stays, int64_t n_stays, Plan* out) {
  if (!out || check_spans(spans, P) || n_stays < 0 || (n_stays > 0 && !stays) || n_stays > MAX_FRAMES) return -1;
  std::vector<int64_t> present((size_t)P, 0), k0((size_t)n_stays, 0);
  for (int64_t i = 0; i < n_stays; ++i) {
    const Stay& s = stays[i];
    if (s.participant < 0 || s.participant >= P || s.n_ticks < 1 || s.n_ticks > MAX_FRAMES || s.first_tick < 0 || s.first_tick > MAX_TICK)
      return -1;
    if (i) {
      const Stay& b = stays[i - 1];
      if (b.participant > s.participant) return -1;
      if (b.participant == s.participant && b.first_tick + b.n_ticks > s.first_tick) return -1;
    }
    k0[(size_t)i] = present[(size_t)s.participant];
    present[(size_t)s.participant] += s.n_ticks;
    if (present[(size_t)s.participant] > MAX_FRAMES) return -1;
  }
  for (int p = 0; p < P; ++p)
    if (present[(size_t)p] != spans[p].n_frames) return -1;
  // events in tick order, leaves before joins on a tick
  struct Event { int64_t tick; int join; int64_t stay; };
  std::vector<Event> ev;
  ev.reserve((size_t)n_stays * 2);
  for (int64_t i = 0; i < n_stays; ++i) {
    ev.push_back({stays[i].first_tick, 1, i});
    ev.push_back({stays[i].first_tick + stays[i].n_ticks, 0, i});
  }
  std::sort(ev.begin(), ev.end(), [](const Event& a, const Event& b) {
    return a.tick != b.tick ? a.tick < b.tick : a.join != b.join ? a.join < b.join : a.stay < b.stay;
  });
  // the entries, counted before anything is built
  {
    int64_t active = 0, entries = 0;
    for (size_t i = 0; i < ev.size();) {
      const int64_t tick = ev[i].tick;
      for (; i < ev.size() && ev[i].tick == tick; ++i) active += ev[i].join ? 1 : -1;
      if (i < ev.size() && active) {
        entries += active;
        if (entries > MAX_ENTRIES) return -1;
      }
    }
  }
  Plan pl;
  pl.epoch_entry.push_back(0);
  pl.epoch_room.push_back(0);
  std::vector<int64_t> cur((size_t)P, -1);   // the stay a participant is in
  std::set<int32_t> active;
  std::vector<int32_t> rows;
  for (size_t i = 0; i < ev.size();) {
    const int64_t tick = ev[i].tick;
    for (; i < ev.size() && ev[i].tick == tick; ++i) {
      const int32_t p = stays[ev[i].stay].participant;
      if (ev[i].join) {
        cur[(size_t)p] = ev[i].stay;
        active.insert(p);
      } else {
        cur[(size_t)p] = -1;
        active.erase(p);
      }
    }
    pl.epoch_tick.push_back(tick);
    if (i == ev.size()) break;   // the meeting's end
    auto room_of = [&](int32_t p) { return stays[cur[(size_t)p]].room; };
    rows.assign(active.begin(), active.end());
    // (participants are ascending: a stable sort by label keeps them so inside a room; no room goes last)
    std::stable_sort(rows.begin(), rows.end(), [&](int32_t a, int32_t b) {
      const int32_t ra = room_of(a), rb = room_of(b);
      return (ra < 0) != (rb < 0) ? rb < 0 : (ra >= 0 && ra < rb);
    });
    int32_t room = -1, members = 0;
    bool big = false;
    for (size_t j = 0; j < rows.size(); ++j) {
      const int32_t p = rows[j], label = room_of(p);
      const Stay& s = stays[cur[(size_t)p]];
      if (label >= 0) {
        if (j == 0 || room_of(rows[j - 1]) != label) {
          pl.room_start.push_back((int32_t)j);
          ++room;
        }
        const int32_t size = (int32_t)j + 1 - pl.room_start.back();
        if (size > bridge::MAX_ROOM) return -1;
        big = big || size > 64;
        ++members;
      }
      pl.entry_participant.push_back(p);
      pl.entry_room.push_back(label >= 0 ? room : -1);
      pl.entry_base.push_back(spans[p].first_frame + k0[(size_t)cur[(size_t)p]] - s.first_tick);
    }
    pl.room_start.push_back(members);
    pl.epoch_members.push_back(members);
    pl.epoch_big.push_back(big ? 1 : 0);
    pl.epoch_entry.push_back((int64_t)pl.entry_participant.size());
    pl.epoch_room.push_back((int64_t)pl.room_start.size());
  }
  if (pl.epoch_tick.empty()) pl.epoch_tick.push_back(0);
  pl.n_ticks = n_stays ? pl.epoch_tick.back() : 0;
  *out = std::move(pl);
  return 0;
}

}  // namespace meeting
#endif  // LYRA_MEETING_PLAN_H_
