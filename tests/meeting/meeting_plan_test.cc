// meeting_plan_test.cc -- lyra_amd/csrc/meeting_plan.h as a program of its own, for a build under the sanitizers
// (tests/test_spans_meeting_cpu.py).  argv[1]: a file of int64 values -- P, n_stays, then P x (stream id, first_frame,
// n_frames), then n_stays x (participant, room, first_tick, n_ticks).  Prints "refused", or the plan: n_ticks, then one line
// each for epoch_tick, epoch_entry, entry_participant, entry_room, entry_base, room_start and epoch_members.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "meeting_plan.h"

template <class V>
static void line(const V& v) {
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s%lld", i ? " " : "", (long long)v[i]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int64_t> in;
  int64_t v;
  while (std::fread(&v, sizeof v, 1, f) == 1) in.push_back(v);
  std::fclose(f);
  if (in.size() < 2) return 2;
  const int64_t P = in[0], n_stays = in[1];
  if (P < 0 || n_stays < 0 || (int64_t)in.size() != 2 + 3 * P + 4 * n_stays) return 2;
  std::vector<meeting::Span> spans((size_t)P);
  std::vector<meeting::Stay> stays((size_t)n_stays);
  size_t at = 2;
  for (auto& s : spans) {
    s.stream_id = (int32_t)in[at];
    s.first_frame = in[at + 1];
    s.n_frames = in[at + 2];
    at += 3;
  }
  for (auto& s : stays) {
    s.participant = (int32_t)in[at];
    s.room = (int32_t)in[at + 1];
    s.first_tick = in[at + 2];
    s.n_ticks = in[at + 3];
    at += 4;
  }
  meeting::Plan pl;
  if (meeting::plan(spans.data(), (int)P, stays.data(), n_stays, &pl)) {
    std::printf("refused\n");
    return 0;
  }
  // the tables agree with each other
  if (pl.epoch_entry.size() != pl.epoch_tick.size() || pl.epoch_room.size() != pl.epoch_tick.size() ||
      pl.epoch_members.size() + 1 != pl.epoch_tick.size() || pl.entry_room.size() != (size_t)pl.n_entries() ||
      pl.entry_base.size() != (size_t)pl.n_entries() || pl.room_start.size() != (size_t)pl.epoch_room.back())
    return 3;
  for (int64_t e = 0; e < pl.n_epochs(); ++e) {
    const int32_t* rs = pl.room_start.data() + pl.epoch_room[(size_t)e];
    if (rs[0] != 0 || rs[pl.n_rooms(e)] != pl.epoch_members[(size_t)e]) return 3;
    for (int64_t i = pl.epoch_entry[(size_t)e]; i < pl.epoch_entry[(size_t)e + 1]; ++i) {
      const meeting::Span& s = spans[(size_t)pl.entry_participant[(size_t)i]];
      for (int64_t t : {pl.epoch_tick[(size_t)e], pl.epoch_tick[(size_t)e + 1] - 1}) {
        const int64_t frame = pl.entry_base[(size_t)i] + t;
        if (frame < s.first_frame || frame >= s.first_frame + s.n_frames) return 4;   // an entry's frames are its span's
      }
    }
  }
  std::printf("%lld\n", (long long)pl.n_ticks);
  line(pl.epoch_tick);
  line(pl.epoch_entry);
  line(pl.entry_participant);
  line(pl.entry_room);
  line(pl.entry_base);
  line(pl.room_start);
  line(pl.epoch_members);
  return 0;
}
