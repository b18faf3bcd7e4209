// bridge_spans_plan.h -- host-only: the data model of a recording through the bridge (include/lyra_hip_bridge_spans.h), shared by
// api.hip and a plain compiler.  P participants over the same T ticks: participant p is spans[p], its tick t is buffer frame
// spans[p].first_frame + t; one room label per participant.  check() holds the rules that need no context; plan() adds the
// membership index of bridge_plan.h over participant numbers 0 .. P-1.
#ifndef LYRA_BRIDGE_SPANS_PLAN_H_
#define LYRA_BRIDGE_SPANS_PLAN_H_

#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "bridge_plan.h"

namespace bridge_spans {

struct Span { int32_t stream_id; int64_t first_frame; int64_t n_frames; };   // = lyra_hip_span

// A recording of more span frames than this is refused: the lossy span decode counts its frames in an int32 with headroom.
constexpr int64_t MAX_FRAMES = INT32_MAX / 2;

// 0 and *n_ticks = T, or -1: a null pointer, P < 1, a negative id, first_frame or n_frames, unequal n_frames, an id named
// twice, frame ranges that overlap, or more than MAX_FRAMES span frames in all
inline int check(const Span* spans, int P, int64_t* n_ticks) {
  if (!spans || P < 1 || !n_ticks) return -1;
  const int64_t T = spans[0].n_frames;
  if (T < 0 || T > MAX_FRAMES / P) return -1;
  std::vector<int32_t> ids((size_t)P);
  std::vector<int64_t> firsts((size_t)P);
  for (int p = 0; p < P; ++p) {
    if (spans[p].stream_id < 0 || spans[p].first_frame < 0 || spans[p].n_frames != T) return -1;
    if (spans[p].first_frame > INT64_MAX / 1024 - T) return -1;   // (frame * 640 bytes stays inside 64 bits)
    ids[(size_t)p] = spans[p].stream_id;
    firsts[(size_t)p] = spans[p].first_frame;
  }
  std::sort(ids.begin(), ids.end());
  if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) return -1;
  if (T > 0) {
    std::sort(firsts.begin(), firsts.end());
    for (int p = 1; p < P; ++p)
      if (firsts[(size_t)p - 1] + T > firsts[(size_t)p]) return -1;
  }
  *n_ticks = T;
  return 0;
}

// check(), then bridge::plan over the participants: order [P], room_start [P + 1]
inline int plan(const Span* spans, int P, const int32_t* rooms, int32_t* order, int32_t* room_start, int* n_rooms, int* n_members,
                int64_t* n_ticks) {
  if (!rooms || check(spans, P, n_ticks)) return -1;
  return bridge::plan(rooms, P, order, room_start, n_rooms, n_members);
}

}  // namespace bridge_spans
#endif  // LYRA_BRIDGE_SPANS_PLAN_H_
