// bridge_recording_test.cc -- the host-only part of BridgeRecordingTimeParallel (lyra_amd/host/lyra_bridge_recording.h) and the
// data-model check of lyra_amd/csrc/bridge_spans_plan.h, as a program of its own for a plain compiler and the sanitizers:
//   bridge_recording_test <script.i32> <num_streams>
// reads a script [ticks][num_streams][3] int32 and prints the first tick of every segment on one line, then "ok".  Before that it
// runs the planner's own cases (no input needed) and aborts on the first that fails.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

#include "bridge_spans_plan.h"
#include "lyra_bridge_recording.h"

#define CHECK_THAT(cond)                                                   \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

int main(int argc, char** argv) {
  using bridge_spans::Span;
  {
    std::vector<Span> s = {{4, 0, 5}, {9, 7, 5}, {2, 12, 5}};
    const int32_t rooms[3] = {7, -1, 7};
    int32_t order[3], start[4];
    int n_rooms = -1, n_members = -1;
    int64_t T = -1;
    CHECK_THAT(bridge_spans::plan(s.data(), 3, rooms, order, start, &n_rooms, &n_members, &T) == 0);
    CHECK_THAT(T == 5 && n_rooms == 1 && n_members == 2 && order[0] == 0 && order[1] == 2 && start[0] == 0 && start[1] == 2);
    s[1].n_frames = 4;                                  // unequal n_frames
    CHECK_THAT(bridge_spans::check(s.data(), 3, &T) != 0);
    s[1] = {9, 4, 5};                                   // overlaps span 0
    CHECK_THAT(bridge_spans::check(s.data(), 3, &T) != 0);
    s[1] = {4, 7, 5};                                   // an id named twice
    CHECK_THAT(bridge_spans::check(s.data(), 3, &T) != 0);
    s[1] = {9, -7, 5};                                  // a negative range
    CHECK_THAT(bridge_spans::check(s.data(), 3, &T) != 0);
    s[1] = {-9, 7, 5};
    CHECK_THAT(bridge_spans::check(s.data(), 3, &T) != 0);
    s[1] = {9, 7, 5};
    CHECK_THAT(bridge_spans::check(s.data(), 3, &T) == 0 && bridge_spans::check(s.data(), 0, &T) != 0);
    CHECK_THAT(bridge_spans::check(nullptr, 3, &T) != 0 && bridge_spans::check(s.data(), 3, nullptr) != 0);
    for (Span& x : s) x.n_frames = 0;                   // an empty recording is a valid one, wherever its spans point
    s[1].first_frame = 0;
    CHECK_THAT(bridge_spans::check(s.data(), 3, &T) == 0 && T == 0);
    std::vector<Span> big = {{0, 0, bridge_spans::MAX_FRAMES / 2 + 1}, {1, bridge_spans::MAX_FRAMES, bridge_spans::MAX_FRAMES / 2 + 1}};
    CHECK_THAT(bridge_spans::check(big.data(), 2, &T) != 0);   // more span frames than one call takes
  }
  if (argc != 3) return 2;
  const int n = std::atoi(argv[2]);
  std::ifstream in(argv[1], std::ios::binary);
  std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  const size_t row = sizeof(int32_t) * chromemedia::codec::kBridgeScriptFields * static_cast<size_t>(n);
  if (!in || n < 1 || raw.size() % row != 0) return 2;
  std::vector<int32_t> script(raw.size() / sizeof(int32_t));
  for (size_t i = 0; i < script.size(); ++i) script[i] = reinterpret_cast<const int32_t*>(raw.data())[i];
  const auto starts = chromemedia::codec::BridgeRecordingSegmentStarts(script.data(), static_cast<int64_t>(raw.size() / row), n);
  for (int64_t t : starts) std::printf("%lld ", static_cast<long long>(t));
  std::printf("\nok\n");
  return 0;
}
