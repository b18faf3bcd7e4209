// bridge_plan.h -- host-only: the membership index of the conference bridge (include/lyra_hip_bridge.h), shared by api.hip
// and a plain compiler (tests/bridge/bridge_plan_test.cc).  Room labels per row -> the inverted index bridge_mix_kernel reads:
// order[] holds row numbers with a room's rows contiguous, rooms in ascending label order and rows in ascending order inside
// a room; room_start[] holds the n_rooms + 1 boundaries.  Rows with a negative label are in no room and are left out.
#ifndef LYRA_BRIDGE_PLAN_H_
#define LYRA_BRIDGE_PLAN_H_

#include <algorithm>
#include <cstdint>
#include <vector>

namespace bridge {

// Up to this many members the int32 sum of a room cannot overflow: 32,767 * 32,768 < 2^31.
constexpr int MAX_ROOM = 32767;

// 0, or -1: null pointer, B < 0, or a room of more than MAX_ROOM members (nothing is written then but scratch values)
inline int plan(const int32_t* rooms, int B, int32_t* order, int32_t* room_start, int* n_rooms, int* n_members) {
  if (B < 0 || !order || !room_start || !n_rooms || !n_members || (B > 0 && !rooms)) return -1;
  std::vector<int32_t> rows;
  rows.reserve((size_t)B);
  for (int b = 0; b < B; ++b)
    if (rooms[b] >= 0) rows.push_back(b);
  // (rows are ascending already: a stable sort by label keeps them so inside a room)
  std::stable_sort(rows.begin(), rows.end(), [&](int32_t a, int32_t b) { return rooms[a] < rooms[b]; });
  int nr = 0;
  const int nm = (int)rows.size();
  for (int i = 0; i < nm; ++i)
    if (i == 0 || rooms[rows[i]] != rooms[rows[i - 1]]) {
      if (nr && i - room_start[nr - 1] > MAX_ROOM) return -1;
      room_start[nr++] = i;
    }
  if (nr && nm - room_start[nr - 1] > MAX_ROOM) return -1;
  room_start[nr] = nm;
  std::copy(rows.begin(), rows.end(), order);
  *n_rooms = nr;
  *n_members = nm;
  return 0;
}

}  // namespace bridge
#endif  // LYRA_BRIDGE_PLAN_H_
