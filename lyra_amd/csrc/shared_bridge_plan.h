// shared_bridge_plan.h -- host-only: what lyra_hip_shared_begin (include/lyra_hip_shared_bridge.h) holds the caller's
// room_labels to, shared by api.hip and a plain compiler (tests/shared_bridge/shared_plan_test.cc).  The encoder rows of a tick
// are laid out room by room in the order of bridge::plan (ascending label); room_labels says which label every block of
// 1 + max_speakers encoder rows belongs to, and is the key of the room's row of the slot table.
#ifndef LYRA_SHARED_BRIDGE_PLAN_H_
#define LYRA_SHARED_BRIDGE_PLAN_H_

#include <cstdint>

namespace shared_bridge {

enum { LABELS_OK = 0, LABELS_NULL = -1, LABELS_COUNT = -2, LABELS_ORDER = -3, LABELS_RANGE = -4, LABELS_SET = -5 };

// rooms[B] and the index that bridge::plan made of it (order, room_start, n_rooms) against labels[n_labels]:
//   LABELS_COUNT  n_labels is not the number of rooms present;   LABELS_ORDER  not strictly ascending;
//   LABELS_RANGE  a label outside [0, label_limit);               LABELS_SET    a label that is not the room's at its position.
// *at receives the offending position in labels where there is one.
inline int check_labels(const int32_t* rooms, const int32_t* order, const int32_t* room_start, int n_rooms,
                        const int32_t* labels, int n_labels, int label_limit, int* at) {
  if (at) *at = -1;
  if (n_labels != n_rooms) return LABELS_COUNT;
  if (n_rooms == 0) return LABELS_OK;
  if (!rooms || !order || !room_start || !labels) return LABELS_NULL;
  for (int i = 0; i < n_rooms; ++i) {
    if (at) *at = i;
    if (labels[i] < 0 || labels[i] >= label_limit) return LABELS_RANGE;
    if (i && labels[i] <= labels[i - 1]) return LABELS_ORDER;
    if (rooms[order[room_start[i]]] != labels[i]) return LABELS_SET;   // (a room of the index is never empty)
  }
  if (at) *at = -1;
  return LABELS_OK;
}

}  // namespace shared_bridge
#endif  // LYRA_SHARED_BRIDGE_PLAN_H_
