// shared_plan_test.cc -- TEST INFRASTRUCTURE: the planner-side check of room_labels (lyra_amd/csrc/shared_bridge_plan.h) behind
// bridge::plan, with a plain compiler.  Prints "ok"; exit status 0 on success.
#include <cstdio>
#include <vector>

#include "bridge_plan.h"
#include "shared_bridge_plan.h"

#define CHECK_THAT(cond)                                                              \
  do {                                                                                \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; }  \
  } while (0)

namespace sb = shared_bridge;

int main() {
  const std::vector<int32_t> rooms = {7, -1, 2, 7, 40, 2, -5, 7};
  const int B = static_cast<int>(rooms.size());
  std::vector<int32_t> order(B), start(B + 1);
  int n_rooms = 0, n_members = 0;
  CHECK_THAT(bridge::plan(rooms.data(), B, order.data(), start.data(), &n_rooms, &n_members) == 0 && n_rooms == 3 && n_members == 6);
  auto check = [&](std::vector<int32_t> labels, int limit, int* at) {
    return sb::check_labels(rooms.data(), order.data(), start.data(), n_rooms, labels.data(), static_cast<int>(labels.size()), limit, at);
  };
  int at = 99;
  CHECK_THAT(check({2, 7, 40}, 41, &at) == sb::LABELS_OK && at == -1);
  CHECK_THAT(check({2, 7, 40}, 40, &at) == sb::LABELS_RANGE && at == 2);
  CHECK_THAT(check({2, 7}, 64, &at) == sb::LABELS_COUNT && check({2, 7, 40, 41}, 64, &at) == sb::LABELS_COUNT && at == -1);
  CHECK_THAT(check({7, 2, 40}, 64, &at) == sb::LABELS_SET && at == 0);       // the first room of the index is label 2
  CHECK_THAT(check({2, 2, 40}, 64, &at) == sb::LABELS_ORDER && at == 1);
  CHECK_THAT(check({2, 8, 40}, 64, &at) == sb::LABELS_SET && at == 1);       // ascending, but nobody sits in room 8
  CHECK_THAT(check({-2, 7, 40}, 64, &at) == sb::LABELS_RANGE && at == 0);
  CHECK_THAT(check({2, 7, 40}, 64, nullptr) == sb::LABELS_OK);
  // nobody in any room: no labels, and nothing is read
  const std::vector<int32_t> none = {-1, -1};
  CHECK_THAT(bridge::plan(none.data(), 2, order.data(), start.data(), &n_rooms, &n_members) == 0 && n_rooms == 0);
  CHECK_THAT(sb::check_labels(none.data(), order.data(), start.data(), 0, nullptr, 0, 64, &at) == sb::LABELS_OK);
  CHECK_THAT(sb::check_labels(none.data(), order.data(), start.data(), 0, rooms.data(), 1, 64, &at) == sb::LABELS_COUNT);
  std::printf("ok\n");
  return 0;
}
