// bridge_plan_test.cc -- a program of its own over lyra_amd/csrc/bridge_plan.h (no GPU, no library): reads room labels (int32,
// one per row) from the file named on the command line, runs the planner and prints
//   rc n_rooms n_members / the order / the room boundaries
// one line each, for tests/test_bridge_cpu.py to compare with its numpy restatement.  Built with -fsanitize=address,undefined:
// the output arrays are sized exactly (B and B + 1 entries), so a planner that writes past either is caught here.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "bridge_plan.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> rooms;
  int32_t v;
  while (std::fread(&v, sizeof v, 1, f) == 1) rooms.push_back(v);
  std::fclose(f);
  const int B = (int)rooms.size();
  std::vector<int32_t> order((size_t)B), start((size_t)B + 1);
  int n_rooms = -1, n_members = -1;
  const int rc = bridge::plan(rooms.data(), B, order.data(), start.data(), &n_rooms, &n_members);
  if (rc) {
    std::printf("%d\n", rc);
    return 0;
  }
  std::printf("%d %d %d\n", rc, n_rooms, n_members);
  for (int i = 0; i < n_members; ++i) std::printf("%d ", order[i]);
  std::printf("\n");
  for (int i = 0; i <= n_rooms; ++i) std::printf("%d ", start[i]);
  std::printf("\n");
  // null pointers and a negative size are refused without a write
  if (bridge::plan(rooms.data(), B, nullptr, start.data(), &n_rooms, &n_members) != -1 ||
      bridge::plan(rooms.data(), -1, order.data(), start.data(), &n_rooms, &n_members) != -1 ||
      bridge::plan(nullptr, B > 0 ? B : 1, order.data(), start.data(), &n_rooms, &n_members) != -1)
    return 3;
  std::printf("ok\n");
  return 0;
}
