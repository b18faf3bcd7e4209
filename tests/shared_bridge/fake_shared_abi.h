// fake_shared_abi.h -- what tests/shared_bridge/fake_shared_abi.cc recorded (TEST INFRASTRUCTURE).
#ifndef TESTS_SHARED_BRIDGE_FAKE_SHARED_ABI_H_
#define TESTS_SHARED_BRIDGE_FAKE_SHARED_ABI_H_
#include <cstdint>
#include <vector>

#include "../../include/lyra_hip_shared_bridge.h"

struct FakeSharedCall {   // one lyra_hip_shared_begin as the fake saw it
  int B = 0, max_speakers = 0, n_rooms = 0;
  unsigned flags = 0;
  std::vector<int32_t> ids, bytes, rooms, muted, labels, enc_ids, enc_bits, enc_dtx;
};
extern std::vector<FakeSharedCall> g_fake_shared_calls;
extern std::vector<int32_t> g_fake_shared_room_resets;   // the labels lyra_hip_shared_reset_rooms was given, in order
extern int g_fake_shared_ends;
extern bool g_fake_shared_fail_begin, g_fake_shared_fail_end;   // the next call returns an error

// What the fake answers for row b of call number `call`.  Member k (counted inside its room, in row order) of a room holds slot
// k if k < max_speakers and it is not muted, else none; its packet is the one of its room's encoder row 1 + slot (or 0): as
// many bytes as that row's bits / 8 rounded up -- none for a row in no room -- with a first byte that is a formula of the
// ENCODER id and the call's number, so that two listeners of one mix receive the same bytes and a wrong setting changes them.
inline int FakeSharedLength(int room, int bits) { return room < 0 ? 0 : (bits + 7) / 8; }
inline uint8_t FakeSharedByte(int enc_id, long call, int dtx) { return static_cast<uint8_t>(enc_id * 37 + 13 * static_cast<int>(call) + dtx); }
inline int64_t FakeSharedLevel(int id, long call, int bytes) { return (int64_t{1} << 35) * (id + 1) + 1000 * call + bytes; }
#endif
