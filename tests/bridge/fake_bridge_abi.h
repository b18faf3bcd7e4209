// fake_bridge_abi.h -- what tests/bridge/fake_bridge_abi.cc recorded (TEST INFRASTRUCTURE).
#ifndef TESTS_BRIDGE_FAKE_BRIDGE_ABI_H_
#define TESTS_BRIDGE_FAKE_BRIDGE_ABI_H_
#include <cstdint>
#include <vector>

#include "../../include/lyra_hip_bridge.h"

struct FakeBridgeCall {   // one lyra_hip_bridge_begin as the fake saw it
  int B = 0;
  unsigned flags = 0;
  std::vector<int32_t> ids, bytes, rooms, muted, bits, dtx;
  std::vector<uint8_t> first;          // byte 0 of row b's incoming packet (0 where the row has none)
};
extern std::vector<FakeBridgeCall> g_fake_bridge_calls;
extern std::vector<int32_t> g_fake_bridge_resets;   // the ids lyra_hip_reset_streams was given, in order
extern int g_fake_bridge_ends;
extern bool g_fake_bridge_fail_begin, g_fake_bridge_fail_end, g_fake_bridge_fail_reset;   // the next call returns an error

// What the fake answers for row b: a packet of bits / 8 (rounded up) bytes -- none for a row in no room -- whose first byte is a
// formula of the stream, the call's number, the room, the mute flag and the incoming packet, so that a row delivered from the
// wrong tick or begun with the wrong settings changes the bytes.
inline int FakeBridgeLength(int room, int bits) { return room < 0 ? 0 : (bits + 7) / 8; }
inline uint8_t FakeBridgeByte(int id, long call, int room, int muted, uint8_t first) {
  return static_cast<uint8_t>(id * 31 + 7 * static_cast<int>(call) + room * 5 + muted * 3 + first);
}
#endif
