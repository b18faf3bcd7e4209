// fake_speakers_abi.h -- what tests/speakers/fake_speakers_abi.cc recorded (TEST INFRASTRUCTURE).
#ifndef TESTS_SPEAKERS_FAKE_SPEAKERS_ABI_H_
#define TESTS_SPEAKERS_FAKE_SPEAKERS_ABI_H_
#include <cstdint>
#include <vector>

#include "../../include/lyra_hip_speakers.h"

struct FakeSpeakersCall {   // one lyra_hip_speakers_begin as the fake saw it
  int B = 0, max_speakers = 0;
  unsigned flags = 0;
  std::vector<int32_t> ids, bytes, rooms, muted, bits, dtx;
};
extern std::vector<FakeSpeakersCall> g_fake_speakers_calls;
extern int g_fake_speakers_ends;
extern bool g_fake_speakers_fail_begin, g_fake_speakers_fail_end;   // the next call returns an error

// What the fake answers for row b of call number `call`: a packet of bits / 8 (rounded up) bytes -- none for a row in no room --
// whose first byte, the row's level and its speaker flag are formulas of the stream, the call's number and the settings, so
// that a row delivered from the wrong tick or begun with the wrong settings changes them.
inline int FakeSpeakersLength(int room, int bits) { return room < 0 ? 0 : (bits + 7) / 8; }
inline uint8_t FakeSpeakersByte(int id, long call, int room, int muted) {
  return static_cast<uint8_t>(id * 29 + 11 * static_cast<int>(call) + room * 5 + muted * 3);
}
inline int64_t FakeSpeakersLevel(int id, long call, int bytes) { return (int64_t{1} << 36) * (id + 1) + 1000 * call + bytes; }
inline int32_t FakeSpeakersFlag(int id, long call, int room, int muted, int max_speakers) {
  return room >= 0 && !muted && (id + static_cast<int>(call)) % 8 < max_speakers ? 1 : 0;
}
#endif
