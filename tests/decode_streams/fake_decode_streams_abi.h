// fake_decode_streams_abi.h -- what tests/decode_streams/fake_decode_streams_abi.cc recorded (TEST INFRASTRUCTURE).
#ifndef TESTS_DECODE_STREAMS_FAKE_DECODE_STREAMS_ABI_H_
#define TESTS_DECODE_STREAMS_FAKE_DECODE_STREAMS_ABI_H_
#include <cstdint>
#include <vector>

#include "../../include/lyra_hip_decode_streams.h"

struct FakeDecodeStreamsCall {   // one lyra_hip_decode_streams_begin as the fake saw it
  int B = 0;
  std::vector<int32_t> ids, rates, bytes;
  std::vector<uint8_t> first;          // byte 0 of row b's packet (0 where the row has none)
  std::vector<long> offsets;           // where the fake wrote row b: the running sum of rates / 50
  long total = 0;
};
extern std::vector<FakeDecodeStreamsCall> g_fake_dstr_calls;
extern int g_fake_dstr_ends;
extern bool g_fake_dstr_fail_begin, g_fake_dstr_fail_end;   // the next begin() / end() returns an error (and does nothing)

// What the fake answers for sample i of a row: a formula of the stream, its rate, the call's number (0, 1, ... over the
// program's life) and the row's packet, so that a row delivered at the wrong packed offset, from the wrong hop or with the
// wrong packet changes the samples.
inline int16_t FakeDecodeStreamsSample(int id, int rate, long call, int bytes, uint8_t first, int i) {
  return static_cast<int16_t>((id + 1) * 1000 + rate / 1000 + 7 * static_cast<int>(call) + bytes * 3 + first + i % 97);
}
#endif
