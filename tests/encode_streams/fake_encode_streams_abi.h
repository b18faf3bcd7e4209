// fake_encode_streams_abi.h -- what tests/encode_streams/fake_encode_streams_abi.cc recorded (TEST INFRASTRUCTURE).
#ifndef TESTS_ENCODE_STREAMS_FAKE_ENCODE_STREAMS_ABI_H_
#define TESTS_ENCODE_STREAMS_FAKE_ENCODE_STREAMS_ABI_H_
#include <cstdint>
#include <vector>

#include "../../include/lyra_hip_encode_streams.h"

struct FakeStreamsCall {   // one lyra_hip_encode_streams_begin as the fake saw it
  int B = 0;
  bool dtx_null = false;
  std::vector<int32_t> ids, rates, bits, dtx;
  std::vector<long> offsets;           // where the fake read row b: the running sum of rates / 50
  std::vector<int16_t> first, last;    // the first and the last sample it found there
  long total = 0;
};
extern std::vector<FakeStreamsCall> g_fake_streams_calls;
extern int g_fake_streams_ends;
#endif
