// fake_decode_streams_abi.cc -- TEST INFRASTRUCTURE: a CPU stand-in for the three calls of include/lyra_hip_decode_streams.h,
// linked next to tests/host_stub/fake_lyra_hip_codec.cc (which has every other entry point the host classes use and stays as
// it is).  It records what each begin() received and answers with FakeDecodeStreamsSample, rows packed back to back; a row
// without a packet is "comfort noise" (is_comfort_noise 1), a row with an 8-byte packet is "noise" (is_noise 1).  Never linked
// into the product.
#include <cstdint>
#include <deque>
#include <vector>

#include "fake_decode_streams_abi.h"

std::vector<FakeDecodeStreamsCall> g_fake_dstr_calls;
int g_fake_dstr_ends = 0;
bool g_fake_dstr_fail_begin = false, g_fake_dstr_fail_end = false;

namespace {
struct Result { std::vector<int16_t> pcm; std::vector<int32_t> noise, cn; };
std::deque<Result> g_queue;
}  // namespace

extern "C" {

int lyra_hip_decode_streams_dev(lyra_hip_ctx*, const int32_t*, int, const uint8_t*, const int32_t*, const int32_t*, int16_t*,
                                long, const int32_t*, int16_t*, int32_t*, int32_t*) {
  return -1;   // (device buffers: nothing a host class calls)
}

int lyra_hip_decode_streams_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets,
                                  const int32_t* packet_bytes, const int32_t* rates) {
  if (g_fake_dstr_fail_begin) { g_fake_dstr_fail_begin = false; return -2; }
  if (!c || !ids || B <= 0 || !packets || !packet_bytes || !rates || g_queue.size() >= 2) return -1;
  FakeDecodeStreamsCall call;
  call.B = B;
  Result r;
  const long number = static_cast<long>(g_fake_dstr_calls.size());
  for (int b = 0; b < B; ++b) {
    const int n = rates[b] / 50, nb = packet_bytes[b];
    const uint8_t first = nb ? packets[static_cast<size_t>(b) * 23] : 0;
    call.ids.push_back(ids[b]);
    call.rates.push_back(rates[b]);
    call.bytes.push_back(nb);
    call.first.push_back(first);
    call.offsets.push_back(static_cast<long>(r.pcm.size()));
    for (int i = 0; i < n; ++i) r.pcm.push_back(FakeDecodeStreamsSample(ids[b], rates[b], number, nb, first, i));
    r.noise.push_back(nb == 8 ? 1 : 0);
    r.cn.push_back(nb == 0 ? 1 : 0);
  }
  call.total = static_cast<long>(r.pcm.size());
  g_fake_dstr_calls.push_back(call);
  g_queue.push_back(r);
  return 0;
}

int lyra_hip_decode_streams_end(lyra_hip_ctx* c, int16_t* pcm, int32_t* is_noise, int32_t* is_comfort_noise) {
  if (g_fake_dstr_fail_end) { g_fake_dstr_fail_end = false; return -2; }
  if (!c || !pcm || g_queue.empty()) return -1;
  const Result& r = g_queue.front();
  for (size_t i = 0; i < r.pcm.size(); ++i) pcm[i] = r.pcm[i];
  for (size_t i = 0; i < r.noise.size(); ++i) {
    if (is_noise) is_noise[i] = r.noise[i];
    if (is_comfort_noise) is_comfort_noise[i] = r.cn[i];
  }
  g_queue.pop_front();
  ++g_fake_dstr_ends;
  return 0;
}

}  // extern "C"
