// fake_bridge_abi.cc -- TEST INFRASTRUCTURE: a CPU stand-in for the calls of include/lyra_hip_bridge.h (and for
// lyra_hip_reset_streams, which no other host class uses), linked next to tests/host_stub/fake_lyra_hip_codec.cc (which has
// every other entry point the host classes use and stays as it is).  It records what each begin() received and answers with
// FakeBridgeLength / FakeBridgeByte; a row without a packet is "comfort noise" (is_comfort_noise 1), a row with an 8-byte packet
// is "noise" (is_noise 1).  Never linked into the product.
#include <cstdint>
#include <deque>
#include <vector>

#include "fake_bridge_abi.h"

std::vector<FakeBridgeCall> g_fake_bridge_calls;
std::vector<int32_t> g_fake_bridge_resets;
int g_fake_bridge_ends = 0;
bool g_fake_bridge_fail_begin = false, g_fake_bridge_fail_end = false, g_fake_bridge_fail_reset = false;

namespace {
struct Result { std::vector<uint8_t> rows; std::vector<int32_t> lens, noise, cn; };
std::deque<Result> g_queue;
}  // namespace

extern "C" {

int lyra_hip_bridge_plan(const int32_t*, int, int32_t*, int32_t*, int*, int*) { return -1; }   // (nothing a host class calls)
int lyra_hip_bridge_mix_dev(lyra_hip_ctx*, const int16_t*, int, const int32_t*, const int32_t*, int, int, const int32_t*,
                            const int32_t*, int16_t*) {
  return -1;   // (device buffers)
}
int lyra_hip_bridge_tick_dev(lyra_hip_ctx*, const lyra_hip_bridge_tick*) { return -1; }
long lyra_hip_bridge_errors(lyra_hip_ctx*, int) { return 0; }

int lyra_hip_reset_streams(lyra_hip_ctx* c, const int32_t* ids, int n) {
  if (g_fake_bridge_fail_reset) { g_fake_bridge_fail_reset = false; return -2; }
  if (!c || !ids || n <= 0) return -1;
  for (int i = 0; i < n; ++i) g_fake_bridge_resets.push_back(ids[i]);
  return 0;
}

int lyra_hip_bridge_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets, const int32_t* packet_bytes,
                          const int32_t* rooms, const int32_t* muted, unsigned flags, const int32_t* num_bits,
                          const int32_t* dtx) {
  if (g_fake_bridge_fail_begin) { g_fake_bridge_fail_begin = false; return -2; }
  if (!c || !ids || B <= 0 || !packets || !packet_bytes || !rooms || !num_bits || g_queue.size() >= 2) return -1;
  FakeBridgeCall call;
  call.B = B;
  call.flags = flags;
  Result r;
  r.rows.assign(static_cast<size_t>(B) * 23, 0);
  const long number = static_cast<long>(g_fake_bridge_calls.size());
  for (int b = 0; b < B; ++b) {
    const int nb = packet_bytes[b], m = muted ? muted[b] : 0;
    const uint8_t first = nb ? packets[static_cast<size_t>(b) * 23] : 0;
    call.ids.push_back(ids[b]);
    call.bytes.push_back(nb);
    call.first.push_back(first);
    call.rooms.push_back(rooms[b]);
    call.muted.push_back(m);
    call.bits.push_back(num_bits[b]);
    call.dtx.push_back(dtx ? dtx[b] : 0);
    const int len = FakeBridgeLength(rooms[b], num_bits[b]);
    r.lens.push_back(len);
    if (len) r.rows[static_cast<size_t>(b) * 23] = FakeBridgeByte(ids[b], number, rooms[b], m, first);
    r.noise.push_back(nb == 8 ? 1 : 0);
    r.cn.push_back(nb == 0 ? 1 : 0);
  }
  g_fake_bridge_calls.push_back(call);
  g_queue.push_back(r);
  return 0;
}

int lyra_hip_bridge_end(lyra_hip_ctx* c, uint8_t* out_packets, int32_t* out_packet_bytes, int32_t* is_noise,
                        int32_t* is_comfort_noise) {
  if (g_fake_bridge_fail_end) { g_fake_bridge_fail_end = false; return -2; }
  if (!c || !out_packets || !out_packet_bytes || g_queue.empty()) return -1;
  const Result& r = g_queue.front();
  for (size_t i = 0; i < r.rows.size(); ++i) out_packets[i] = r.rows[i];
  for (size_t i = 0; i < r.lens.size(); ++i) {
    out_packet_bytes[i] = r.lens[i];
    if (is_noise) is_noise[i] = r.noise[i];
    if (is_comfort_noise) is_comfort_noise[i] = r.cn[i];
  }
  g_queue.pop_front();
  ++g_fake_bridge_ends;
  return 0;
}

}  // extern "C"
