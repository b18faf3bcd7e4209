// fake_decode_samples_any_abi.cc -- TEST INFRASTRUCTURE: the calls of include/lyra_hip_decode_samples_any.h and the stream-state
// calls of the C ABI without a GPU, for tests/test_decode_samples_any_class_cpu.py (next to the unchanged fake of
// tests/host_stub).  A stream's "state" is a blob: a reset blob, or whatever was imported last.  begin() keeps the integers
// the device keeps -- DsState and the leftover count -- in that blob, advanced with the shared host/device functions from the
// arguments it was GIVEN, so a class that hands over the wrong packets or sizes ends up with a mirror that differs from the
// exported blob.  Import runs the real sb::validate.  Never linked into the product.
#include <cstring>
#include <deque>
#include <map>
#include <utility>
#include <vector>

#include "include/lyra_hip_decode_samples_any.h"
#include "lyra_amd/csrc/stream_blob.h"

using namespace lyra;

namespace {
std::map<std::pair<const void*, int>, std::vector<uint8_t>> g_state;
std::map<const void*, std::deque<std::pair<int, int>>> g_flight;   // (B, n) of the requests begun, oldest first
int g_begun = 0;

std::vector<uint8_t>& slot(const void* c, int id) {
  std::vector<uint8_t>& b = g_state[{c, id}];
  if (b.empty()) {
    b.assign(sb::BYTES, 0);
    sb::put32(b.data() + sb::region_off(st::R_NOISE_E) + st::N_IS_NOISE, 1);
    sb::put32(b.data() + sb::region_off(st::R_NOISE_D) + st::N_IS_NOISE, 1);
  }
  return b;
}
}  // namespace

extern "C" {
int fake_any_requests_begun() { return g_begun; }
size_t lyra_hip_stream_blob_bytes(void) { return sb::BYTES; }
int lyra_hip_export_streams(lyra_hip_ctx* c, const int32_t* ids, int B, uint8_t* blobs) {
  if (!g_flight[c].empty()) return LYRA_HIP_EINVAL;
  for (int b = 0; b < B; ++b) {
    uint8_t* out = blobs + (size_t)b * sb::BYTES;
    std::memcpy(out, slot(c, ids[b]).data(), sb::BYTES);
    uint32_t w[16];
    sb::header_words(LYRA_HIP_REQUANT_DEFAULT, ids[b], 0x1234u ^ (unsigned)ids[b], w);
    std::memset(out, 0, sb::HEADER_BYTES);
    std::memcpy(out, w, sizeof w);
  }
  return 0;
}
int lyra_hip_import_streams(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* blobs, unsigned sides) {
  if (sides == 0 || sides > 3 || !g_flight[c].empty()) return LYRA_HIP_EINVAL;
  for (int b = 0; b < B; ++b)
    if (sb::validate(blobs + (size_t)b * sb::BYTES, LYRA_HIP_REQUANT_DEFAULT) != sb::V_OK) return LYRA_HIP_EINVAL;
  for (int b = 0; b < B; ++b) slot(c, ids[b]).assign(blobs + (size_t)b * sb::BYTES, blobs + (size_t)(b + 1) * sb::BYTES);
  return 0;
}
int lyra_hip_decode_samples_any_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets,
                                      const int32_t* packet_bytes, int n, int rate) {
  if (!ds_any_valid(n, rate) || !ids || !packets || !packet_bytes || g_flight[c].size() >= 2) return LYRA_HIP_EINVAL;
  for (int b = 0; b < B; ++b) {
    uint8_t* blob = slot(c, ids[b]).data();
    uint8_t* cnt = blob + sb::region_off(st::R_RS_D) + DSA_LEFT_COUNT;
    DsState s;
    std::memcpy(&s, blob + sb::region_off(st::R_CNG) + DS_STATE, sizeof s);
    const DsaStep step = ds_any_step((int)sb::ld32(cnt), n, rate);
    sb::put32(cnt, (uint32_t)step.left);
    const int R = ds_any_rounds(n, rate);
    for (int r = 0; r < (R > 0 ? R : 1); ++r) s = ds_plan(s, r == 0 && mixed_received(packet_bytes[b]), ds_any_round_total(step.n_int, r)).s;
    std::memcpy(blob + sb::region_off(st::R_CNG) + DS_STATE, &s, sizeof s);
  }
  g_flight[c].push_back({B, n});
  ++g_begun;
  return 0;
}
int lyra_hip_decode_samples_any_end(lyra_hip_ctx* c, int16_t* pcm) {
  if (g_flight[c].empty()) return LYRA_HIP_EINVAL;
  const std::pair<int, int> q = g_flight[c].front();
  if (q.second > 0 && !pcm) return LYRA_HIP_EINVAL;
  g_flight[c].pop_front();
  for (long i = 0; i < (long)q.first * q.second; ++i) pcm[i] = (int16_t)(q.second + i % 7);   // (the request's size, so a swapped pair shows)
  return 0;
}
}
