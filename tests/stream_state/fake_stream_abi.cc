// fake_stream_abi.cc -- the stream-state calls of the C ABI (and lyra_hip_decode_samples_begin / _end, which
// tests/host_stub/fake_lyra_hip_codec.cc does not have) without a GPU, for tests/test_stream_state_cpu.py: a stream's "state"
// is whatever blob was imported last, or a reset blob whose DsState the test sets through fake_set_ds_state.  Import runs the
// real sb::validate.
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "include/lyra_hip.h"
#include "lyra_amd/csrc/stream_blob.h"

using namespace lyra;

namespace {
std::map<std::pair<const void*, int>, std::vector<uint8_t>> g_state;
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
void fake_set_ds_state(const void* c, int id, const DsState* s) {
  std::memcpy(slot(c, id).data() + sb::region_off(st::R_CNG) + DS_STATE, s, sizeof *s);
}
int fake_requests_begun() { return g_begun; }
size_t lyra_hip_stream_blob_bytes(void) { return sb::BYTES; }
int lyra_hip_export_streams(lyra_hip_ctx* c, const int32_t* ids, int B, uint8_t* blobs) {
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
  if (sides == 0 || sides > 3) return LYRA_HIP_EINVAL;
  for (int b = 0; b < B; ++b)
    if (sb::validate(blobs + (size_t)b * sb::BYTES, LYRA_HIP_REQUANT_DEFAULT) != sb::V_OK) return LYRA_HIP_EINVAL;
  for (int b = 0; b < B; ++b) slot(c, ids[b]).assign(blobs + (size_t)b * sb::BYTES, blobs + (size_t)(b + 1) * sb::BYTES);
  return 0;
}
int lyra_hip_decode_samples_begin(lyra_hip_ctx*, const int32_t*, int, const uint8_t*, const int32_t*, int, int) { ++g_begun; return 0; }
int lyra_hip_decode_samples_end(lyra_hip_ctx*, int16_t*) { return 0; }
}
