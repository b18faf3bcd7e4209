// fake_decode_samples_streams_abi.cc -- TEST INFRASTRUCTURE: the three calls of include/lyra_hip_decode_samples_streams.h
// without a GPU, for tests/test_decode_samples_streams_class_cpu.py.  Linked NEXT TO the unchanged fakes of
// tests/decode_samples_any (whose stream blobs and export / import it uses, so a stream moves between the two pipelines as on
// the device) and tests/host_stub.  begin() advances the integers the device keeps -- DsState and the leftover count -- with
// the shared host/device functions from the arguments it was GIVEN, row by row with the row's own rate and size, so a class
// that hands over the wrong rows ends up with a mirror that differs from the exported blob.  Never linked into the product.
#include <cstring>
#include <deque>
#include <map>
#include <vector>

#include "include/lyra_hip_decode_samples_streams.h"
#include "lyra_amd/csrc/decode_samples_streams_plan.h"
#include "lyra_amd/csrc/stream_blob.h"

using namespace lyra;

namespace {
struct Request { std::vector<int32_t> sizes; std::vector<int32_t> cn; };
std::map<const void*, std::deque<Request>> g_flight;
int g_begun = 0, g_max_hops = 0;
}  // namespace

extern "C" {
int fake_streams_requests_begun() { return g_begun; }
int fake_streams_last_max_hops() { return g_max_hops; }

int lyra_hip_decode_samples_streams_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets,
                                          const int32_t* packet_bytes, const int32_t* rates, const int32_t* sizes) {
  if (!ids || !packets || !packet_bytes || !rates || !sizes || B <= 0 || g_flight[c].size() >= 2) return LYRA_HIP_EINVAL;
  for (int b = 0; b < B; ++b) {
    if (dss_size_verdict(rates[b], sizes[b]) != DSS_OK) return LYRA_HIP_EINVAL;
    for (int a = 0; a < b; ++a)
      if (ids[a] == ids[b]) return LYRA_HIP_EINVAL;
  }
  const int R = dss_batch_rounds(rates, sizes, B);
  Request q;
  std::vector<uint8_t> blob(sb::BYTES);
  for (int b = 0; b < B; ++b) {
    if (lyra_hip_export_streams(c, &ids[b], 1, blob.data()) != 0) return LYRA_HIP_EINVAL;
    uint8_t* cnt = blob.data() + sb::region_off(st::R_RS_D) + DSA_LEFT_COUNT;
    DsState s;
    std::memcpy(&s, blob.data() + sb::region_off(st::R_CNG) + DS_STATE, sizeof s);
    const DsaStep step = ds_any_step((int)sb::ld32(cnt), sizes[b], rates[b]);
    sb::put32(cnt, (uint32_t)step.left);
    for (int r = 0; r < R; ++r)   // (every row runs the call's rounds; those past its own plan 0 samples)
      s = ds_plan(s, r == 0 && mixed_received(packet_bytes[b]), ds_any_round_total(step.n_int, r)).s;
    std::memcpy(blob.data() + sb::region_off(st::R_CNG) + DS_STATE, &s, sizeof s);
    if (lyra_hip_import_streams(c, &ids[b], 1, blob.data(), LYRA_HIP_STATE_DECODER) != 0) return LYRA_HIP_EINVAL;
    q.sizes.push_back(sizes[b]);
    q.cn.push_back(s.fade == LOSSY_FADE ? 1 : 0);
  }
  g_flight[c].push_back(q);
  g_max_hops = R;
  ++g_begun;
  return 0;
}

int lyra_hip_decode_samples_streams_end(lyra_hip_ctx* c, int16_t* pcm, int32_t* is_noise, int32_t* is_comfort_noise) {
  if (g_flight[c].empty()) return LYRA_HIP_EINVAL;
  const Request q = g_flight[c].front();
  long total = 0;
  for (int32_t n : q.sizes) total += n;
  if (total > 0 && !pcm) return LYRA_HIP_EINVAL;
  g_flight[c].pop_front();
  long at = 0;
  for (size_t b = 0; b < q.sizes.size(); ++b) {   // every row says its own size, so a row in the wrong place shows
    for (int i = 0; i < q.sizes[b]; ++i) pcm[at++] = (int16_t)(q.sizes[b] + i % 7);
    if (is_noise) is_noise[b] = 1;
    if (is_comfort_noise) is_comfort_noise[b] = q.cn[b];
  }
  return 0;
}

int lyra_hip_decode_samples_streams_dev(lyra_hip_ctx*, const int32_t*, int, const uint8_t*, const int32_t*, const int32_t*,
                                        const int32_t*, int, int16_t*, long, const int32_t*, int32_t*, int32_t*) {
  return LYRA_HIP_EINVAL;   // (device pointers: not what a host class calls)
}
}
