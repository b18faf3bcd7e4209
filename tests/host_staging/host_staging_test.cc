// host_staging_test.cc -- a program of its own over lyra_amd/csrc/host_staging.h (no GPU, no library), built with
// -fsanitize=address,undefined by tests/test_pipeline_exclusion_cpu.py.  For every pipelined host-buffer form, at n = 1, 2, 7
// and 289262 rows (the top of the documented stream-id range) on a context of max_streams = n:
//   - no two arrays of a run overlap, and none reaches past the run's room;
//   - every device sub-buffer -- an array that is copied or handed to a kernel on its own -- starts on a 256-byte boundary (the
//     pipelines with one copy per direction have one sub-buffer per run, at 0);
//   - int32 arrays are 4-byte aligned, int16 arrays 2-byte aligned in the pinned runs (none of these pipelines stages an int64
//     array; the bridge's levels are bridge_staging_test.cc's);
//   - every array has at least the room it had when each family allocated its own buffers: the sizes below are literals taken
//     from those allocations;
//   - the room of a run is at most what was allocated then plus 256 bytes of padding per device sub-buffer, and is what a
//     computation in floating point gives (nothing wrapped).
// Prints one line per failure and "ok" at the end.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "host_staging.h"

using namespace host_staging;

namespace {

struct Arr {
  const char* name;
  size_t at, had, align;   // offset in its run, the bytes it had, required alignment of the offset
};
struct Run {
  const char* name;
  bool device;             // every array is a sub-buffer of its own: 256-byte boundaries
  size_t room;
  std::vector<Arr> arrs;
};

int failures = 0;

void fail(const char* what, const char* pipeline, const char* run, const char* arr, size_t n) {
  std::printf("FAIL %s: %s %s %s (n %zu)\n", what, pipeline, run, arr, n);
  ++failures;
}

void check(const char* pipeline, size_t n, const std::vector<Run>& runs) {
  for (const Run& r : runs) {
    std::vector<Arr> a = r.arrs;
    size_t had = 0;
    double had_f = 0;
    for (const Arr& x : a) {
      if (x.at % x.align) fail("alignment", pipeline, r.name, x.name, n);
      if (r.device && x.at % 256) fail("256-byte boundary", pipeline, r.name, x.name, n);
      if (x.at + x.had > r.room || x.at + x.had < x.at) fail("past the room", pipeline, r.name, x.name, n);
      had += x.had;
      had_f += (double)x.had;
    }
    std::sort(a.begin(), a.end(), [](const Arr& x, const Arr& y) { return x.at < y.at; });
    for (size_t i = 1; i < a.size(); ++i)
      if (a[i - 1].at + a[i - 1].had > a[i].at) fail("overlap", pipeline, r.name, a[i].name, n);
    if (r.room < had) fail("less room than before", pipeline, r.name, "", n);
    const size_t pad = r.device ? 256 * a.size() : 0;
    if (r.room > had + pad) fail("more room than before plus padding", pipeline, r.name, "", n);
    if (std::fabs((double)r.room - had_f) > (double)pad) fail("wrapped", pipeline, r.name, "", n);
  }
}

void check_all(size_t n) {
  const size_t m = n;   // max_streams
  {
    const Encode L = encode(m);   // pipe_slot_ensure
    check("encode", n,
          {{"h_in", false, L.room.h_in, {{"ids", L.h_ids, m * 4, 4}}},
           {"h_out", false, L.room.h_out, {{"packets", L.h_packets, m * 24, 1}, {"packet_bytes", L.h_packet_bytes, m * 4, 4}}},
           {"d_in", true, L.room.d_in, {{"ids", L.d_ids, m * 4, 4}, {"pcm", L.d_pcm, m * 960 * 2, 16}, {"pcm16", L.d_pcm16, m * 320 * 2, 16}}},
           {"d_out", true, L.room.d_out, {{"packets", L.d_packets, m * 24, 16}, {"packet_bytes", L.d_packet_bytes, m * 4, 4}}}});
  }
  {
    const Decode L = decode(m);   // lyra_hip_decode_begin
    check("decode", n,
          {{"h_in", false, L.room.h_in, {{"ids", L.h_ids, m * 4, 4}, {"packets", L.h_packets, m * 24, 1}}},
           {"h_out", false, L.room.h_out, {}},
           {"d_in", true, L.room.d_in, {{"ids", L.d_ids, m * 4, 4}, {"packets", L.d_packets, m * 24, 16}}},
           {"d_out", true, L.room.d_out, {{"pcm", L.d_pcm, m * 320 * 2, 16}}}});
  }
  for (size_t hops : {(size_t)1, (size_t)4}) {   // ds_host_begin: decode_samples, decode_samples_any
    const DecodeSamples L = decode_samples(m, hops);
    check(hops == 1 ? "decode_samples" : "decode_samples_any", n,
          {{"h_in", false, L.room.h_in,
            {{"ids", L.h_ids, m * 4, 4}, {"packet_bytes", L.h_packet_bytes, m * 4, 4}, {"packets", L.h_packets, m * 24, 1}}},
           {"h_out", false, L.room.h_out, {}},
           {"d_in", true, L.room.d_in,
            {{"ids", L.d_ids, m * 4, 4}, {"packet_bytes", L.d_packet_bytes, m * 4, 4}, {"packets", L.d_packets, m * 24, 16}}},
           {"d_out", true, L.room.d_out, {{"pcm", L.d_pcm, m * hops * 960 * 2, 16}}}});
  }
  {
    const EncodeStreams L = encode_streams(n, m);   // es_slot_ensure
    if (L.meta_bytes != n * 20) fail("the upload", "encode_streams", "meta", "", n);
    check("encode_streams", n,
          {{"h_in", false, L.room.h_in,
            {{"ids", L.ids, n * 4, 4}, {"rates", L.rates, n * 4, 4}, {"bits", L.bits, n * 4, 4}, {"dtx", L.dtx, n * 4, 4},
             {"offsets", L.offsets, n * 4, 4}}},
           {"h_out", false, L.room.h_out, {{"packets", L.h_packets, m * 24, 1}, {"packet_bytes", L.h_packet_bytes, m * 4, 4}}},
           {"d_in", true, L.room.d_in, {{"meta", L.d_meta, m * 5 * 4, 4}, {"pcm", L.d_pcm, m * 960 * 2, 16}}},
           {"d_out", true, L.room.d_out, {{"packets", L.d_packets, m * 23, 16}, {"packet_bytes", L.d_packet_bytes, m * 4, 4}}}});
  }
  {
    const DecodeStreams L = decode_streams(n, m);   // dstr_slot_ensure: one run per direction, the same on the host and the device
    if (L.in_bytes != n * 39) fail("the upload", "decode_streams", "in", "", n);
    const std::vector<Arr> in = {{"ids", L.ids, n * 4, 4}, {"packet_bytes", L.packet_bytes, n * 4, 4}, {"rates", L.rates, n * 4, 4},
                                 {"offsets", L.offsets, n * 4, 4}, {"packets", L.packets, n * 23, 1}};
    const std::vector<Arr> out = {{"is_noise", L.is_noise, n * 4, 4}, {"is_comfort_noise", L.is_comfort_noise, n * 4, 4},
                                  {"pcm", L.pcm, m * 960 * 2, 2}};
    check("decode_streams", n,
          {{"h_in", false, L.room.h_in, in}, {"h_out", false, L.room.h_out, out},
           {"d_in", true, L.room.d_in, {{"run", 0, m * (4 * 4 + 23), 16}}},
           {"d_out", true, L.room.d_out, {{"run", 0, m * (2 * 4 + 960 * 2), 16}}},
           {"d_in arrays", false, L.room.d_in, in}, {"d_out arrays", false, L.room.d_out, out}});
  }
  {
    const DecodeSamplesStreams L = decode_samples_streams(n);   // dss_slot_ensure: grows with the request
    if (L.in_bytes != n * 43) fail("the upload", "decode_samples_streams", "in", "", n);
    const std::vector<Arr> in = {{"ids", L.ids, n * 4, 4}, {"packet_bytes", L.packet_bytes, n * 4, 4}, {"rates", L.rates, n * 4, 4},
                                 {"sizes", L.sizes, n * 4, 4}, {"offsets", L.offsets, n * 4, 4}, {"packets", L.packets, n * 23, 1}};
    const std::vector<Arr> out = {{"is_noise", L.is_noise, n * 4, 4}, {"is_comfort_noise", L.is_comfort_noise, n * 4, 4},
                                  {"pcm", L.pcm, n * 3840 * 2, 2}};
    check("decode_samples_streams", n,
          {{"h_in", false, L.room.h_in, in}, {"h_out", false, L.room.h_out, out},
           {"d_in", true, L.room.d_in, {{"run", 0, n * (5 * 4 + 23), 16}}},
           {"d_out", true, L.room.d_out, {{"run", 0, n * (2 * 4 + 3840 * 2), 16}}},
           {"d_in arrays", false, L.room.d_in, in}, {"d_out arrays", false, L.room.d_out, out}});
  }
  {
    const Room R = bridge(m);   // brg_slot_ensure; where a tick's arrays lie in it: bridge_staging_test.cc
    const size_t in = (9 * m + 1) * 4 + m * 23, out = 7 * m * 4 + m * 23;
    check("bridge", n,
          {{"h_in", false, R.h_in, {{"run", 0, in, 4}}}, {"h_out", false, R.h_out, {{"run", 0, out, 8}}},
           {"d_in", true, R.d_in, {{"run", 0, in, 16}}}, {"d_out", true, R.d_out, {{"run", 0, out, 16}}}});
    for (bridge_staging::Kind kind : {bridge_staging::FULL, bridge_staging::SPEAKERS, bridge_staging::SHARED}) {
      const bridge_staging::Layout T = bridge_staging::layout(kind, n, kind == bridge_staging::SHARED ? m : 0);
      if (T.in_bytes > R.h_in || T.out_bytes > R.h_out) fail("a tick past the room", "bridge", "", "", n);
    }
  }
}

}  // namespace

int main() {
  int cases = 0;
  for (size_t n : {(size_t)1, (size_t)2, (size_t)7, (size_t)289262}) {
    check_all(n);
    ++cases;
  }
  std::printf("%d sizes, %d failures\n", cases, failures);
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
