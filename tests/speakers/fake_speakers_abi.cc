// fake_speakers_abi.cc -- TEST INFRASTRUCTURE: a CPU stand-in for the calls of include/lyra_hip_speakers.h, linked next to
// tests/bridge/fake_bridge_abi.cc and tests/host_stub/fake_lyra_hip_codec.cc (which stay as they are).  It records what each
// begin() received and answers with the formulas of fake_speakers_abi.h; a row without a packet is "comfort noise", a row with
// an 8-byte packet is "noise", as in the bridge's fake.  Never linked into the product.
#include <cstdint>
#include <deque>
#include <vector>

#include "fake_speakers_abi.h"

std::vector<FakeSpeakersCall> g_fake_speakers_calls;
int g_fake_speakers_ends = 0;
bool g_fake_speakers_fail_begin = false, g_fake_speakers_fail_end = false;

namespace {
struct Result { std::vector<uint8_t> rows; std::vector<int32_t> lens, noise, cn, speaker; std::vector<int64_t> levels; };
std::deque<Result> g_queue;
}  // namespace

extern "C" {

int lyra_hip_speakers_mix_dev(lyra_hip_ctx*, const int16_t*, int, const int32_t*, const int32_t*, int, int, const int32_t*,
                              const int32_t*, int, int16_t*, int64_t*, int32_t*) {
  return -1;   // (device buffers)
}
int lyra_hip_speakers_tick_dev(lyra_hip_ctx*, const lyra_hip_speakers_tick*) { return -1; }

int lyra_hip_speakers_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets, const int32_t* packet_bytes,
                            const int32_t* rooms, const int32_t* muted, unsigned flags, const int32_t* num_bits,
                            const int32_t* dtx, int max_speakers) {
  if (g_fake_speakers_fail_begin) { g_fake_speakers_fail_begin = false; return -2; }
  if (!c || !ids || B <= 0 || !packets || !packet_bytes || !rooms || !num_bits || g_queue.size() >= 2 || max_speakers < 1 ||
      max_speakers > LYRA_HIP_SPEAKERS_MAX)
    return -1;
  FakeSpeakersCall call;
  call.B = B;
  call.flags = flags;
  call.max_speakers = max_speakers;
  Result r;
  r.rows.assign(static_cast<size_t>(B) * 23, 0);
  const long number = static_cast<long>(g_fake_speakers_calls.size());
  for (int b = 0; b < B; ++b) {
    const int nb = packet_bytes[b], m = muted ? muted[b] : 0;
    call.ids.push_back(ids[b]);
    call.bytes.push_back(nb);
    call.rooms.push_back(rooms[b]);
    call.muted.push_back(m);
    call.bits.push_back(num_bits[b]);
    call.dtx.push_back(dtx ? dtx[b] : 0);
    const int len = FakeSpeakersLength(rooms[b], num_bits[b]);
    r.lens.push_back(len);
    if (len) r.rows[static_cast<size_t>(b) * 23] = FakeSpeakersByte(ids[b], number, rooms[b], m);
    r.noise.push_back(nb == 8 ? 1 : 0);
    r.cn.push_back(nb == 0 ? 1 : 0);
    r.levels.push_back(FakeSpeakersLevel(ids[b], number, nb));
    r.speaker.push_back(FakeSpeakersFlag(ids[b], number, rooms[b], m, max_speakers));
  }
  g_fake_speakers_calls.push_back(call);
  g_queue.push_back(r);
  return 0;
}

int lyra_hip_speakers_end(lyra_hip_ctx* c, uint8_t* out_packets, int32_t* out_packet_bytes, int32_t* is_noise,
                          int32_t* is_comfort_noise, int64_t* levels, int32_t* is_speaker) {
  if (g_fake_speakers_fail_end) { g_fake_speakers_fail_end = false; return -2; }
  if (!c || !out_packets || !out_packet_bytes || g_queue.empty()) return -1;
  const Result& r = g_queue.front();
  for (size_t i = 0; i < r.rows.size(); ++i) out_packets[i] = r.rows[i];
  for (size_t i = 0; i < r.lens.size(); ++i) {
    out_packet_bytes[i] = r.lens[i];
    if (is_noise) is_noise[i] = r.noise[i];
    if (is_comfort_noise) is_comfort_noise[i] = r.cn[i];
    if (levels) levels[i] = r.levels[i];
    if (is_speaker) is_speaker[i] = r.speaker[i];
  }
  g_queue.pop_front();
  ++g_fake_speakers_ends;
  return 0;
}

}  // extern "C"
