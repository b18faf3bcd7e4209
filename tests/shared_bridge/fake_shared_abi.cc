// fake_shared_abi.cc -- TEST INFRASTRUCTURE: a CPU stand-in for the calls of include/lyra_hip_shared_bridge.h, linked next to
// tests/bridge/fake_bridge_abi.cc and tests/host_stub/fake_lyra_hip_codec.cc (which stay as they are).  It holds begin() to
// what the library holds it to (labels strictly ascending and exactly those present, encoder ids distinct), records what it
// received and answers with the formulas of fake_shared_abi.h; a row without a packet is "comfort noise", a row with an 8-byte
// packet is "noise", as in the bridge's fake.  Never linked into the product.
#include <algorithm>
#include <cstdint>
#include <deque>
#include <set>
#include <vector>

#include "fake_shared_abi.h"

std::vector<FakeSharedCall> g_fake_shared_calls;
std::vector<int32_t> g_fake_shared_room_resets;
int g_fake_shared_ends = 0;
bool g_fake_shared_fail_begin = false, g_fake_shared_fail_end = false;

namespace {
struct Answer { std::vector<uint8_t> rows; std::vector<int32_t> lens, noise, cn, speaker, slot; std::vector<int64_t> levels; };
std::deque<Answer> g_pending;
}  // namespace

extern "C" {

int lyra_hip_shared_mix_dev(lyra_hip_ctx*, const int16_t*, const int32_t*, int, const int32_t*, const int32_t*, int, int,
                            const int32_t*, const int32_t*, int, const int32_t*, int32_t*, int, int16_t*, int64_t*, int32_t*,
                            int32_t*) {
  return -1;   // (device buffers)
}
int lyra_hip_shared_tick_dev(lyra_hip_ctx*, const lyra_hip_shared_tick*) { return -1; }

int lyra_hip_shared_begin(lyra_hip_ctx* c, const int32_t* ids, int B, const uint8_t* packets, const int32_t* packet_bytes,
                          const int32_t* rooms, const int32_t* muted, unsigned flags, int max_speakers, const int32_t* room_labels,
                          int n_rooms, const int32_t* enc_ids, const int32_t* enc_bits, const int32_t* enc_dtx) {
  if (g_fake_shared_fail_begin) { g_fake_shared_fail_begin = false; return -2; }
  if (!c || !ids || B <= 0 || !packets || !packet_bytes || !rooms || g_pending.size() >= 2 || max_speakers < 1 ||
      max_speakers > LYRA_HIP_SPEAKERS_MAX || n_rooms < 0 || (n_rooms > 0 && (!room_labels || !enc_ids || !enc_bits)))
    return -1;
  std::set<int32_t> present;
  for (int b = 0; b < B; ++b)
    if (rooms[b] >= 0) present.insert(rooms[b]);
  if (std::vector<int32_t>(present.begin(), present.end()) != std::vector<int32_t>(room_labels, room_labels + n_rooms)) return -1;
  const int per = 1 + max_speakers, E = n_rooms * per;
  if (std::set<int32_t>(enc_ids, enc_ids + E).size() != static_cast<size_t>(E)) return -1;
  FakeSharedCall call;
  call.B = B;
  call.flags = flags;
  call.max_speakers = max_speakers;
  call.n_rooms = n_rooms;
  call.labels.assign(room_labels, room_labels + n_rooms);
  call.enc_ids.assign(enc_ids, enc_ids + E);
  call.enc_bits.assign(enc_bits, enc_bits + E);
  for (int e = 0; e < E; ++e) call.enc_dtx.push_back(enc_dtx ? enc_dtx[e] : 0);
  Answer r;
  r.rows.assign(static_cast<size_t>(B) * 23, 0);
  const long number = static_cast<long>(g_fake_shared_calls.size());
  std::vector<int> seen(static_cast<size_t>(n_rooms), 0);   // members of each room so far
  for (int b = 0; b < B; ++b) {
    const int nb = packet_bytes[b], m = muted ? muted[b] : 0;
    call.ids.push_back(ids[b]);
    call.bytes.push_back(nb);
    call.rooms.push_back(rooms[b]);
    call.muted.push_back(m);
    int slot = -1, len = 0;
    if (rooms[b] >= 0) {
      const int r_at = static_cast<int>(std::lower_bound(call.labels.begin(), call.labels.end(), rooms[b]) - call.labels.begin());
      const int k = seen[r_at]++;
      if (k < max_speakers && !m) slot = k;
      const int e = r_at * per + 1 + slot;
      len = FakeSharedLength(rooms[b], call.enc_bits[e]);
      r.rows[static_cast<size_t>(b) * 23] = FakeSharedByte(call.enc_ids[e], number, call.enc_dtx[e]);
    }
    r.lens.push_back(len);
    r.slot.push_back(slot);
    r.speaker.push_back(slot >= 0 ? 1 : 0);
    r.noise.push_back(nb == 8 ? 1 : 0);
    r.cn.push_back(nb == 0 ? 1 : 0);
    r.levels.push_back(FakeSharedLevel(ids[b], number, nb));
  }
  g_fake_shared_calls.push_back(call);
  g_pending.push_back(r);
  return 0;
}

int lyra_hip_shared_end(lyra_hip_ctx* c, uint8_t* out_packets, int32_t* out_packet_bytes, int32_t* is_noise,
                        int32_t* is_comfort_noise, int64_t* levels, int32_t* is_speaker, int32_t* slot_of) {
  if (g_fake_shared_fail_end) { g_fake_shared_fail_end = false; return -2; }
  if (!c || !out_packets || !out_packet_bytes || g_pending.empty()) return -1;
  const Answer& r = g_pending.front();
  std::copy(r.rows.begin(), r.rows.end(), out_packets);
  std::copy(r.lens.begin(), r.lens.end(), out_packet_bytes);
  if (is_noise) std::copy(r.noise.begin(), r.noise.end(), is_noise);
  if (is_comfort_noise) std::copy(r.cn.begin(), r.cn.end(), is_comfort_noise);
  if (levels) std::copy(r.levels.begin(), r.levels.end(), levels);
  if (is_speaker) std::copy(r.speaker.begin(), r.speaker.end(), is_speaker);
  if (slot_of) std::copy(r.slot.begin(), r.slot.end(), slot_of);
  g_pending.pop_front();
  ++g_fake_shared_ends;
  return 0;
}

int lyra_hip_shared_reset_rooms(lyra_hip_ctx* c, const int32_t* room_labels, int n) {
  if (!c || n < 0 || (n > 0 && !room_labels)) return -1;
  g_fake_shared_room_resets.insert(g_fake_shared_room_resets.end(), room_labels, room_labels + n);
  return 0;
}

}  // extern "C"
