// shared_class_test.cc -- TEST INFRASTRUCTURE: the host logic of LyraSharedBridge (lyra_amd/host/lyra_shared_bridge.cc) against
// the fake C ABI (fake_shared_abi.cc next to tests/bridge/fake_bridge_abi.cc and tests/host_stub/fake_lyra_hip_codec.cc).  The
// staging, the mutes and the latch are LyraConferenceBridge's and have their own program (tests/bridge); this one holds what the
// subclass adds: the ticks go through the shared-encoder calls and through no other; the labels are those present, ascending;
// every room's 1 + N encoder rows lie above the participants' ids and carry the ROOM's bitrate and DTX; levels, speaker flags
// and slots are those of the last tick DELIVERED; ResetRoom resets the room's table row and its encoder streams.  A program of
// its own, built with -fsanitize=address,undefined by tests/test_shared_bridge_cpu.py; exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fake_bridge_abi.h"
#include "fake_shared_abi.h"
#include "lyra_shared_bridge.h"

using chromemedia::codec::BridgeStream;
using chromemedia::codec::LyraConferenceBridge;
using chromemedia::codec::LyraSharedBridge;

#define CHECK_THAT(cond)                                                              \
  do {                                                                                \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; }  \
  } while (0)

int main() {
  const std::vector<BridgeStream> streams = {{3200, true}, {6000, false}, {9200, true}, {6000, true}, {3200, false}, {9200, false}};
  const int n = static_cast<int>(streams.size()), N = 2, kRooms = 10;
  const auto all = absl::MakeConstSpan(streams);
  {
    for (int bad_n : {0, -1, 9}) CHECK_THAT(LyraSharedBridge::Create(all, "model", 0, false, bad_n, kRooms) == nullptr);
    for (int bad_rooms : {0, -3}) CHECK_THAT(LyraSharedBridge::Create(all, "model", 0, false, N, bad_rooms) == nullptr);
    CHECK_THAT(LyraSharedBridge::Create(all, "model", 0, false, N, kRooms, {8000, false}) == nullptr);
    CHECK_THAT(LyraSharedBridge::Create(absl::Span<const BridgeStream>(), "model", 0, false, N, kRooms) == nullptr);
  }
  auto bridge = LyraSharedBridge::Create(all, "model", 0, true, N, kRooms, {9200, true});
  CHECK_THAT(bridge != nullptr && bridge->num_streams() == n && bridge->max_speakers() == N && bridge->max_rooms() == kRooms);
  for (int s = -1; s <= n; ++s) CHECK_THAT(bridge->slot(s) == -1 && !bridge->is_speaker(s) && bridge->level(s) == 0);
  CHECK_THAT(bridge->room_bitrate(4) == 9200 && bridge->room_dtx(4) && bridge->room_bitrate(kRooms) == 0 && !bridge->room_dtx(-1));
  // rooms: labels 4 and 9 (not contiguous), stream 4 in no room; a label at or above max_rooms is refused
  const std::vector<int> room_of = {4, 4, 9, 4, -1, 9};
  for (int s = 0; s < n; ++s) CHECK_THAT(bridge->SetRoom(s, room_of[s]));
  CHECK_THAT(!bridge->SetRoom(0, kRooms) && !bridge->SetRoom(n, 1) && bridge->room(0) == 4);
  CHECK_THAT(bridge->SetRoomBitrate(4, 3200) && bridge->SetRoomDtx(4, false) && !bridge->SetRoomBitrate(4, 8000) &&
             !bridge->SetRoomBitrate(kRooms, 3200) && !bridge->SetRoomDtx(-1, true) && bridge->room_bitrate(4) == 3200);
  CHECK_THAT(bridge->SetMuted(1, true) && bridge->set_bitrate(0, 6000));   // (a listener's own bitrate: accepted by the base, unused)
  const int per = 1 + N;
  auto sane = [&](long number) {   // what every begin() must have carried
    const FakeSharedCall& c = g_fake_shared_calls[number];
    if (c.B != n || c.max_speakers != N || c.labels != std::vector<int32_t>{4, 9} || c.n_rooms != 2) return false;
    for (int r = 0; r < 2; ++r)
      for (int k = 0; k < per; ++k) {
        const int e = r * per + k, room = c.labels[r];
        if (c.enc_ids[e] != n + room * per + k || c.enc_ids[e] < n) return false;
        if (c.enc_bits[e] != bridge->room_bitrate(room) / 50 || c.enc_dtx[e] != (bridge->room_dtx(room) ? 1 : 0)) return false;
      }
    return true;
  };
  auto delivered = [&](const std::vector<uint8_t>& pk, const std::vector<int32_t>& len, long number) {
    const FakeSharedCall& c = g_fake_shared_calls[number];
    std::vector<int> seen(2, 0);
    for (int s = 0; s < n; ++s) {
      int slot = -1, want_len = 0;
      uint8_t want = 0;
      if (c.rooms[s] >= 0) {
        const int r = c.rooms[s] == 4 ? 0 : 1, k = seen[r]++;
        if (k < N && !c.muted[s]) slot = k;
        const int e = r * per + 1 + slot;
        want_len = FakeSharedLength(c.rooms[s], c.enc_bits[e]);
        want = FakeSharedByte(c.enc_ids[e], number, c.enc_dtx[e]);
      }
      if (len[s] != want_len || pk[static_cast<size_t>(s) * 23] != want) return false;
      if (bridge->slot(s) != slot || bridge->is_speaker(s) != (slot >= 0) || bridge->level(s) != FakeSharedLevel(s, number, c.bytes[s]))
        return false;
    }
    return true;
  };
  std::vector<uint8_t> r(static_cast<size_t>(n) * 23, 0xEE);
  // a blocking tick goes through the shared-encoder calls and through no other
  {
    const std::vector<int32_t> len = {8, 23, 0, 15, 8, 23};
    CHECK_THAT(bridge->SetEncodedPackets(absl::MakeConstSpan(r), absl::MakeConstSpan(len)));
    auto got = bridge->Tick();
    CHECK_THAT(got.has_value() && g_fake_shared_calls.size() == 1 && g_fake_shared_ends == 1);
    CHECK_THAT(g_fake_bridge_calls.empty() && g_fake_bridge_ends == 0);
    const FakeSharedCall& c = g_fake_shared_calls[0];
    CHECK_THAT(c.bytes == len && c.flags == LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE && sane(0));
    CHECK_THAT(c.rooms == (std::vector<int32_t>{4, 4, 9, 4, -1, 9}) && c.muted == (std::vector<int32_t>{0, 1, 0, 0, 0, 0}));
    CHECK_THAT(c.enc_bits == (std::vector<int32_t>{64, 64, 64, 184, 184, 184}) && c.enc_dtx == (std::vector<int32_t>{0, 0, 0, 1, 1, 1}));
    CHECK_THAT(delivered(got->first, got->second, 0));
    // rows 1 (muted) and 3 (third member) of room 4 hear the same mix: the same packet
    CHECK_THAT(bridge->slot(0) == 0 && bridge->slot(1) == -1 && bridge->slot(3) == -1 && got->first[1 * 23] == got->first[3 * 23]);
    CHECK_THAT(got->second[4] == 0 && bridge->is_noise(0) && bridge->is_comfort_noise(2));
  }
  // two in flight: settings reach the NEXT tick begun, the status is that of the last tick DELIVERED
  std::vector<uint8_t> out(static_cast<size_t>(n) * 23);
  std::vector<int32_t> out_len(n);
  auto span_rows = [&]() { return absl::Span<uint8_t>(out.data(), out.size()); };
  auto span_len = [&]() { return absl::Span<int32_t>(out_len.data(), out_len.size()); };
  {
    CHECK_THAT(bridge->TickAsync() && sane(1) && bridge->SetRoomBitrate(9, 6000) && bridge->SetMuted(0, true) && bridge->TickAsync() &&
               sane(2) && !bridge->TickAsync());
    CHECK_THAT(g_fake_shared_calls[1].enc_bits[3] == 184 && g_fake_shared_calls[2].enc_bits[3] == 120);
    CHECK_THAT(!bridge->WaitTick(absl::Span<uint8_t>(out.data(), out.size() - 1), span_len()) && bridge->slot(0) == 0);
    CHECK_THAT(bridge->WaitTick(span_rows(), span_len()) && delivered(out, out_len, 1) && bridge->slot(0) == 0);
    CHECK_THAT(bridge->WaitTick(span_rows(), span_len()) && delivered(out, out_len, 2) && bridge->slot(0) == -1);
    CHECK_THAT(bridge->ticks_in_flight() == 0 && g_fake_shared_ends == 3);
  }
  // a room that empties leaves the labels; ResetStream and ResetRoom
  {
    CHECK_THAT(bridge->SetRoom(2, -1) && bridge->SetRoom(5, 4) && bridge->Tick().has_value());
    CHECK_THAT(g_fake_shared_calls[3].labels == std::vector<int32_t>{4} && g_fake_shared_calls[3].enc_ids.size() == 3u);
    CHECK_THAT(bridge->SetRoom(2, 9) && bridge->SetRoom(5, 9) && bridge->Tick().has_value() && sane(4) && bridge->level(3) != 0);
    CHECK_THAT(bridge->ResetStream(3) && g_fake_bridge_resets == (std::vector<int32_t>{3}));
    CHECK_THAT(bridge->level(3) == 0 && bridge->slot(3) == -1 && !bridge->is_speaker(3) && bridge->level(2) != 0);
    CHECK_THAT(bridge->ResetRoom(9) && !bridge->ResetRoom(kRooms) && g_fake_shared_room_resets == (std::vector<int32_t>{9}));
    CHECK_THAT(g_fake_bridge_resets == (std::vector<int32_t>{3, n + 9 * per, n + 9 * per + 1, n + 9 * per + 2}));
    CHECK_THAT(bridge->Tick().has_value() && sane(5));
  }
  // through a pointer to the base class the ticks are still this class's; the base SetRoom lets any label through, the tick refuses
  {
    LyraConferenceBridge* base = bridge.get();
    const size_t calls = g_fake_shared_calls.size();
    CHECK_THAT(base->Tick().has_value() && g_fake_shared_calls.size() == calls + 1 && g_fake_bridge_calls.empty());
  }
  // the failed-call latch is the base class's and holds for this one's calls
  {
    g_fake_shared_fail_end = true;
    CHECK_THAT(bridge->TickAsync() && !bridge->WaitTick(span_rows(), span_len()));
    const size_t calls = g_fake_shared_calls.size();
    CHECK_THAT(!bridge->TickAsync() && !bridge->Tick().has_value() && !bridge->SetRoom(0, 1) && g_fake_shared_calls.size() == calls);
  }
  bridge.reset();
  {
    uint8_t pk[6 * 23];
    int32_t len[6];
    lyra_hip_ctx* any = reinterpret_cast<lyra_hip_ctx*>(pk);
    CHECK_THAT(lyra_hip_shared_end(any, pk, len, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);   // (a fresh queue)
    auto b2 = LyraSharedBridge::Create(all, "model", 0, false, 8, 1);
    g_fake_shared_fail_begin = true;
    CHECK_THAT(b2 != nullptr && !b2->TickAsync() && !b2->TickAsync() && b2->ticks_in_flight() == 0);
    auto b3 = LyraSharedBridge::Create(all, "model", 0, false, 8, 1);
    CHECK_THAT(b3 != nullptr && b3->Tick().has_value() && g_fake_shared_calls.back().flags == 0u &&
               g_fake_shared_calls.back().max_speakers == 8 && g_fake_shared_calls.back().labels.empty());
    LyraConferenceBridge* base = b3.get();
    CHECK_THAT(base->SetRoom(0, 5) && !b3->Tick().has_value());   // room 5 of a bridge with one room: refused before the device
  }
  CHECK_THAT(g_fake_bridge_calls.empty() && g_fake_bridge_ends == 0);
  std::printf("ok\n");
  return 0;
}
