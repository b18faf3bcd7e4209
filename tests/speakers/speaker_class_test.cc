// speaker_class_test.cc -- TEST INFRASTRUCTURE: the host logic of LyraSpeakerBridge (lyra_amd/host/lyra_speaker_bridge.cc) against
// the fake C ABI (fake_speakers_abi.cc next to tests/bridge/fake_bridge_abi.cc and tests/host_stub/fake_lyra_hip_codec.cc).  The
// staging, the settings and the latch are LyraConferenceBridge's and have their own program (tests/bridge); this one holds what
// the subclass adds: the ticks go through the selection's calls and through no other, max_speakers arrives, levels and
// speaker flags are those of the last tick DELIVERED.  A program of its own, built with -fsanitize=address,undefined by
// tests/test_speakers_cpu.py; exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fake_bridge_abi.h"
#include "fake_speakers_abi.h"
#include "lyra_speaker_bridge.h"

using chromemedia::codec::BridgeStream;
using chromemedia::codec::LyraConferenceBridge;
using chromemedia::codec::LyraSpeakerBridge;

#define CHECK_THAT(cond)                                                              \
  do {                                                                                \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; }  \
  } while (0)

int main() {
  const std::vector<BridgeStream> streams = {{3200, true}, {6000, false}, {9200, true}, {6000, true}, {3200, false}};
  const int n = static_cast<int>(streams.size());
  // creation: max_speakers outside 1..8, and what the base class refuses
  {
    for (int bad_n : {0, -1, 9}) CHECK_THAT(LyraSpeakerBridge::Create(absl::MakeConstSpan(streams), "model", 0, false, bad_n) == nullptr);
    std::vector<BridgeStream> bad = streams;
    bad[3].bitrate = 8000;
    CHECK_THAT(LyraSpeakerBridge::Create(absl::MakeConstSpan(bad), "model", 0, false, 3) == nullptr);
    CHECK_THAT(LyraSpeakerBridge::Create(absl::Span<const BridgeStream>(), "model", 0, false, 3) == nullptr);
    for (int ok_n : {1, 8}) {
      auto b = LyraSpeakerBridge::Create(absl::MakeConstSpan(streams), "model", 0, false, ok_n);
      CHECK_THAT(b != nullptr && b->max_speakers() == ok_n);
    }
  }
  auto bridge = LyraSpeakerBridge::Create(absl::MakeConstSpan(streams), "model", 0, true, 2);
  CHECK_THAT(bridge != nullptr && bridge->num_streams() == n && bridge->max_speakers() == 2);
  for (int s = -1; s <= n; ++s) CHECK_THAT(!bridge->is_speaker(s) && bridge->level(s) == 0);
  const std::vector<int> room_of = {4, 4, 9, 4, -1};
  for (int s = 0; s < n; ++s) CHECK_THAT(bridge->SetRoom(s, room_of[s]));
  CHECK_THAT(bridge->SetMuted(1, true));
  auto matches = [&](const std::vector<uint8_t>& pk, const std::vector<int32_t>& len, long call) {
    const FakeSpeakersCall& c = g_fake_speakers_calls[call];
    if (pk.size() != static_cast<size_t>(n) * 23 || len.size() != static_cast<size_t>(n) || c.B != n || c.max_speakers != 2) return false;
    for (int s = 0; s < n; ++s) {
      if (c.ids[s] != s || len[s] != FakeSpeakersLength(c.rooms[s], c.bits[s])) return false;
      if (len[s] && pk[s * 23] != FakeSpeakersByte(s, call, c.rooms[s], c.muted[s])) return false;
    }
    return true;
  };
  auto status_of = [&](long call) {   // levels and flags as of the tick delivered from call number `call`
    const FakeSpeakersCall& c = g_fake_speakers_calls[call];
    for (int s = 0; s < n; ++s) {
      if (bridge->level(s) != FakeSpeakersLevel(s, call, c.bytes[s])) return false;
      if (bridge->is_speaker(s) != (FakeSpeakersFlag(s, call, c.rooms[s], c.muted[s], 2) != 0)) return false;
    }
    return true;
  };
  std::vector<uint8_t> r(static_cast<size_t>(n) * 23, 0xEE);
  // a blocking tick goes through the selection's calls and through no other
  {
    const std::vector<int32_t> len = {8, 23, 0, 15, 8};
    CHECK_THAT(bridge->SetEncodedPackets(absl::MakeConstSpan(r), absl::MakeConstSpan(len)));
    auto got = bridge->Tick();
    CHECK_THAT(got.has_value() && g_fake_speakers_calls.size() == 1 && g_fake_speakers_ends == 1);
    CHECK_THAT(g_fake_bridge_calls.empty() && g_fake_bridge_ends == 0);
    const FakeSpeakersCall& c = g_fake_speakers_calls[0];
    CHECK_THAT(c.bytes == len && c.flags == LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE && c.max_speakers == 2);
    CHECK_THAT(c.rooms == (std::vector<int32_t>{4, 4, 9, 4, -1}) && c.muted == (std::vector<int32_t>{0, 1, 0, 0, 0}));
    CHECK_THAT(c.bits == (std::vector<int32_t>{64, 120, 184, 120, 64}) && c.dtx == (std::vector<int32_t>{1, 0, 1, 1, 0}));
    CHECK_THAT(matches(got->first, got->second, 0) && status_of(0));
    CHECK_THAT(bridge->is_speaker(0) && !bridge->is_speaker(1) && !bridge->is_speaker(4) && bridge->level(4) > bridge->level(0));
    CHECK_THAT(bridge->is_noise(0) && bridge->is_comfort_noise(2));   // the base class's flags come through the same end()
  }
  // two in flight: the status is that of the last tick DELIVERED, not of the last one begun
  std::vector<uint8_t> out(static_cast<size_t>(n) * 23);
  std::vector<int32_t> out_len(n);
  auto span_rows = [&]() { return absl::Span<uint8_t>(out.data(), out.size()); };
  auto span_len = [&]() { return absl::Span<int32_t>(out_len.data(), out_len.size()); };
  {
    CHECK_THAT(bridge->TickAsync() && bridge->SetMuted(0, true) && bridge->TickAsync() && !bridge->TickAsync());   // calls 1, 2
    CHECK_THAT(g_fake_speakers_calls.size() == 3 && status_of(0));
    CHECK_THAT(!bridge->WaitTick(absl::Span<uint8_t>(out.data(), out.size() - 1), span_len()) && status_of(0));
    CHECK_THAT(bridge->WaitTick(span_rows(), span_len()) && matches(out, out_len, 1) && status_of(1));
    CHECK_THAT(bridge->WaitTick(span_rows(), span_len()) && matches(out, out_len, 2) && status_of(2) && !bridge->is_speaker(0));
    CHECK_THAT(bridge->ticks_in_flight() == 0 && g_fake_speakers_ends == 3);
  }
  // ResetStream: the stream's level and flag read 0 / false until the next tick is delivered
  {
    CHECK_THAT(bridge->SetMuted(0, false) && bridge->Tick().has_value() && status_of(3) && bridge->level(3) != 0);
    CHECK_THAT(bridge->ResetStream(3) && g_fake_bridge_resets == (std::vector<int32_t>{3}));
    CHECK_THAT(bridge->level(3) == 0 && !bridge->is_speaker(3) && bridge->level(2) != 0);
    CHECK_THAT(bridge->Tick().has_value() && status_of(4));
  }
  // through a pointer to the base class the ticks are still the selection's (the demo holds it that way)
  {
    LyraConferenceBridge* base = bridge.get();
    const size_t calls = g_fake_speakers_calls.size();
    CHECK_THAT(base->Tick().has_value() && g_fake_speakers_calls.size() == calls + 1 && g_fake_bridge_calls.empty());
  }
  // the failed-call latch is the base class's and holds for this one's calls
  {
    g_fake_speakers_fail_end = true;
    CHECK_THAT(bridge->TickAsync() && !bridge->WaitTick(span_rows(), span_len()));
    const size_t calls = g_fake_speakers_calls.size();
    CHECK_THAT(!bridge->TickAsync() && !bridge->Tick().has_value() && !bridge->SetRoom(0, 1) && g_fake_speakers_calls.size() == calls);
  }
  bridge.reset();
  {
    uint8_t pk[5 * 23];
    int32_t len[5];
    lyra_hip_ctx* any = reinterpret_cast<lyra_hip_ctx*>(pk);
    CHECK_THAT(lyra_hip_speakers_end(any, pk, len, nullptr, nullptr, nullptr, nullptr) == 0);   // (a fresh queue)
    auto b2 = LyraSpeakerBridge::Create(absl::MakeConstSpan(streams), "model", 0, false, 8);
    g_fake_speakers_fail_begin = true;
    CHECK_THAT(b2 != nullptr && !b2->TickAsync() && !b2->TickAsync() && b2->ticks_in_flight() == 0);
    auto b3 = LyraSpeakerBridge::Create(absl::MakeConstSpan(streams), "model", 0, false, 8);
    CHECK_THAT(b3 != nullptr && b3->Tick().has_value() && g_fake_speakers_calls.back().flags == 0u &&
               g_fake_speakers_calls.back().max_speakers == 8);
  }
  CHECK_THAT(g_fake_bridge_calls.empty() && g_fake_bridge_ends == 0);
  std::printf("ok\n");
  return 0;
}
