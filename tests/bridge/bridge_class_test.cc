// bridge_class_test.cc -- TEST INFRASTRUCTURE: the host logic of LyraConferenceBridge (lyra_amd/host/lyra_conference_bridge.cc)
// against the fake C ABI (fake_bridge_abi.cc + tests/host_stub/fake_lyra_hip_codec.cc).  A program of its own, built with
// -fsanitize=address,undefined by tests/test_bridge_cpu.py; exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fake_bridge_abi.h"
#include "lyra_conference_bridge.h"

using chromemedia::codec::BridgeStream;
using chromemedia::codec::LyraConferenceBridge;

#define CHECK_THAT(cond)                                                              \
  do {                                                                                \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; }  \
  } while (0)

int main() {
  const std::vector<BridgeStream> streams = {{3200, true}, {6000, false}, {9200, true}, {6000, true}, {3200, false}};
  const int n = static_cast<int>(streams.size());
  // creation: an unsupported bitrate, no streams
  {
    std::vector<BridgeStream> bad = streams;
    bad[3].bitrate = 8000;
    CHECK_THAT(LyraConferenceBridge::Create(absl::MakeConstSpan(bad), "model") == nullptr);
    CHECK_THAT(LyraConferenceBridge::Create(absl::Span<const BridgeStream>(), "model") == nullptr);
  }
  auto bridge = LyraConferenceBridge::Create(absl::MakeConstSpan(streams), "model", 0, true);
  CHECK_THAT(bridge != nullptr);
  CHECK_THAT(bridge->num_streams() == n && bridge->ticks_in_flight() == 0 && bridge->sample_rate_hz() == 16000);
  for (int s = 0; s < n; ++s)
    CHECK_THAT(bridge->room(s) == -1 && !bridge->muted(s) && bridge->bitrate(s) == streams[s].bitrate &&
               !bridge->is_comfort_noise(s) && !bridge->is_noise(s));
  CHECK_THAT(bridge->room(n) == -1 && bridge->bitrate(-1) == 0 && !bridge->is_comfort_noise(n) && !bridge->is_noise(-1));
  // settings of streams that do not exist, unsupported bitrates
  CHECK_THAT(!bridge->SetRoom(n, 0) && !bridge->SetRoom(-1, 0) && !bridge->SetMuted(n, true) && !bridge->set_bitrate(n, 3200));
  CHECK_THAT(!bridge->set_bitrate(1, 8000) && bridge->bitrate(1) == 6000 && !bridge->ResetStream(n));
  const std::vector<int> room_of = {4, 4, 9, 4, -1};
  for (int s = 0; s < n; ++s) CHECK_THAT(bridge->SetRoom(s, room_of[s]));
  CHECK_THAT(bridge->SetRoom(4, -7) && bridge->room(4) == -1);
  // packets whose first byte names stream and tick
  auto rows = [&](int t) {
    std::vector<uint8_t> r(static_cast<size_t>(n) * 23, 0xEE);
    for (int s = 0; s < n; ++s) r[s * 23] = static_cast<uint8_t>(16 * (t + 1) + s);
    return r;
  };
  // what a delivered tick must hold, from what the fake recorded for call number `call`
  auto matches = [&](const std::vector<uint8_t>& pk, const std::vector<int32_t>& len, long call) {
    const FakeBridgeCall& c = g_fake_bridge_calls[call];
    if (pk.size() != static_cast<size_t>(n) * 23 || len.size() != static_cast<size_t>(n) || c.B != n) return false;
    for (int s = 0; s < n; ++s) {
      if (c.ids[s] != s || len[s] != FakeBridgeLength(c.rooms[s], c.bits[s])) return false;
      if (len[s] && pk[s * 23] != FakeBridgeByte(s, call, c.rooms[s], c.muted[s], c.first[s])) return false;
    }
    return true;
  };
  // staging calls that are refused as a whole and stage nothing: wrong shapes, an unknown length, a second packet for a stream
  {
    const std::vector<uint8_t> r = rows(0);
    const std::vector<int32_t> ok = {23, 0, 8, 15, 0};
    CHECK_THAT(!bridge->SetEncodedPackets(absl::MakeConstSpan(r.data(), r.size() - 1), absl::MakeConstSpan(ok)));
    CHECK_THAT(!bridge->SetEncodedPackets(absl::MakeConstSpan(r), absl::MakeConstSpan(ok.data(), n - 1)));
    std::vector<int32_t> bad = ok;
    bad[4] = 16;   // streams 0, 2, 3 come before it: none of them may be staged
    CHECK_THAT(!bridge->SetEncodedPackets(absl::MakeConstSpan(r), absl::MakeConstSpan(bad)));
    bad[4] = -1;
    CHECK_THAT(!bridge->SetEncodedPackets(absl::MakeConstSpan(r), absl::MakeConstSpan(bad)));
    CHECK_THAT(!bridge->SetEncodedPacket(n, absl::MakeConstSpan(r.data(), 8)));
    CHECK_THAT(!bridge->SetEncodedPacket(1, absl::MakeConstSpan(r.data(), 9)));
    CHECK_THAT(!bridge->SetEncodedPacket(1, absl::Span<const uint8_t>()));
    CHECK_THAT(bridge->SetEncodedPacket(3, absl::MakeConstSpan(r.data() + 3 * 23, 15)));
    CHECK_THAT(!bridge->SetEncodedPacket(3, absl::MakeConstSpan(r.data() + 3 * 23, 15)));   // a second one
    CHECK_THAT(!bridge->SetEncodedPackets(absl::MakeConstSpan(r), absl::MakeConstSpan(ok)));   // stream 3 has one: nothing staged
    // a blocking tick: only stream 3's packet was ever staged
    auto got = bridge->Tick();
    CHECK_THAT(got.has_value() && g_fake_bridge_calls.size() == 1 && g_fake_bridge_ends == 1);
    const FakeBridgeCall& c = g_fake_bridge_calls[0];
    CHECK_THAT(c.bytes == (std::vector<int32_t>{0, 0, 0, 15, 0}) && c.first[3] == r[3 * 23]);
    CHECK_THAT(c.flags == LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE);
    CHECK_THAT(c.rooms == (std::vector<int32_t>{4, 4, 9, 4, -1}) && c.muted == (std::vector<int32_t>{0, 0, 0, 0, 0}));
    CHECK_THAT(c.bits == (std::vector<int32_t>{64, 120, 184, 120, 64}) && c.dtx == (std::vector<int32_t>{1, 0, 1, 1, 0}));
    CHECK_THAT(matches(got->first, got->second, 0) && got->second[4] == 0 && got->second[2] == 23);
    CHECK_THAT(bridge->is_comfort_noise(0) && !bridge->is_comfort_noise(3) && !bridge->is_noise(3));
  }
  // the staging was consumed: the next tick sees the packets staged after it
  {
    const std::vector<uint8_t> r = rows(1);
    const std::vector<int32_t> len = {8, 23, 0, 15, 8};
    CHECK_THAT(bridge->SetEncodedPackets(absl::MakeConstSpan(r), absl::MakeConstSpan(len)));
    auto got = bridge->Tick();
    CHECK_THAT(got.has_value() && g_fake_bridge_calls[1].bytes == len && matches(got->first, got->second, 1));
    CHECK_THAT(bridge->is_noise(0) && bridge->is_noise(4) && bridge->is_comfort_noise(2) && !bridge->is_comfort_noise(0));
  }
  // two ticks in flight, a third refused; room, mute and bitrate changes reach the next tick only
  std::vector<uint8_t> out(static_cast<size_t>(n) * 23);
  std::vector<int32_t> out_len(n);
  auto span_rows = [&]() { return absl::Span<uint8_t>(out.data(), out.size()); };
  auto span_len = [&]() { return absl::Span<int32_t>(out_len.data(), out_len.size()); };
  {
    CHECK_THAT(!bridge->WaitTick(span_rows(), span_len()));   // nothing in flight
    CHECK_THAT(bridge->TickAsync() && bridge->ticks_in_flight() == 1);                        // call 2
    CHECK_THAT(bridge->SetRoom(4, 9) && bridge->SetMuted(1, true) && bridge->set_bitrate(0, 9200));
    CHECK_THAT(!bridge->Tick().has_value());                  // refused while ticks are in flight
    CHECK_THAT(bridge->TickAsync() && bridge->ticks_in_flight() == 2);                        // call 3
    CHECK_THAT(!bridge->TickAsync() && bridge->ticks_in_flight() == 2 && g_fake_bridge_calls.size() == 4);
    CHECK_THAT(g_fake_bridge_calls[2].rooms[4] == -1 && g_fake_bridge_calls[2].muted[1] == 0 && g_fake_bridge_calls[2].bits[0] == 64);
    CHECK_THAT(g_fake_bridge_calls[3].rooms[4] == 9 && g_fake_bridge_calls[3].muted[1] == 1 && g_fake_bridge_calls[3].bits[0] == 184);
    // a WaitTick refused for a size consumes nothing
    const int ends = g_fake_bridge_ends;
    CHECK_THAT(!bridge->WaitTick(absl::Span<uint8_t>(out.data(), out.size() - 1), span_len()));
    CHECK_THAT(!bridge->WaitTick(span_rows(), absl::Span<int32_t>(out_len.data(), n - 1)));
    CHECK_THAT(bridge->ticks_in_flight() == 2 && g_fake_bridge_ends == ends);
    CHECK_THAT(bridge->WaitTick(span_rows(), span_len()) && matches(out, out_len, 2) && out_len[4] == 0 && out_len[0] == 8);
    CHECK_THAT(bridge->WaitTick(span_rows(), span_len()) && matches(out, out_len, 3) && out_len[4] == 8 && out_len[0] == 23);
    CHECK_THAT(bridge->ticks_in_flight() == 0 && bridge->room(4) == 9 && bridge->muted(1) && bridge->bitrate(0) == 9200);
  }
  // ResetStream: the slot's id goes to the device, a staged packet is dropped, the flags read false
  {
    const std::vector<uint8_t> r = rows(2);
    CHECK_THAT(bridge->SetEncodedPacket(2, absl::MakeConstSpan(r.data() + 2 * 23, 23)));
    CHECK_THAT(bridge->is_comfort_noise(2));
    CHECK_THAT(bridge->ResetStream(2) && g_fake_bridge_resets == (std::vector<int32_t>{2}) && !bridge->is_comfort_noise(2));
    CHECK_THAT(bridge->room(2) == 9 && bridge->bitrate(2) == 9200);
    auto got = bridge->Tick();
    CHECK_THAT(got.has_value() && g_fake_bridge_calls[4].bytes[2] == 0);
  }
  // the failed-call latch: a device call fails, every further call is refused
  {
    g_fake_bridge_fail_end = true;
    CHECK_THAT(bridge->TickAsync() && !bridge->WaitTick(span_rows(), span_len()));
    const size_t calls = g_fake_bridge_calls.size();
    const std::vector<uint8_t> r = rows(3);
    CHECK_THAT(!bridge->TickAsync() && !bridge->Tick().has_value() && !bridge->WaitTick(span_rows(), span_len()));
    CHECK_THAT(!bridge->SetEncodedPacket(0, absl::MakeConstSpan(r.data(), 8)) && !bridge->SetRoom(0, 1) && !bridge->SetMuted(0, true));
    CHECK_THAT(!bridge->set_bitrate(0, 3200) && !bridge->ResetStream(0) && g_fake_bridge_calls.size() == calls);
  }
  bridge.reset();   // (the fake's queue still holds the tick whose end() failed: a fresh bridge needs a fresh queue)
  {
    uint8_t pk[5 * 23];
    int32_t len[5], noise[5], cn[5];
    lyra_hip_ctx* any = reinterpret_cast<lyra_hip_ctx*>(pk);
    CHECK_THAT(lyra_hip_bridge_end(any, pk, len, noise, cn) == 0);
    auto b2 = LyraConferenceBridge::Create(absl::MakeConstSpan(streams), "model");
    CHECK_THAT(b2 != nullptr);
    g_fake_bridge_fail_begin = true;
    CHECK_THAT(!b2->TickAsync() && !b2->TickAsync() && b2->ticks_in_flight() == 0);
    auto b3 = LyraConferenceBridge::Create(absl::MakeConstSpan(streams), "model");
    g_fake_bridge_fail_reset = true;
    CHECK_THAT(b3 != nullptr && !b3->ResetStream(1) && !b3->Tick().has_value());
    auto b4 = LyraConferenceBridge::Create(absl::MakeConstSpan(streams), "model");
    CHECK_THAT(b4 != nullptr && b4->Tick().has_value() && g_fake_bridge_calls.back().flags == 0u);
  }
  std::printf("ok\n");
  return 0;
}
