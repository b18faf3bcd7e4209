// mixed_decoder_test.cc -- TEST INFRASTRUCTURE: the host logic of MixedBatchLyraDecoder (lyra_amd/host/lyra_mixed_decoder.cc)
// against the fake C ABI (fake_decode_streams_abi.cc + tests/host_stub/fake_lyra_hip_codec.cc).  A program of its own, built
// with -fsanitize=address,undefined by tests/test_decode_streams_cpu.py; exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fake_decode_streams_abi.h"
#include "lyra_mixed_decoder.h"

using chromemedia::codec::MixedBatchLyraDecoder;

#define CHECK_THAT(cond)                                                              \
  do {                                                                                \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; }  \
  } while (0)

int main() {
  const std::vector<int> rates = {32000, 8000, 48000, 16000, 8000, 32000};   // (not monotonic)
  const int n = static_cast<int>(rates.size());
  // creation: unsupported rate, channel count, no streams
  {
    std::vector<int> bad = rates;
    bad[2] = 44100;
    CHECK_THAT(MixedBatchLyraDecoder::Create(absl::MakeConstSpan(bad), 1, "model") == nullptr);
    bad[2] = 0;
    CHECK_THAT(MixedBatchLyraDecoder::Create(absl::MakeConstSpan(bad), 1, "model") == nullptr);
    CHECK_THAT(MixedBatchLyraDecoder::Create(absl::MakeConstSpan(rates), 2, "model") == nullptr);
    CHECK_THAT(MixedBatchLyraDecoder::Create(absl::Span<const int>(), 1, "model") == nullptr);
  }
  auto dec = MixedBatchLyraDecoder::Create(absl::MakeConstSpan(rates), 1, "model");
  CHECK_THAT(dec != nullptr);
  CHECK_THAT(dec->num_streams() == n && dec->hops_in_flight() == 0 && dec->frame_rate() == 50 && dec->num_channels() == 1);
  size_t total = 0;
  std::vector<size_t> start;
  for (int s = 0; s < n; ++s) {
    CHECK_THAT(dec->sample_rate_hz(s) == rates[s] && !dec->is_comfort_noise(s) && !dec->is_noise(s));
    start.push_back(total);
    total += rates[s] / 50;
  }
  CHECK_THAT(total == 640 + 160 + 960 + 320 + 160 + 640 && dec->hop_samples() == total);
  CHECK_THAT(!dec->is_comfort_noise(-1) && !dec->is_comfort_noise(n) && !dec->is_noise(n));
  CHECK_THAT(dec->sample_rate_hz(-1) == 0 && dec->sample_rate_hz(n) == 0);
  // packets whose first byte names stream and hop
  auto rows = [&](int t) {
    std::vector<uint8_t> r(static_cast<size_t>(n) * 23, 0xEE);
    for (int s = 0; s < n; ++s) r[s * 23] = static_cast<uint8_t>(16 * (t + 1) + s);
    return r;
  };
  // what a delivered hop must hold, from what the fake recorded for call number `call`
  auto matches = [&](const std::vector<int16_t>& pcm, long call) {
    const FakeDecodeStreamsCall& c = g_fake_dstr_calls[call];
    if (pcm.size() != total || c.total != static_cast<long>(total) || c.B != n) return false;
    for (int s = 0; s < n; ++s) {
      if (c.ids[s] != s || c.rates[s] != rates[s] || c.offsets[s] != static_cast<long>(start[s])) return false;
      for (int i = 0; i < rates[s] / 50; ++i)
        if (pcm[start[s] + i] != FakeDecodeStreamsSample(s, rates[s], call, c.bytes[s], c.first[s], i)) return false;
    }
    return true;
  };
  // calls that are refused as a whole and stage nothing: wrong shapes, an unknown length, a second packet for a stream
  {
    const std::vector<uint8_t> r = rows(0);
    const std::vector<int32_t> ok = {23, 0, 8, 15, 0, 8};
    CHECK_THAT(!dec->SetEncodedPackets(absl::MakeConstSpan(r.data(), r.size() - 1), absl::MakeConstSpan(ok)));
    CHECK_THAT(!dec->SetEncodedPackets(absl::MakeConstSpan(r), absl::MakeConstSpan(ok.data(), n - 1)));
    std::vector<int32_t> bad = ok;
    bad[5] = 16;   // streams 0, 2, 3 come before it: none of them may be staged
    CHECK_THAT(!dec->SetEncodedPackets(absl::MakeConstSpan(r), absl::MakeConstSpan(bad)));
    bad[5] = -1;
    CHECK_THAT(!dec->SetEncodedPackets(absl::MakeConstSpan(r), absl::MakeConstSpan(bad)));
    CHECK_THAT(!dec->SetEncodedPacket(1, absl::MakeConstSpan(r.data(), 9)));
    CHECK_THAT(!dec->SetEncodedPacket(1, absl::Span<const uint8_t>()));
    CHECK_THAT(!dec->SetEncodedPacket(-1, absl::MakeConstSpan(r.data(), 8)) && !dec->SetEncodedPacket(n, absl::MakeConstSpan(r.data(), 8)));
    CHECK_THAT(dec->SetEncodedPackets(absl::MakeConstSpan(r), absl::MakeConstSpan(ok)));
    // stream 4 is free, stream 0 is taken: the whole second call is refused, stream 4 stays without a packet
    const std::vector<int32_t> again = {8, 0, 0, 0, 15, 0};
    std::vector<uint8_t> other = rows(5);
    CHECK_THAT(!dec->SetEncodedPackets(absl::MakeConstSpan(other), absl::MakeConstSpan(again)));
    CHECK_THAT(!dec->SetEncodedPacket(3, absl::MakeConstSpan(other.data() + 3 * 23, 8)));
    CHECK_THAT(dec->SetEncodedPacket(1, absl::MakeConstSpan(other.data() + 1 * 23, 15)));   // a free stream, singly
    CHECK_THAT(g_fake_dstr_calls.empty());
    auto pcm = dec->DecodeHop();
    CHECK_THAT(pcm.has_value() && g_fake_dstr_calls.size() == 1 && g_fake_dstr_ends == 1 && dec->hops_in_flight() == 0);
    const FakeDecodeStreamsCall& c = g_fake_dstr_calls[0];
    const int want[] = {23, 15, 8, 15, 0, 8};
    for (int s = 0; s < n; ++s) {
      CHECK_THAT(c.bytes[s] == want[s]);
      CHECK_THAT(c.first[s] == (s == 4 ? 0 : s == 1 ? other[23] : r[s * 23]));
      CHECK_THAT(dec->is_comfort_noise(s) == (want[s] == 0) && dec->is_noise(s) == (want[s] == 8));
    }
    CHECK_THAT(matches(*pcm, 0));
  }
  // staging is consumed by the hop BEGUN, not by the one delivered; two deep, oldest first; a third is refused
  {
    const std::vector<uint8_t> r1 = rows(1), r2 = rows(2);
    const std::vector<int32_t> l1 = {8, 8, 0, 0, 23, 23}, l2 = {0, 15, 15, 0, 0, 8};
    CHECK_THAT(dec->SetEncodedPackets(absl::MakeConstSpan(r1), absl::MakeConstSpan(l1)));
    CHECK_THAT(dec->DecodeHopAsync() && dec->hops_in_flight() == 1);
    // hop 1 is in flight and undelivered: every stream is free again
    CHECK_THAT(dec->SetEncodedPackets(absl::MakeConstSpan(r2), absl::MakeConstSpan(l2)));
    CHECK_THAT(dec->DecodeHopAsync() && dec->hops_in_flight() == 2);
    CHECK_THAT(!dec->DecodeHopAsync() && dec->hops_in_flight() == 2);
    CHECK_THAT(!dec->DecodeHop().has_value() && dec->hops_in_flight() == 2);
    CHECK_THAT(g_fake_dstr_calls.size() == 3);
    for (int s = 0; s < n; ++s) {
      CHECK_THAT(g_fake_dstr_calls[1].bytes[s] == l1[s] && g_fake_dstr_calls[2].bytes[s] == l2[s]);
      CHECK_THAT(g_fake_dstr_calls[1].first[s] == (l1[s] ? r1[s * 23] : 0) && g_fake_dstr_calls[2].first[s] == (l2[s] ? r2[s * 23] : 0));
    }
    // flags are those of the last hop DELIVERED: still hop 0's
    CHECK_THAT(dec->is_comfort_noise(4) && !dec->is_comfort_noise(2));
    std::vector<int16_t> out(total);
    // a span of the wrong size is refused and consumes nothing
    CHECK_THAT(!dec->WaitDecoded(absl::Span<int16_t>(out.data(), total - 1)) && dec->hops_in_flight() == 2);
    CHECK_THAT(!dec->WaitDecoded(absl::Span<int16_t>()) && dec->hops_in_flight() == 2 && g_fake_dstr_ends == 1);
    CHECK_THAT(dec->WaitDecoded(absl::Span<int16_t>(out.data(), out.size())) && dec->hops_in_flight() == 1);
    CHECK_THAT(matches(out, 1));
    CHECK_THAT(dec->is_comfort_noise(2) && dec->is_comfort_noise(3) && !dec->is_comfort_noise(4) && dec->is_noise(0));
    CHECK_THAT(dec->WaitDecoded(absl::Span<int16_t>(out.data(), out.size())) && dec->hops_in_flight() == 0);
    CHECK_THAT(matches(out, 2));
    CHECK_THAT(dec->is_comfort_noise(0) && !dec->is_comfort_noise(1) && dec->is_noise(5) && !dec->is_noise(0));
    CHECK_THAT(!dec->WaitDecoded(absl::Span<int16_t>(out.data(), out.size())) && dec->hops_in_flight() == 0);
    CHECK_THAT(g_fake_dstr_ends == 3);
  }
  // a hop without any packet: every stream conceals
  {
    auto pcm = dec->DecodeHop();
    CHECK_THAT(pcm.has_value() && matches(*pcm, 3));
    for (int s = 0; s < n; ++s) CHECK_THAT(g_fake_dstr_calls[3].bytes[s] == 0 && dec->is_comfort_noise(s));
  }
  // a failing device call latches the object: everything is refused from then on
  {
    std::vector<int16_t> out(total);
    const std::vector<uint8_t> r = rows(4);
    const std::vector<int32_t> l = {8, 8, 8, 8, 8, 8};
    g_fake_dstr_fail_begin = true;
    CHECK_THAT(!dec->DecodeHopAsync() && dec->hops_in_flight() == 0);
    CHECK_THAT(!dec->DecodeHopAsync() && !dec->DecodeHop().has_value());
    CHECK_THAT(!dec->SetEncodedPackets(absl::MakeConstSpan(r), absl::MakeConstSpan(l)));
    CHECK_THAT(!dec->SetEncodedPacket(0, absl::MakeConstSpan(r.data(), 8)));
    CHECK_THAT(!dec->WaitDecoded(absl::Span<int16_t>(out.data(), out.size())));
    CHECK_THAT(g_fake_dstr_calls.size() == 4 && !g_fake_dstr_fail_begin);
    // ... and a failing end()
    auto d2 = MixedBatchLyraDecoder::Create(absl::MakeConstSpan(rates), 1, "model");
    CHECK_THAT(d2 != nullptr && d2->DecodeHopAsync() && d2->DecodeHopAsync());
    g_fake_dstr_fail_end = true;
    CHECK_THAT(!d2->WaitDecoded(absl::Span<int16_t>(out.data(), out.size())));
    CHECK_THAT(!d2->WaitDecoded(absl::Span<int16_t>(out.data(), out.size())) && !d2->DecodeHopAsync());
    CHECK_THAT(g_fake_dstr_ends == 4);
  }
  std::printf("ok\n");
  return 0;
}
