// mixed_encoder_test.cc -- TEST INFRASTRUCTURE: the host logic of MixedBatchLyraEncoder (lyra_amd/host/lyra_mixed_encoder.cc)
// against the fake C ABI (fake_encode_streams_abi.cc + tests/host_stub/fake_lyra_hip_codec.cc).  A program of its own, built
// with -fsanitize=address,undefined by tests/test_encode_streams_cpu.py; exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fake_encode_streams_abi.h"
#include "lyra_mixed_encoder.h"

using chromemedia::codec::MixedBatchLyraEncoder;
using Params = MixedBatchLyraEncoder::EncoderParams;

#define CHECK_THAT(cond)                                                              \
  do {                                                                                \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; }  \
  } while (0)

int main() {
  const std::vector<Params> params = {{8000, 3200, true},  {48000, 9200, false}, {16000, 6000, true},
                                      {32000, 3200, false}, {16000, 9200, true},  {8000, 6000, false}};
  const int n = static_cast<int>(params.size());
  // creation: unsupported rate, bitrate, channel count, no streams
  {
    std::vector<Params> bad = params;
    bad[3].sample_rate_hz = 44100;
    CHECK_THAT(MixedBatchLyraEncoder::Create(absl::MakeConstSpan(bad), 1, "model") == nullptr);
    bad = params;
    bad[5].bitrate = 8000;
    CHECK_THAT(MixedBatchLyraEncoder::Create(absl::MakeConstSpan(bad), 1, "model") == nullptr);
    CHECK_THAT(MixedBatchLyraEncoder::Create(absl::MakeConstSpan(params), 2, "model") == nullptr);
    CHECK_THAT(MixedBatchLyraEncoder::Create(absl::Span<const Params>(), 1, "model") == nullptr);
  }
  auto enc = MixedBatchLyraEncoder::Create(absl::MakeConstSpan(params), 1, "model");
  CHECK_THAT(enc != nullptr);
  CHECK_THAT(enc->num_streams() == n && enc->hops_in_flight() == 0);
  size_t total = 0;
  std::vector<size_t> start;
  for (int s = 0; s < n; ++s) {
    CHECK_THAT(enc->sample_rate_hz(s) == params[s].sample_rate_hz && enc->bitrate(s) == params[s].bitrate &&
               enc->enable_dtx(s) == params[s].enable_dtx);
    start.push_back(total);
    total += params[s].sample_rate_hz / 50;
  }
  // a hop whose rows are marked at both ends; stream 2 (DTX) and stream 3 (no DTX) are quiet
  auto hop = [&](int t) {
    std::vector<int16_t> a(total);
    for (int s = 0; s < n; ++s) {
      const size_t len = params[s].sample_rate_hz / 50;
      for (size_t i = 0; i < len; ++i) a[start[s] + i] = (s == 2 || s == 3) ? (int16_t)((i + t) % 5) : (int16_t)(1000 + 37 * i + t);
      a[start[s]] = (int16_t)(100 * (s + 1) + t);
      a[start[s] + len - 1] = (int16_t)(-100 * (s + 1) - t);
    }
    a[start[2]] = 3; a[start[2] + 319] = -3; a[start[3]] = 4; a[start[3] + 639] = -4;
    return a;
  };
  // wrong total sizes are refused, nothing reaches the device
  {
    std::vector<int16_t> a = hop(0);
    a.push_back(0);
    CHECK_THAT(!enc->Encode(absl::MakeConstSpan(a)).has_value());
    CHECK_THAT(!enc->EncodeAsync(absl::MakeConstSpan(a.data(), total - 1)));
    CHECK_THAT(!enc->EncodeAsync(absl::MakeConstSpan(a.data(), (size_t)n * 320)));
    CHECK_THAT(!enc->EncodeAsync(absl::Span<const int16_t>()));
    CHECK_THAT(g_fake_streams_calls.empty() && enc->hops_in_flight() == 0);
  }
  // blocking hop: what the fake received
  {
    const std::vector<int16_t> a = hop(0);
    auto pk = enc->Encode(absl::MakeConstSpan(a));
    CHECK_THAT(pk.has_value() && pk->size() == (size_t)n * 23);
    CHECK_THAT(g_fake_streams_calls.size() == 1 && g_fake_streams_ends == 1);
    const FakeStreamsCall& c = g_fake_streams_calls[0];
    CHECK_THAT(c.B == n && !c.dtx_null && c.total == (long)total);
    const int want_bits[] = {64, 184, 120, 64, 184, 120};
    for (int s = 0; s < n; ++s) {
      CHECK_THAT(c.ids[s] == s && c.rates[s] == params[s].sample_rate_hz && c.bits[s] == want_bits[s]);
      CHECK_THAT(c.dtx[s] == (params[s].enable_dtx ? 1 : 0));
      CHECK_THAT(c.offsets[s] == (long)start[s]);
      CHECK_THAT(c.first[s] == a[start[s]] && c.last[s] == a[start[s] + params[s].sample_rate_hz / 50 - 1]);
    }
    // lengths: the DTX stream's quiet hop is the empty packet, the quiet stream without DTX sends a packet
    const int want_len[] = {8, 23, 0, 8, 23, 15};
    for (int s = 0; s < n; ++s) {
      CHECK_THAT(enc->packet_lengths()[s] == want_len[s]);
      for (int j = want_len[s]; j < 23; ++j) CHECK_THAT((*pk)[s * 23 + j] == 0);
    }
  }
  // set_bitrate: refused for unsupported values and streams that do not exist; takes effect on the next hop begun
  CHECK_THAT(!enc->set_bitrate(0, 8000) && !enc->set_bitrate(-1, 3200) && !enc->set_bitrate(n, 3200));
  CHECK_THAT(enc->bitrate(0) == 3200);
  CHECK_THAT(enc->set_bitrate(0, 9200) && enc->set_bitrate(4, 3200) && enc->bitrate(0) == 9200 && enc->bitrate(4) == 3200);
  // two hops in flight, a refused third, Encode() refused meanwhile, delivery oldest first
  {
    const std::vector<int16_t> a1 = hop(1), a2 = hop(2), a3 = hop(3);
    CHECK_THAT(enc->EncodeAsync(absl::MakeConstSpan(a1)) && enc->hops_in_flight() == 1);
    CHECK_THAT(enc->set_bitrate(1, 6000));   // after hop 1 was begun: hop 2 on
    CHECK_THAT(enc->EncodeAsync(absl::MakeConstSpan(a2)) && enc->hops_in_flight() == 2);
    CHECK_THAT(!enc->EncodeAsync(absl::MakeConstSpan(a3)) && enc->hops_in_flight() == 2);
    CHECK_THAT(!enc->Encode(absl::MakeConstSpan(a3)).has_value() && enc->hops_in_flight() == 2);
    CHECK_THAT(g_fake_streams_calls.size() == 3);
    CHECK_THAT(g_fake_streams_calls[1].bits[0] == 184 && g_fake_streams_calls[1].bits[4] == 64 &&
               g_fake_streams_calls[1].bits[1] == 184 && g_fake_streams_calls[2].bits[1] == 120);
    CHECK_THAT(g_fake_streams_calls[1].first[0] == a1[0] && g_fake_streams_calls[2].first[0] == a2[0]);
    auto p1 = enc->WaitEncoded();
    CHECK_THAT(p1.has_value() && enc->hops_in_flight() == 1);
    const int len1[] = {23, 23, 0, 8, 8, 15};
    for (int s = 0; s < n; ++s) CHECK_THAT(enc->packet_lengths()[s] == len1[s]);
    auto p2 = enc->WaitEncoded();
    CHECK_THAT(p2.has_value() && enc->hops_in_flight() == 0);
    CHECK_THAT(enc->packet_lengths()[1] == 15 && enc->packet_lengths()[2] == 0);
    CHECK_THAT(*p1 != *p2);
    CHECK_THAT(!enc->WaitEncoded().has_value() && enc->hops_in_flight() == 0);
    CHECK_THAT(g_fake_streams_ends == 3);
  }
  // an encoder without any DTX stream hands no flag array over
  {
    const std::vector<Params> plain = {{16000, 3200, false}, {8000, 9200, false}};
    auto e2 = MixedBatchLyraEncoder::Create(absl::MakeConstSpan(plain), 1, "model");
    CHECK_THAT(e2 != nullptr);
    std::vector<int16_t> a(320 + 160, 0);
    auto pk = e2->Encode(absl::MakeConstSpan(a));
    CHECK_THAT(pk.has_value() && g_fake_streams_calls.back().dtx_null);
    CHECK_THAT(e2->packet_lengths()[0] == 8 && e2->packet_lengths()[1] == 23);
  }
  std::printf("ok\n");
  return 0;
}
