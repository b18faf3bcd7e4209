// mixed_any_decoder_test.cc -- lyra_amd/host/lyra_mixed_device_decoder.cc against the fake ABI
// (fake_decode_samples_streams_abi.cc + the unchanged fakes of tests/decode_samples_any and tests/host_stub): the host mirror's
// leftover count and DsState follow what the device keeps, stream by stream, over a script with four rates and changing
// sizes; the packed order of the output; the refusals; the class blob round trip to and from AnySizeDeviceLyraDecoder.
// A program of its own, built with -fsanitize=address,undefined.  Prints "mixed any decoder ok" and returns 0 when all held.
#include <cstdio>
#include <cstring>
#include <vector>

#include "lyra_amd/csrc/stream_blob.h"
#include "lyra_device_decoder_any.h"
#include "lyra_mixed_device_decoder.h"

using namespace chromemedia::codec;
extern "C" int fake_streams_requests_begun();
extern "C" int fake_streams_last_max_hops();
#define CHECK_OR(cond) do { if (!(cond)) { std::fprintf(stderr, "mixed_any_decoder_test: %s (line %d)\n", #cond, __LINE__); return 1; } } while (0)

namespace {
int BlobLeft(const std::vector<uint8_t>& blob) {
  return (int)lyra::sb::ld32(blob.data() + 16 + lyra::sb::region_off(lyra::st::R_RS_D) + lyra::DSA_LEFT_COUNT);
}
lyra::DsState BlobState(const std::vector<uint8_t>& blob) {
  lyra::DsState s;
  std::memcpy(&s, blob.data() + 16 + lyra::sb::region_off(lyra::st::R_CNG) + lyra::DS_STATE, sizeof s);
  return s;
}
template <class T>
absl::Span<const T> S(const std::vector<T>& v) { return absl::MakeConstSpan(v); }
}  // namespace

int main() {
  const std::vector<int> rates = {48000, 8000, 32000, 16000, 48000};
  const int n = (int)rates.size();
  auto dec = MixedAnySizeDeviceLyraDecoder::Create(S(rates), "unused");
  CHECK_OR(dec && dec->num_streams() == n && dec->sample_rate_hz(2) == 32000 && dec->sample_rate_hz(n) == 0);
  CHECK_OR(!MixedAnySizeDeviceLyraDecoder::Create(S(std::vector<int>{48000, 44100}), "unused"));
  CHECK_OR(!MixedAnySizeDeviceLyraDecoder::Create(S(std::vector<int>{}), "unused"));
  const std::vector<int32_t> all = {0, 1, 2, 3, 4};
  std::vector<uint8_t> pk(15 * n, 7);
  // ---- four rates, changing sizes; packets for streams 1 and 4 only, a long burst for the others ----
  const std::vector<std::vector<int>> script = {
      {128, 160, 441, 320, 1024}, {128, 1, 1, 7, 441}, {128, 161, 641, 1024, 1}, {961, 640, 2560, 1280, 3840}, {2, 128, 75, 321, 0},
      {0, 0, 0, 0, 0},            {3840, 640, 2560, 1280, 3840}, {3840, 640, 2560, 1280, 959}, {1, 1, 1, 1, 1}, {2001, 400, 1300, 700, 2}};
  const int want_hops[] = {2, 1, 4, 4, 2, 1, 4, 4, 1, 3};
  const std::vector<int32_t> some = {1, 4};
  for (size_t k = 0; k < script.size(); ++k) {
    if (k % 2 == 0) CHECK_OR(dec->SetEncodedPackets(S(some), absl::MakeConstSpan(pk.data(), 30)));
    auto out = dec->DecodeSamples(S(all), S(script[k]));
    CHECK_OR(out);
    size_t at = 0;
    for (int s = 0; s < n; ++s) {   // packed in request order, every row of its own size
      for (int i = 0; i < script[k][s]; ++i) CHECK_OR((*out)[at + i] == (int16_t)(script[k][s] + i % 7));
      at += script[k][s];
    }
    CHECK_OR(at == out->size() && fake_streams_last_max_hops() == want_hops[k]);
    for (int s = 0; s < n; ++s) {
      auto blob = dec->ExportStream(s);
      CHECK_OR(blob && blob->size() == 16 + lyra_hip_stream_blob_bytes());
      CHECK_OR(BlobLeft(*blob) == dec->leftover_samples(s));
      CHECK_OR(dec->is_comfort_noise(s) == (BlobState(*blob).fade == lyra::LOSSY_FADE));
      CHECK_OR(dec->leftover_samples(s) <= (rates[s] == 48000 ? 2 : rates[s] == 32000 ? 1 : 0));
    }
  }
  CHECK_OR(dec->is_comfort_noise(0) && dec->is_comfort_noise(2) && dec->is_comfort_noise(3) && !dec->is_comfort_noise(1) &&
           !dec->is_comfort_noise(4));
  // ---- a request for some streams in another order; a packet staged for a stream it does not name goes along ----
  {
    const int32_t three = 3;
    CHECK_OR(dec->SetEncodedPackets(absl::MakeConstSpan(&three, 1), absl::MakeConstSpan(pk.data(), 15)));
    const int wait_before = BlobState(*dec->ExportStream(0)).wait;   // (exports stream 0; stream 3's packet stays staged)
    const std::vector<int32_t> order = {4, 1};
    const std::vector<int> sizes = {3, 161};
    const int begun = fake_streams_requests_begun();
    auto out = dec->DecodeSamples(S(order), S(sizes));
    CHECK_OR(out && out->size() == 164 && (*out)[0] == 3 && (*out)[3] == 161 && fake_streams_requests_begun() == begun + 1);
    auto b3 = dec->ExportStream(3);
    CHECK_OR(b3 && fake_streams_requests_begun() == begun + 1);   // nothing was left to flush
    CHECK_OR(BlobState(*b3).cp <= 0 && BlobState(*dec->ExportStream(0)).wait == wait_before);
  }
  // ---- refusals: nothing reaches the device ----
  {
    const int begun = fake_streams_requests_begun();
    std::vector<int16_t> buf(8000);
    auto req = [&](std::vector<int32_t> st, std::vector<int> sz) { return dec->DecodeSamplesAsync(S(st), S(sz)); };
    CHECK_OR(!req({0}, {3841}) && !req({1}, {641}) && !req({2}, {2561}) && !req({3}, {1281}) && !req({0}, {-1}));
    CHECK_OR(!req({0, 0}, {1, 1}) && !req({5}, {1}) && !req({-1}, {1}) && !req({0, 1}, {1}));
    CHECK_OR(!dec->WaitDecoded(absl::Span<int16_t>(buf.data(), 0)));                       // nothing in flight
    CHECK_OR(!dec->DecodeSamples(S(all), S(script[0]), absl::Span<int16_t>(buf.data(), 5)));   // wrong span: nothing begun
    CHECK_OR(fake_streams_requests_begun() == begun && dec->requests_in_flight() == 0);
    CHECK_OR(req({0, 1}, {1024, 160}) && req({4, 2}, {441, 75}) && !req({0}, {128}));     // two deep
    CHECK_OR(dec->requests_in_flight() == 2 && !dec->ExportStream(0) && !dec->DecodeSamples(S(all), S(script[0])));
    CHECK_OR(!dec->WaitDecoded(absl::Span<int16_t>(buf.data(), 5)));                       // wrong span consumes nothing
    CHECK_OR(dec->WaitDecoded(absl::Span<int16_t>(buf.data(), 1184)) && buf[0] == 1024 && buf[1024] == 160);
    CHECK_OR(dec->WaitDecoded(absl::Span<int16_t>(buf.data(), 516)) && buf[0] == 441 && buf[441] == 75);
    CHECK_OR(dec->requests_in_flight() == 0);
    CHECK_OR(req({}, {}) && dec->requests_in_flight() == 1 && dec->WaitDecoded(absl::Span<int16_t>(buf.data(), 0)));   // empty
  }
  // ---- the class blob: kind 3 with the stream's rate; to an AnySizeDeviceLyraDecoder of that rate and back ----
  auto any48 = AnySizeDeviceLyraDecoder::Create(48000, 1, "unused", 3);
  auto any32 = AnySizeDeviceLyraDecoder::Create(32000, 1, "unused", 3);
  CHECK_OR(any48 && any32);
  const std::vector<int32_t> zero = {0};
  while (dec->leftover_samples(0) == 0) CHECK_OR(dec->DecodeSamples(S(zero), S(std::vector<int>{128})));
  const int left0 = dec->leftover_samples(0);
  CHECK_OR(dec->SetEncodedPackets(S(zero), absl::MakeConstSpan(pk.data(), 15)));
  const int begun = fake_streams_requests_begun();
  auto blob = dec->ExportStream(0);                       // the staged packet goes to the device first
  CHECK_OR(blob && fake_streams_requests_begun() == begun + 1);
  uint32_t h[4];
  std::memcpy(h, blob->data(), 16);
  CHECK_OR(h[1] == 3 && h[2] == 48000 && h[3] == 0 && BlobLeft(*blob) == left0 && BlobState(*blob).wait >= 1);
  CHECK_OR(any48->ImportStream(2, absl::MakeConstSpan(*blob)) && any48->leftover_samples(2) == left0);
  CHECK_OR(!any32->ImportStream(2, absl::MakeConstSpan(*blob)));
  CHECK_OR(!dec->ImportStream(2, absl::MakeConstSpan(*blob)) && !dec->ImportStream(1, absl::MakeConstSpan(*blob)));   // 32 and 8 kHz streams
  CHECK_OR(dec->ImportStream(4, absl::MakeConstSpan(*blob)) && dec->leftover_samples(4) == left0);
  // all three go on alike
  const std::vector<int32_t> both = {4, 0};
  CHECK_OR(dec->DecodeSamples(S(both), S(std::vector<int>{441, 441})) && any48->DecodeSamples(441));
  CHECK_OR(dec->leftover_samples(0) == dec->leftover_samples(4) && dec->leftover_samples(0) == any48->leftover_samples(2));
  CHECK_OR(dec->is_comfort_noise(0) == any48->is_comfort_noise(2));
  // ... and back: a stream of an AnySizeDeviceLyraDecoder into this class
  CHECK_OR(any32->DecodeSamples(1) && any32->leftover_samples(1) == 1);
  auto from_any = any32->ExportStream(1);
  CHECK_OR(from_any && dec->ImportStream(2, absl::MakeConstSpan(*from_any)) && dec->leftover_samples(2) == 1);
  CHECK_OR(!dec->ImportStream(0, absl::MakeConstSpan(*from_any)));
  // a blob of kind "device decoder" is taken; kind 1, a count of 3, a short blob, a stream that does not exist are not
  std::vector<uint8_t> other = *blob;
  h[1] = 2;
  std::memcpy(other.data(), h, 16);
  lyra::sb::put32(other.data() + 16 + lyra::sb::region_off(lyra::st::R_RS_D) + lyra::DSA_LEFT_COUNT, 0);
  CHECK_OR(dec->ImportStream(4, absl::MakeConstSpan(other)) && dec->leftover_samples(4) == 0);
  h[1] = 1;
  std::memcpy(other.data(), h, 16);
  CHECK_OR(!dec->ImportStream(4, absl::MakeConstSpan(other)));
  other = *blob;
  lyra::sb::put32(other.data() + 16 + lyra::sb::region_off(lyra::st::R_RS_D) + lyra::DSA_LEFT_COUNT, 3);
  CHECK_OR(!dec->ImportStream(4, absl::MakeConstSpan(other)) && dec->leftover_samples(4) == 0);
  CHECK_OR(!dec->ImportStream(4, absl::MakeConstSpan(blob->data(), blob->size() - 1)));
  CHECK_OR(!dec->ImportStream(5, absl::MakeConstSpan(*blob)) && !dec->ExportStream(-1));
  std::printf("mixed any decoder ok\n");
  return 0;
}
