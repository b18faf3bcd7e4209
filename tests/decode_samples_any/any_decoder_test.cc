// any_decoder_test.cc -- lyra_amd/host/lyra_device_decoder_any.cc against the fake ABI (fake_decode_samples_any_abi.cc +
// tests/host_stub/fake_lyra_hip_codec.cc): the host mirror's leftover count and DsState follow what the device keeps, request
// by request; the refusals; the class blob round trip, the two kinds it takes and the ones it refuses.  A program of its own,
// built with -fsanitize=address,undefined.  Prints "any decoder ok" and returns 0 when all held.
#include <cstdio>
#include <cstring>
#include <vector>

#include "lyra_amd/csrc/stream_blob.h"
#include "lyra_device_decoder_any.h"

using namespace chromemedia::codec;
extern "C" int fake_any_requests_begun();
#define CHECK_OR(cond) do { if (!(cond)) { std::fprintf(stderr, "any_decoder_test: %s (line %d)\n", #cond, __LINE__); return 1; } } while (0)

namespace {
int BlobLeft(const std::vector<uint8_t>& blob) {
  return (int)lyra::sb::ld32(blob.data() + 16 + lyra::sb::region_off(lyra::st::R_RS_D) + lyra::DSA_LEFT_COUNT);
}
lyra::DsState BlobState(const std::vector<uint8_t>& blob) {
  lyra::DsState s;
  std::memcpy(&s, blob.data() + 16 + lyra::sb::region_off(lyra::st::R_CNG) + lyra::DS_STATE, sizeof s);
  return s;
}
}  // namespace

int main() {
  const int n = 3;
  auto dec = AnySizeDeviceLyraDecoder::Create(48000, 1, "unused", n);
  auto dec2 = AnySizeDeviceLyraDecoder::Create(48000, 1, "unused", 5);
  auto dec32 = AnySizeDeviceLyraDecoder::Create(32000, 1, "unused", n);
  CHECK_OR(dec && dec2 && dec32 && !AnySizeDeviceLyraDecoder::Create(44100, 1, "unused", n));
  std::vector<uint8_t> pk(15 * n, 7);
  // ---- the mirror's leftover count: 128-frame callbacks at 48 kHz walk 0 -> 1 -> 2 -> 0 ----
  const int want_left[6] = {1, 2, 0, 1, 2, 0};
  for (int k = 0; k < 6; ++k) {
    if (k == 0) CHECK_OR(dec->SetEncodedPackets(absl::MakeConstSpan(pk)));
    auto out = dec->DecodeSamples(128);
    CHECK_OR(out && out->size() == 128u * n && (*out)[0] == 128);
    for (int s = 0; s < n; ++s) CHECK_OR(dec->leftover_samples(s) == want_left[k]);
  }
  CHECK_OR(dec->leftover_samples(-1) == -1 && dec->leftover_samples(n) == -1);
  // sizes of every kind, packets for stream 1 only, a long burst for the others: the mirror equals the device's integers
  const int sizes[] = {1024, 441, 1, 2, 0, 960, 3840, 959, 3840, 3840, 128, 3, 2000};   // (the last: stream 1 past the rest of its comfort-noise hop)
  const int32_t one = 1;
  for (int k = 0; k < (int)(sizeof sizes / sizeof sizes[0]); ++k) {
    if (k % 2 == 0) CHECK_OR(dec->SetEncodedPackets(absl::MakeConstSpan(&one, 1), absl::MakeConstSpan(pk.data(), 15)));
    std::vector<int16_t> out((size_t)n * sizes[k]);
    CHECK_OR(dec->DecodeSamples(sizes[k], absl::Span<int16_t>(out.data(), out.size())));
    for (int s = 0; s < n; ++s) {
      auto blob = dec->ExportStream(s);
      CHECK_OR(blob && blob->size() == 16 + lyra_hip_stream_blob_bytes());
      CHECK_OR(BlobLeft(*blob) == dec->leftover_samples(s));
      CHECK_OR(dec->is_comfort_noise(s) == (BlobState(*blob).fade == lyra::LOSSY_FADE));
    }
  }
  CHECK_OR(dec->is_comfort_noise(0) && dec->is_comfort_noise(2) && !dec->is_comfort_noise(1));
  // ---- refusals ----
  CHECK_OR(!dec->DecodeSamples(3841) && !dec->DecodeSamples(-1) && !dec32->DecodeSamples(2561) && dec32->DecodeSamples(2560));
  CHECK_OR(dec32->DecodeSamples(1) && dec32->leftover_samples(0) == 1 && dec32->DecodeSamples(1) && dec32->leftover_samples(0) == 0);
  std::vector<int16_t> buf((size_t)n * 1024);
  CHECK_OR(!dec->WaitDecoded(absl::Span<int16_t>(buf.data(), buf.size())));            // nothing in flight
  CHECK_OR(dec->DecodeSamplesAsync(1024) && dec->DecodeSamplesAsync(441) && !dec->DecodeSamplesAsync(128));   // two deep
  CHECK_OR(dec->requests_in_flight() == 2 && !dec->DecodeSamples(128) && !dec->ExportStream(0));
  CHECK_OR(!dec->WaitDecoded(absl::Span<int16_t>(buf.data(), 5)));                      // wrong span
  CHECK_OR(dec->WaitDecoded(absl::Span<int16_t>(buf.data(), (size_t)n * 1024)) && buf[0] == 1024);
  CHECK_OR(dec->WaitDecoded(absl::Span<int16_t>(buf.data(), (size_t)n * 441)) && buf[0] == 441);
  CHECK_OR(dec->requests_in_flight() == 0);
  // ---- the class blob: kind 3, round trip under another index of another object; the mirror follows the blob ----
  CHECK_OR(dec->DecodeSamples(128));
  while (dec->leftover_samples(0) == 0) CHECK_OR(dec->DecodeSamples(128));
  const int left0 = dec->leftover_samples(0);
  CHECK_OR(left0 == 1 || left0 == 2);
  const int begun = fake_any_requests_begun();
  CHECK_OR(dec->SetEncodedPackets(absl::MakeConstSpan(pk)));
  auto blob = dec->ExportStream(0);                       // the staged packet goes to the device first
  CHECK_OR(blob && fake_any_requests_begun() == begun + 1);
  uint32_t h[4];
  std::memcpy(h, blob->data(), 16);
  CHECK_OR(h[1] == 3 && h[2] == 48000 && h[3] == 0 && BlobLeft(*blob) == left0 && BlobState(*blob).wait == 1);
  CHECK_OR(dec2->leftover_samples(4) == 0 && !dec2->is_comfort_noise(4));
  CHECK_OR(dec2->ImportStream(4, absl::MakeConstSpan(*blob)));
  CHECK_OR(dec2->leftover_samples(4) == left0 && dec2->is_comfort_noise(4) == dec->is_comfort_noise(0));
  auto again = dec2->ExportStream(4);
  CHECK_OR(again && std::memcmp(again->data() + 16 + 256, blob->data() + 16 + 256, blob->size() - 16 - 256) == 0);
  // both go on alike
  CHECK_OR(dec->DecodeSamples(441) && dec2->DecodeSamples(441) && dec->leftover_samples(0) == dec2->leftover_samples(4));
  // a blob of kind "device decoder" is taken (its leftover is empty); kind 1, another rate, a count of 3, a short blob are not
  std::vector<uint8_t> other = *blob;
  h[1] = 2;
  std::memcpy(other.data(), h, 16);
  lyra::sb::put32(other.data() + 16 + lyra::sb::region_off(lyra::st::R_RS_D) + lyra::DSA_LEFT_COUNT, 0);
  CHECK_OR(dec2->ImportStream(1, absl::MakeConstSpan(other)) && dec2->leftover_samples(1) == 0);
  h[1] = 1;
  std::memcpy(other.data(), h, 16);
  CHECK_OR(!dec2->ImportStream(1, absl::MakeConstSpan(other)));
  CHECK_OR(!dec32->ImportStream(0, absl::MakeConstSpan(*blob)));
  other = *blob;
  lyra::sb::put32(other.data() + 16 + lyra::sb::region_off(lyra::st::R_RS_D) + lyra::DSA_LEFT_COUNT, 3);
  CHECK_OR(!dec2->ImportStream(2, absl::MakeConstSpan(other)) && dec2->leftover_samples(2) == 0);
  CHECK_OR(!dec2->ImportStream(2, absl::MakeConstSpan(blob->data(), blob->size() - 1)));
  CHECK_OR(!dec2->ImportStream(5, absl::MakeConstSpan(*blob)) && !dec2->ExportStream(-1));
  std::printf("any decoder ok\n");
  return 0;
}
