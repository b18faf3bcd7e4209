// class_blob_test.cc -- lyra_amd/host/lyra_stream_state.cc against the fake ABI (fake_stream_abi.cc +
// tests/host_stub/fake_lyra_hip_codec.cc): the class header round-trips, a wrong kind, a wrong rate and calls with requests in
// flight are refused, DeviceLyraDecoder rebuilds its host mirror and drops the target's staged packet.  Exit code 0 = all held.
#include <cstdio>
#include <cstring>
#include <vector>

#include "lyra_batch_codec.h"
#include "lyra_device_decoder.h"

using namespace chromemedia::codec;
extern "C" void fake_set_ds_state(const void* c, int id, const lyra::DsState* s);
extern "C" int fake_requests_begun();
#define CHECK_OR(cond) do { if (!(cond)) { std::fprintf(stderr, "class_blob_test: %s (line %d)\n", #cond, __LINE__); return 1; } } while (0)

// the context pointer of an object, for the fake's test hook: the first member behind no vtable in both classes
template <class T> const void* CtxOf(const T* obj) { const void* p; std::memcpy(&p, obj, sizeof p); return p; }

int main() {
  auto dec = DeviceLyraDecoder::Create(48000, 1, "unused", 4);
  auto dec2 = DeviceLyraDecoder::Create(48000, 1, "unused", 6);
  auto dec16 = DeviceLyraDecoder::Create(16000, 1, "unused", 4);
  auto enc = BatchLyraEncoder::Create(48000, 1, 6000, true, "unused", 4);
  auto enc2 = BatchLyraEncoder::Create(48000, 1, 6000, true, "unused", 4);
  auto enc16 = BatchLyraEncoder::Create(16000, 1, 6000, true, "unused", 4);
  CHECK_OR(dec && dec2 && dec16 && enc && enc2 && enc16);
  const lyra::DsState cn = {lyra::LOSSY_CONCEAL, lyra::LOSSY_FADE, 1, 0, 160, lyra::DS_FIFO_DEPTH - 1, 2};   // in comfort noise, 3 vectors wait
  fake_set_ds_state(CtxOf(dec.get()), 1, &cn);
  auto blob = dec->ExportStream(1);
  CHECK_OR(blob && blob->size() == 16 + lyra_hip_stream_blob_bytes());
  uint32_t h[4];
  std::memcpy(h, blob->data(), 16);
  CHECK_OR(h[1] == 2 && h[2] == 48000 && h[3] == 0);
  // round trip into another object under another index: the mirror follows the blob
  CHECK_OR(!dec2->is_comfort_noise(5));
  CHECK_OR(dec2->ImportStream(5, absl::MakeConstSpan(*blob)) && dec2->is_comfort_noise(5) && !dec2->is_comfort_noise(1));
  auto again = dec2->ExportStream(5);
  CHECK_OR(again && std::memcmp(again->data(), blob->data(), 16) == 0);
  CHECK_OR(std::memcmp(again->data() + 16 + 256, blob->data() + 16 + 256, blob->size() - 16 - 256) == 0);
  // wait == 3 of the rebuilt mirror: one more packet is taken, the next finds the FIFO full
  const uint8_t pk[15] = {1, 2, 3};
  const int32_t five = 5;
  CHECK_OR(dec2->SetEncodedPackets(absl::MakeConstSpan(&five, 1), absl::MakeConstSpan(pk, 15)));
  CHECK_OR(!dec2->SetEncodedPackets(absl::MakeConstSpan(&five, 1), absl::MakeConstSpan(pk, 15)));
  // ImportStream drops the staged packet: a fresh stream's blob, then DEPTH packets fit again (the staged one would count)
  auto fresh = dec->ExportStream(0);
  CHECK_OR(fresh && dec2->ImportStream(5, absl::MakeConstSpan(*fresh)) && !dec2->is_comfort_noise(5));
  for (int k = 0; k < lyra::DS_FIFO_DEPTH; ++k) CHECK_OR(dec2->SetEncodedPackets(absl::MakeConstSpan(&five, 1), absl::MakeConstSpan(pk, 15)));
  CHECK_OR(!dec2->SetEncodedPackets(absl::MakeConstSpan(&five, 1), absl::MakeConstSpan(pk, 15)));
  // ExportStream hands a staged packet to the device first
  const int begun = fake_requests_begun();
  CHECK_OR(dec2->ExportStream(5) && fake_requests_begun() == begun + 1);
  // wrong kind, wrong rate, wrong size, wrong magic, bad index
  auto eblob = enc->ExportStream(2);
  CHECK_OR(eblob && eblob->size() == blob->size());
  std::memcpy(h, eblob->data(), 16);
  CHECK_OR(h[1] == 1 && h[2] == 48000);
  CHECK_OR(enc2->ImportStream(3, absl::MakeConstSpan(*eblob)));
  CHECK_OR(!dec2->ImportStream(0, absl::MakeConstSpan(*eblob)) && !enc2->ImportStream(0, absl::MakeConstSpan(*blob)));
  CHECK_OR(!dec16->ImportStream(0, absl::MakeConstSpan(*blob)) && !enc16->ImportStream(0, absl::MakeConstSpan(*eblob)));
  CHECK_OR(!dec2->ImportStream(0, absl::MakeConstSpan(blob->data(), blob->size() - 1)));
  { auto bad = *blob; bad[0] ^= 1; CHECK_OR(!dec2->ImportStream(0, absl::MakeConstSpan(bad))); }
  { auto bad = *blob; bad[16] ^= 1; CHECK_OR(!dec2->ImportStream(0, absl::MakeConstSpan(bad))); }       // the C blob's magic
  CHECK_OR(!dec2->ImportStream(6, absl::MakeConstSpan(*blob)) && !dec2->ImportStream(-1, absl::MakeConstSpan(*blob)));
  CHECK_OR(!dec2->ExportStream(6) && !enc->ExportStream(4));
  // requests in flight
  CHECK_OR(dec->DecodeSamplesAsync(480));
  CHECK_OR(!dec->ExportStream(0) && !dec->ImportStream(0, absl::MakeConstSpan(*blob)));
  std::vector<int16_t> out(4 * 480);
  CHECK_OR(dec->WaitDecoded(absl::Span<int16_t>(out.data(), out.size())) && dec->ExportStream(0));
  std::vector<int16_t> pcm(4 * 960, 0);
  CHECK_OR(enc->EncodeAsync(absl::MakeConstSpan(pcm)));
  CHECK_OR(!enc->ExportStream(0) && !enc->ImportStream(0, absl::MakeConstSpan(*eblob)));
  CHECK_OR(enc->WaitEncoded() && enc->ExportStream(0) && enc->ImportStream(0, absl::MakeConstSpan(*eblob)));
  std::printf("class blobs ok\n");
  return 0;
}
