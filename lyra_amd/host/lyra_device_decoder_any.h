// lyra_device_decoder_any.h -- AnySizeDeviceLyraDecoder: DeviceLyraDecoder (lyra_device_decoder.h) without its size rule.
// A request is 0 .. 4 * sample_rate_hz / 50 samples of ANY size (include/lyra_hip_decode_samples_any.h): the 128 / 256 / 441 /
// 512 / 1024-frame callbacks of audio back ends, at every codec rate.  BufferedResampler's leftover lives with the stream on
// the device; the host mirrors its count beside DsState and advances both with the functions the device runs
// (decode_samples_any_plan.h, decode_samples_plan.h).  Method names and signatures are DeviceLyraDecoder's, so one can stand in
// for the other; everything else that header says -- the bounded packet FIFO, the second packet of a stream in a device
// call of its own, two requests in flight -- holds here too.
// ExportStream / ImportStream: BatchLyraEncoder::ExportStream's format, kind "any-size device decoder".  ImportStream also
// accepts a blob of kind "device decoder" (a DeviceLyraDecoder's stream has an empty leftover) and reads the leftover count
// from the device blob.  A translation unit of its own (lyra_device_decoder_any.cc): nothing else references the calls of
// lyra_hip_decode_samples_any.h.
#ifndef LYRA_AMD_HOST_LYRA_DEVICE_DECODER_ANY_H_
#define LYRA_AMD_HOST_LYRA_DEVICE_DECODER_ANY_H_

#include <cstdint>
#include <memory>
#include <optional>
#include <vector>

#include "../csrc/decode_samples_any_plan.h"
#include "lyra_batch_codec.h"

namespace chromemedia {
namespace codec {

class AnySizeDeviceLyraDecoder {
 public:
  static std::unique_ptr<AnySizeDeviceLyraDecoder> Create(int sample_rate_hz, int num_channels,
                                                          const ghc::filesystem::path& model_path, int num_streams,
                                                          int device = 0);
  ~AnySizeDeviceLyraDecoder();
  bool SetEncodedPackets(absl::Span<const uint8_t> encoded);
  bool SetEncodedPackets(absl::Span<const int32_t> streams, absl::Span<const uint8_t> encoded);
  std::optional<std::vector<int16_t>> DecodeSamples(int num_samples);
  bool DecodeSamples(int num_samples, absl::Span<int16_t> out);
  bool DecodeSamplesAsync(int num_samples);
  bool WaitDecoded(absl::Span<int16_t> out);
  int requests_in_flight() const { return static_cast<int>(pending_.size()); }
  int sample_rate_hz() const { return sample_rate_hz_; }
  int num_channels() const { return 1; }
  int frame_rate() const { return kBatchFrameRate; }
  bool is_comfort_noise(int stream) const;
  int num_streams() const { return num_streams_; }
  int leftover_samples(int stream) const;   // 0 .. 2 resampled samples the stream holds for its next request (-1: no such stream)
  std::optional<std::vector<uint8_t>> ExportStream(int stream);
  bool ImportStream(int stream, absl::Span<const uint8_t> blob);

 private:
  AnySizeDeviceLyraDecoder(lyra_hip_ctx* ctx, int sample_rate_hz, int num_streams);
  bool Begin(int num_samples);   // the staged packets + a request of num_samples to the device, host mirror advanced
  bool FlushStaged();            // the staged packets alone: a device call of 0 samples, ended at once
  bool StreamIdle(const char* method, int stream) const;

  lyra_hip_ctx* ctx_;
  int sample_rate_hz_;
  int num_streams_;
  bool failed_ = false;
  std::vector<int32_t> all_ids_;
  std::vector<lyra::DsState> state_;           // the device's per-stream integers, mirrored (never read back)
  std::vector<int> left_;                      // ... and its leftover counts
  std::vector<uint8_t> staged_;                // [num_streams][LYRA_HIP_MAX_PACKET_BYTES] packets for the next device call
  std::vector<int32_t> staged_bytes_;          // [num_streams] 0 = none
  std::vector<int> pending_;                   // num_samples of the requests begun, oldest first
};

}  // namespace codec
}  // namespace chromemedia
#endif
