// lyra_mixed_device_decoder.h -- MixedAnySizeDeviceLyraDecoder: AnySizeDeviceLyraDecoder (lyra_device_decoder_any.h) where
// EVERY STREAM has a sample rate of its own and every request a size per stream, in one device call
// (include/lyra_hip_decode_samples_streams.h).  An 8 kHz telephony leg that pulls 160 samples, a 48 kHz callback of 1024 and
// a 32 kHz one of 441 are served by one object, one context and one call per tick; with AnySizeDeviceLyraDecoder they need one
// object per rate and one request per size.
//
// A request names the streams it is for and a size for each: 0 .. 4 * sample_rate_hz(s) / 50 samples of ANY size.  Audio
// comes back PACKED in the order the request names its streams: stream streams[i] contributes num_samples[i] samples, rows
// back to back.  Streams the request does not name play nothing; a packet staged for one of them is still handed to the
// device with the request (SetEncodedPacket alone), so packets never wait on the host for longer than one request.
// BufferedResampler's leftover lives with the stream on the device; the host mirrors its count beside DsState and advances
// both with the functions the device runs (decode_samples_streams_plan.h and the headers it builds on).  Everything else is
// AnySizeDeviceLyraDecoder's: the bounded packet FIFO, the second packet of a stream in a device call of its own, two
// requests in flight, nullptr / nullopt / false + LOG(ERROR) and no exceptions.
// ExportStream / ImportStream: BatchLyraEncoder::ExportStream's format, kind "any-size device decoder" with the stream's rate,
// so a stream moves between this class and an AnySizeDeviceLyraDecoder of its rate (a blob of kind "device decoder" is taken
// as well, as there).  A translation unit of its own (lyra_mixed_device_decoder.cc): nothing else references the calls of
// lyra_hip_decode_samples_streams.h.
#ifndef LYRA_AMD_HOST_LYRA_MIXED_DEVICE_DECODER_H_
#define LYRA_AMD_HOST_LYRA_MIXED_DEVICE_DECODER_H_

#include <cstdint>
#include <memory>
#include <optional>
#include <vector>

#include "../csrc/decode_samples_streams_plan.h"
#include "lyra_batch_codec.h"

namespace chromemedia {
namespace codec {

class MixedAnySizeDeviceLyraDecoder {
 public:
  // One rate per stream (the argument of LyraDecoder::Create that may differ from stream to stream).  nullptr if a rate is
  // unsupported or `sample_rates_hz` is empty.
  static std::unique_ptr<MixedAnySizeDeviceLyraDecoder> Create(absl::Span<const int> sample_rates_hz,
                                                               const ghc::filesystem::path& model_path, int device = 0);
  ~MixedAnySizeDeviceLyraDecoder();
  // Packets of ONE size (one bitrate) for the named streams, encoded.size() / streams.size() bytes each, for the next request
  // begun; streams at other bitrates take calls of their own.  AnySizeDeviceLyraDecoder's rules.
  bool SetEncodedPackets(absl::Span<const int32_t> streams, absl::Span<const uint8_t> encoded);
  // num_samples[i] samples of stream streams[i], packed in that order into out_packed (exactly their sum).  A stream named
  // twice, a stream that does not exist or a size outside 0 .. 4 hops of its stream's rate refuses the whole request.
  bool DecodeSamples(absl::Span<const int32_t> streams, absl::Span<const int> num_samples, absl::Span<int16_t> out_packed);
  std::optional<std::vector<int16_t>> DecodeSamples(absl::Span<const int32_t> streams, absl::Span<const int> num_samples);
  // The same in two halves; up to two requests in flight.  WaitDecoded() delivers the OLDEST; a WaitDecoded() refused for
  // its size consumes nothing.
  bool DecodeSamplesAsync(absl::Span<const int32_t> streams, absl::Span<const int> num_samples);
  bool WaitDecoded(absl::Span<int16_t> out_packed);
  int requests_in_flight() const { return static_cast<int>(pending_.size()); }
  // 0 for a stream that does not exist
  int sample_rate_hz(int stream) const { return stream >= 0 && stream < num_streams_ ? rates_[stream] : 0; }
  int num_channels() const { return 1; }
  int frame_rate() const { return kBatchFrameRate; }
  int num_streams() const { return num_streams_; }
  bool is_comfort_noise(int stream) const;
  int leftover_samples(int stream) const;   // 0 .. 2 resampled samples the stream holds for its next request (-1: no such stream)
  std::optional<std::vector<uint8_t>> ExportStream(int stream);
  bool ImportStream(int stream, absl::Span<const uint8_t> blob);

 private:
  MixedAnySizeDeviceLyraDecoder(lyra_hip_ctx* ctx, absl::Span<const int> sample_rates_hz);
  // the request + every staged packet to the device, host mirror advanced; *total: the samples it will deliver
  bool Begin(absl::Span<const int32_t> streams, absl::Span<const int> num_samples, long* total);
  bool FlushStaged();            // the staged packets alone: a device call of 0 samples, ended at once
  bool RowAcceptable(int32_t stream, int num_samples) const;   // one (stream, size) of a request; says why not
  bool StreamIdle(const char* method, int stream) const;

  lyra_hip_ctx* ctx_;
  int num_streams_;
  bool failed_ = false;
  std::vector<int32_t> rates_;
  std::vector<lyra::DsState> state_;           // the device's per-stream integers, mirrored (never read back)
  std::vector<int> left_;                      // ... and its leftover counts
  std::vector<uint8_t> staged_;                // [num_streams][LYRA_HIP_MAX_PACKET_BYTES] packets for the next device call
  std::vector<int32_t> staged_bytes_;          // [num_streams] 0 = none
  std::vector<long> pending_;                  // packed samples of the requests begun, oldest first
  std::vector<int32_t> row_of_;                // [num_streams] scratch of Begin: the stream's row in the call, or -1
  // the arguments of one device call, rows = the request's streams in its order, then the other streams with a staged packet
  std::vector<int32_t> call_ids_, call_bytes_, call_rates_, call_sizes_;
  std::vector<uint8_t> call_packets_;
};

}  // namespace codec
}  // namespace chromemedia
#endif
