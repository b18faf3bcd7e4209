// lyra_mixed_encoder.h -- MixedBatchLyraEncoder: LyraEncoder (lyra/lyra_encoder.h:61-101) for many streams in one GPU context
// where EVERY STREAM has the three settings a LyraEncoder is created with -- sample rate, bitrate, enable_dtx
// (lyra_encoder.cc:44-111) -- of its own.  BatchLyraEncoder (lyra_batch_codec.h) has one of each for all its streams; a server
// with mixed callers would need one object, one context and one under-filled batch per class of caller.  Same method names,
// argument meaning and error behaviour as BatchLyraEncoder: nullptr / nullopt / false + LOG(ERROR), no exceptions.
// One device call per hop for the whole batch (include/lyra_hip_encode_streams.h).
//
// Buffers.  Audio is PACKED and stream-major: stream s contributes sample_rate_hz(s) / 50 samples, the streams' rows lie back
// to back in stream order.  Packets come back as num_streams rows of kMixedPacketRowBytes (23) bytes: row s holds
// packet_lengths()[s] bytes of packet -- 8 / 15 / 23 by the stream's bitrate, or 0 for a DTX empty packet
// (lyra_encoder.cc:136-141) -- and zeros behind them.
#ifndef LYRA_AMD_HOST_LYRA_MIXED_ENCODER_H_
#define LYRA_AMD_HOST_LYRA_MIXED_ENCODER_H_
#include <cstdint>
#include <memory>
#include <optional>
#include <vector>

#include "absl/types/span.h"
#include "include/ghc/filesystem.hpp"

struct lyra_hip_ctx;

namespace chromemedia {
namespace codec {

constexpr int kMixedPacketRowBytes = 23;   // LYRA_HIP_MAX_PACKET_BYTES

class MixedBatchLyraEncoder {
 public:
  // The arguments of LyraEncoder::Create (lyra_encoder.h:61-63) that may differ from stream to stream
  struct EncoderParams { int sample_rate_hz; int bitrate; bool enable_dtx; };
  // nullptr if a parameter of any stream is unsupported (lyra_encoder.cc:46-66) or `streams` is empty.
  static std::unique_ptr<MixedBatchLyraEncoder> Create(absl::Span<const EncoderParams> streams, int num_channels,
                                                      const ghc::filesystem::path& model_path, int device = 0);
  ~MixedBatchLyraEncoder();
  // One 20 ms frame of every stream, packed: packed_audio.size() must be exactly the sum of sample_rate_hz(s) / 50
  // (lyra_encoder.cc:124-129 per stream), else nullopt.  Returns num_streams rows of kMixedPacketRowBytes bytes.
  std::optional<std::vector<uint8_t>> Encode(absl::Span<const int16_t> packed_audio);
  // The same in two halves: EncodeAsync() starts a hop and returns -- `packed_audio` may be reused at once --, WaitEncoded()
  // returns the packets of the OLDEST hop started.  Up to two hops may be in flight; with EncodeAsync(n + 1) issued before
  // WaitEncoded(n) the upload of hop n + 1 and the download of hop n run under the kernels.  Same packets as Encode().
  bool EncodeAsync(absl::Span<const int16_t> packed_audio);
  std::optional<std::vector<uint8_t>> WaitEncoded();
  // lyra_encoder.cc:158-166 for one stream: refused (false) for an unsupported bitrate or a stream that does not exist;
  // takes effect on the next hop begun.  Sample rate and DTX are fixed at Create, as in the reference.
  bool set_bitrate(int stream, int bitrate);
  // Bytes of each stream's packet from the last Encode / WaitEncoded; 0 for a DTX empty packet.
  const std::vector<int32_t>& packet_lengths() const { return lengths_; }
  int sample_rate_hz(int stream) const { return rates_[stream]; }
  int bitrate(int stream) const { return bitrates_[stream]; }
  bool enable_dtx(int stream) const { return dtx_[stream] != 0; }
  int num_channels() const { return 1; }
  int frame_rate() const { return 50; }
  int num_streams() const { return static_cast<int>(rates_.size()); }
  int hops_in_flight() const { return in_flight_; }

 private:
  MixedBatchLyraEncoder(lyra_hip_ctx* ctx, absl::Span<const EncoderParams> streams);
  lyra_hip_ctx* ctx_;
  std::vector<int32_t> ids_;        // stream slots 0 .. num_streams - 1 of the context
  std::vector<int32_t> rates_, bitrates_, bits_, dtx_;
  bool any_dtx_ = false;
  size_t hop_samples_ = 0;          // samples of one packed hop of all streams
  std::vector<int32_t> lengths_;
  int in_flight_ = 0;
};

}  // namespace codec
}  // namespace chromemedia
#endif
