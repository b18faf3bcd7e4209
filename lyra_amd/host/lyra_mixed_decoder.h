// lyra_mixed_decoder.h -- MixedBatchLyraDecoder: LyraDecoder (lyra/lyra_decoder.h:54-107) for many streams in one GPU context
// where EVERY STREAM has the one setting a LyraDecoder is created with -- the sample rate (lyra_decoder.cc:86-142) -- of its
// own; the bitrate comes with each packet's size (lyra_decoder.cc:172-179).  BatchLyraDecoder and DeviceLyraDecoder have one
// rate for all their streams: a process that receives at 8, 16, 32 and 48 kHz would need four objects, four contexts and four
// under-filled batches per tick.  The counterpart of MixedBatchLyraEncoder (lyra_mixed_encoder.h); BatchLyraDecoder's
// conventions: nullptr / nullopt / false + LOG(ERROR), no exceptions.  One device call per hop for the whole batch
// (include/lyra_hip_decode_streams.h).
//
// A HOP-SYNCHRONOUS receiver: per hop every stream takes at most ONE packet and delivers exactly one 20 ms frame,
// sample_rate_hz(s) / 50 samples.  A stream without a staged packet conceals, then fades to comfort noise, as the reference
// does (lyra_decoder.cc:228-340).  Two packets for a stream before a hop, or requests that are not one hop, are
// DeviceLyraDecoder's territory (lyra_device_decoder.h), at one rate per object.
//
// Buffers.  Audio comes back PACKED and stream-major: stream s contributes sample_rate_hz(s) / 50 samples, the streams' rows
// lie back to back in stream order.  Packets go in as rows of kMixedDecoderPacketRowBytes (23) bytes with a length per row.
#ifndef LYRA_AMD_HOST_LYRA_MIXED_DECODER_H_
#define LYRA_AMD_HOST_LYRA_MIXED_DECODER_H_
#include <cstdint>
#include <memory>
#include <optional>
#include <vector>

#include "absl/types/span.h"
#include "include/ghc/filesystem.hpp"

struct lyra_hip_ctx;

namespace chromemedia {
namespace codec {

constexpr int kMixedDecoderPacketRowBytes = 23;   // LYRA_HIP_MAX_PACKET_BYTES

class MixedBatchLyraDecoder {
 public:
  // The argument of LyraDecoder::Create (lyra_decoder.h:54-56) that may differ from stream to stream: one rate per stream.
  // nullptr if a rate or the channel count is unsupported (lyra_decoder.cc:90-93) or `sample_rates_hz` is empty.
  static std::unique_ptr<MixedBatchLyraDecoder> Create(absl::Span<const int> sample_rates_hz, int num_channels,
                                                      const ghc::filesystem::path& model_path, int device = 0);
  ~MixedBatchLyraDecoder();
  // Stages packets for the NEXT hop begun: `rows` holds num_streams rows of 23 bytes, lengths[s] bytes of row s are stream s's
  // packet; length 0: none for that stream.  A length other than 0 / 8 / 15 / 23 (lyra_decoder.cc:172-179 returns false on an
  // unknown size) or a packet for a stream that already has one staged refuses the WHOLE call: nothing is staged.
  bool SetEncodedPackets(absl::Span<const uint8_t> rows, absl::Span<const int32_t> lengths);
  // The same for one stream; an empty packet is refused.
  bool SetEncodedPacket(int stream, absl::Span<const uint8_t> packet);
  // One hop of every stream, packed: the sum of sample_rate_hz(s) / 50 samples.  Refused while DecodeHopAsync() hops are in
  // flight.
  std::optional<std::vector<int16_t>> DecodeHop();
  // The same in two halves: DecodeHopAsync() consumes the staged packets, starts a hop and returns; WaitDecoded() delivers
  // the OLDEST hop started into `out`, whose size must be exactly the packed hop's.  Up to two hops may be in flight; with
  // DecodeHopAsync(n + 1) issued before WaitDecoded(n) the copies run under the kernels.  A WaitDecoded() refused for its
  // size consumes nothing.
  bool DecodeHopAsync();
  bool WaitDecoded(absl::Span<int16_t> out);
  // As of the last hop DELIVERED (DecodeHop / WaitDecoded): LyraDecoder::is_comfort_noise (lyra_decoder.cc:375-377), and the
  // decoder-side estimator's is_noise().  false for a stream that does not exist.
  bool is_comfort_noise(int stream) const;
  bool is_noise(int stream) const;
  // 0 for a stream that does not exist
  int sample_rate_hz(int stream) const { return stream >= 0 && stream < num_streams() ? rates_[stream] : 0; }
  int num_channels() const { return 1; }
  int frame_rate() const { return 50; }
  int num_streams() const { return static_cast<int>(rates_.size()); }
  int hops_in_flight() const { return in_flight_; }
  size_t hop_samples() const { return hop_samples_; }   // samples of one packed hop of all streams

 private:
  MixedBatchLyraDecoder(lyra_hip_ctx* ctx, absl::Span<const int> sample_rates_hz);
  lyra_hip_ctx* ctx_;
  std::vector<int32_t> ids_;            // stream slots 0 .. num_streams - 1 of the context
  std::vector<int32_t> rates_;
  size_t hop_samples_ = 0;
  std::vector<uint8_t> staged_;         // [num_streams][23] packets for the next hop begun
  std::vector<int32_t> staged_bytes_;   // [num_streams] 0 = none
  std::vector<int32_t> noise_, cn_;     // flags of the last hop delivered
  int in_flight_ = 0;
  bool failed_ = false;                 // a device call failed: every further call is refused
};

}  // namespace codec
}  // namespace chromemedia
#endif
