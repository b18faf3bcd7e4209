// lyra_mixed_encoder.cc -- see lyra_mixed_encoder.h.  Plain C++17 over the C ABI (include/lyra_hip_encode_streams.h); no HIP
// here.  A translation unit of its own: the three calls it needs are not among those lyra_batch_codec.cc is built against.
#include "lyra_mixed_encoder.h"

#include "../../include/lyra_hip_encode_streams.h"
#include "glog/logging.h"
#include "host_common.h"
#include "lyra_batch_codec.h"

namespace chromemedia {
namespace codec {
using namespace host;

static_assert(kMixedPacketRowBytes == LYRA_HIP_MAX_PACKET_BYTES, "packet row stride");

MixedBatchLyraEncoder::MixedBatchLyraEncoder(lyra_hip_ctx* ctx, absl::Span<const EncoderParams> streams)
    : ctx_(ctx), ids_(Iota(static_cast<int>(streams.size()))), lengths_(streams.size(), 0) {
  for (const EncoderParams& p : streams) {
    rates_.push_back(p.sample_rate_hz);
    bitrates_.push_back(p.bitrate);
    bits_.push_back(BatchBitrateToNumQuantizedBits(p.bitrate));
    dtx_.push_back(p.enable_dtx ? 1 : 0);
    any_dtx_ = any_dtx_ || p.enable_dtx;
    hop_samples_ += static_cast<size_t>(p.sample_rate_hz / kBatchFrameRate);
  }
}

std::unique_ptr<MixedBatchLyraEncoder> MixedBatchLyraEncoder::Create(absl::Span<const EncoderParams> streams,
                                                                    int num_channels,
                                                                    const ghc::filesystem::path& model_path, int device) {
  const int n = static_cast<int>(streams.size());
  if (n == 0) {
    LOG(ERROR) << "num_streams must be positive.";
    return nullptr;
  }
  for (int s = 0; s < n; ++s) {
    if (!ParamsSupported(streams[s].sample_rate_hz, num_channels, n)) return nullptr;
    if (BatchBitrateToNumQuantizedBits(streams[s].bitrate) < 0) {
      LOG(ERROR) << "Bitrate " << streams[s].bitrate << " bps (stream " << s << ") is not supported by codec.";
      return nullptr;
    }
  }
  lyra_hip_ctx* ctx = NewContext(model_path, device, n);
  if (ctx == nullptr) {
    LOG(ERROR) << "Could not create Features Extractor.";
    return nullptr;
  }
  return std::unique_ptr<MixedBatchLyraEncoder>(new MixedBatchLyraEncoder(ctx, streams));
}

MixedBatchLyraEncoder::~MixedBatchLyraEncoder() { lyra_hip_destroy(ctx_); }

bool MixedBatchLyraEncoder::EncodeAsync(absl::Span<const int16_t> packed_audio) {
  if (packed_audio.size() != hop_samples_) {
    LOG(ERROR) << "The number of audio samples has to be exactly " << hop_samples_ << " (one 20 ms frame of each of "
               << num_streams() << " streams, packed), but is " << packed_audio.size() << ".";
    return false;
  }
  if (in_flight_ >= 2) {
    LOG(ERROR) << "Two hops are already in flight: call WaitEncoded() first.";
    return false;
  }
  // lyra_encoder.cc:119-156 per stream on the device: the stream's own resampler, with DTX its own noise decision, extract,
  // quantize at its own bit count, pack
  if (lyra_hip_encode_streams_begin(ctx_, ids_.data(), num_streams(), packed_audio.data(), rates_.data(), bits_.data(),
                                    any_dtx_ ? dtx_.data() : nullptr) != 0) {
    LOG(ERROR) << "Unable to extract and quantize features from audio: " << lyra_hip_last_error(ctx_);
    return false;
  }
  ++in_flight_;
  return true;
}

std::optional<std::vector<uint8_t>> MixedBatchLyraEncoder::WaitEncoded() {
  if (in_flight_ == 0) {
    LOG(ERROR) << "WaitEncoded() without a hop in flight.";
    return std::nullopt;
  }
  --in_flight_;
  std::vector<uint8_t> packets(static_cast<size_t>(num_streams()) * kMixedPacketRowBytes);
  if (lyra_hip_encode_streams_end(ctx_, packets.data(), lengths_.data()) != 0) {
    LOG(ERROR) << "Unable to extract and quantize features from audio: " << lyra_hip_last_error(ctx_);
    return std::nullopt;
  }
  return packets;
}

std::optional<std::vector<uint8_t>> MixedBatchLyraEncoder::Encode(absl::Span<const int16_t> packed_audio) {
  if (in_flight_ != 0) {
    LOG(ERROR) << "Encode() while " << in_flight_ << " EncodeAsync() hops are in flight: call WaitEncoded() first.";
    return std::nullopt;
  }
  if (!EncodeAsync(packed_audio)) return std::nullopt;
  return WaitEncoded();
}

bool MixedBatchLyraEncoder::set_bitrate(int stream, int bitrate) {
  if (stream < 0 || stream >= num_streams()) {
    LOG(ERROR) << "Stream " << stream << " does not exist.";
    return false;
  }
  const int bits = BatchBitrateToNumQuantizedBits(bitrate);
  if (bits < 0) {
    LOG(ERROR) << "Bitrate " << bitrate << " bps is not supported by codec.";
    return false;
  }
  bitrates_[stream] = bitrate;
  bits_[stream] = bits;
  return true;
}

}  // namespace codec
}  // namespace chromemedia
