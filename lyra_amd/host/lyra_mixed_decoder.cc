// lyra_mixed_decoder.cc -- see lyra_mixed_decoder.h.  Plain C++17 over the C ABI (include/lyra_hip_decode_streams.h); no HIP
// here.  A translation unit of its own: the three calls it needs are not among those lyra_batch_codec.cc is built against.
#include "lyra_mixed_decoder.h"

#include <algorithm>
#include <cstring>

#include "../../include/lyra_hip_decode_streams.h"
#include "glog/logging.h"
#include "host_common.h"

namespace chromemedia {
namespace codec {
using namespace host;

static_assert(kMixedDecoderPacketRowBytes == LYRA_HIP_MAX_PACKET_BYTES, "packet row stride");

MixedBatchLyraDecoder::MixedBatchLyraDecoder(lyra_hip_ctx* ctx, absl::Span<const int> sample_rates_hz)
    : ctx_(ctx),
      ids_(Iota(static_cast<int>(sample_rates_hz.size()))),
      staged_(sample_rates_hz.size() * kMixedDecoderPacketRowBytes, 0),
      staged_bytes_(sample_rates_hz.size(), 0),
      noise_(sample_rates_hz.size(), 0),
      cn_(sample_rates_hz.size(), 0) {
  for (int rate : sample_rates_hz) {
    rates_.push_back(rate);
    hop_samples_ += static_cast<size_t>(rate / 50);
  }
}

std::unique_ptr<MixedBatchLyraDecoder> MixedBatchLyraDecoder::Create(absl::Span<const int> sample_rates_hz, int num_channels,
                                                                    const ghc::filesystem::path& model_path, int device) {
  const int n = static_cast<int>(sample_rates_hz.size());
  if (n == 0) {
    LOG(ERROR) << "num_streams must be positive.";
    return nullptr;
  }
  for (int rate : sample_rates_hz)
    if (!ParamsSupported(rate, num_channels, n)) return nullptr;
  lyra_hip_ctx* ctx = NewContext(model_path, device, n);
  if (ctx == nullptr) {
    LOG(ERROR) << "Could not create the decoder's context.";
    return nullptr;
  }
  return std::unique_ptr<MixedBatchLyraDecoder>(new MixedBatchLyraDecoder(ctx, sample_rates_hz));
}

MixedBatchLyraDecoder::~MixedBatchLyraDecoder() { lyra_hip_destroy(ctx_); }

bool MixedBatchLyraDecoder::SetEncodedPackets(absl::Span<const uint8_t> rows, absl::Span<const int32_t> lengths) {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  const size_t n = static_cast<size_t>(num_streams());
  if (lengths.size() != n || rows.size() != n * kMixedDecoderPacketRowBytes) {
    LOG(ERROR) << "SetEncodedPackets takes " << n << " rows of " << kMixedDecoderPacketRowBytes << " bytes and " << n
               << " lengths, but got " << rows.size() << " bytes and " << lengths.size() << " lengths.";
    return false;
  }
  // the whole call is judged before any of it is staged
  for (size_t s = 0; s < n; ++s) {
    if (lengths[s] == 0) continue;
    if (PacketSizeToBits(lengths[s]) < 0) {   // lyra_decoder.cc:172-179
      LOG(ERROR) << "The packet size (" << lengths[s] << " bytes, stream " << s << ") is not supported.";
      return false;
    }
    if (staged_bytes_[s] != 0) {
      LOG(ERROR) << "Stream " << s << " already has a packet for the next hop: one packet per stream and hop "
                 << "(two are DeviceLyraDecoder's).";
      return false;
    }
  }
  for (size_t s = 0; s < n; ++s) {
    if (lengths[s] == 0) continue;
    std::memcpy(&staged_[s * kMixedDecoderPacketRowBytes], &rows[s * kMixedDecoderPacketRowBytes],
                static_cast<size_t>(lengths[s]));
    staged_bytes_[s] = lengths[s];
  }
  return true;
}

bool MixedBatchLyraDecoder::SetEncodedPacket(int stream, absl::Span<const uint8_t> packet) {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  if (stream < 0 || stream >= num_streams()) {
    LOG(ERROR) << "Stream " << stream << " does not exist.";
    return false;
  }
  if (PacketSizeToBits(static_cast<int>(packet.size())) < 0) {
    LOG(ERROR) << "The packet size (" << packet.size() << " bytes) is not supported.";
    return false;
  }
  if (staged_bytes_[stream] != 0) {
    LOG(ERROR) << "Stream " << stream << " already has a packet for the next hop: one packet per stream and hop "
               << "(two are DeviceLyraDecoder's).";
    return false;
  }
  std::memcpy(&staged_[static_cast<size_t>(stream) * kMixedDecoderPacketRowBytes], packet.data(), packet.size());
  staged_bytes_[stream] = static_cast<int32_t>(packet.size());
  return true;
}

bool MixedBatchLyraDecoder::DecodeHopAsync() {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  if (in_flight_ >= 2) {
    LOG(ERROR) << "Two hops are already in flight: call WaitDecoded() first.";
    return false;
  }
  // lyra_decoder.cc:172-340 per stream on the device: the packet at its own size (or concealment / comfort noise), the
  // stream's own output resampler, rows packed in stream order
  if (lyra_hip_decode_streams_begin(ctx_, ids_.data(), num_streams(), staged_.data(), staged_bytes_.data(), rates_.data()) != 0) {
    LOG(ERROR) << "Unable to decode the hop: " << lyra_hip_last_error(ctx_);
    failed_ = true;
    return false;
  }
  std::fill(staged_bytes_.begin(), staged_bytes_.end(), 0);   // the staging belongs to the hop begun
  ++in_flight_;
  return true;
}

bool MixedBatchLyraDecoder::WaitDecoded(absl::Span<int16_t> out) {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  if (in_flight_ == 0) {
    LOG(ERROR) << "WaitDecoded() without a hop in flight.";
    return false;
  }
  if (out.size() != hop_samples_) {
    LOG(ERROR) << "The output has to hold exactly " << hop_samples_ << " samples (one 20 ms frame of each of "
               << num_streams() << " streams, packed), but holds " << out.size() << ".";
    return false;
  }
  --in_flight_;
  if (lyra_hip_decode_streams_end(ctx_, out.data(), noise_.data(), cn_.data()) != 0) {
    LOG(ERROR) << "Unable to decode the hop: " << lyra_hip_last_error(ctx_);
    failed_ = true;   // the hop's samples are lost and the streams have moved on
    return false;
  }
  return true;
}

std::optional<std::vector<int16_t>> MixedBatchLyraDecoder::DecodeHop() {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return std::nullopt;
  }
  if (in_flight_ != 0) {
    LOG(ERROR) << "DecodeHop() while " << in_flight_ << " DecodeHopAsync() hops are in flight: call WaitDecoded() first.";
    return std::nullopt;
  }
  if (!DecodeHopAsync()) return std::nullopt;
  std::vector<int16_t> out(hop_samples_);
  if (!WaitDecoded(absl::Span<int16_t>(out.data(), out.size()))) return std::nullopt;
  return out;
}

bool MixedBatchLyraDecoder::is_comfort_noise(int stream) const {
  return stream >= 0 && stream < num_streams() && cn_[stream] != 0;
}

bool MixedBatchLyraDecoder::is_noise(int stream) const {
  return stream >= 0 && stream < num_streams() && noise_[stream] != 0;
}

}  // namespace codec
}  // namespace chromemedia
