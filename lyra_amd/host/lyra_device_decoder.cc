// lyra_device_decoder.cc -- see lyra_device_decoder.h.
#include "lyra_device_decoder.h"

#include <cstring>

#include "../../include/lyra_hip.h"
#include "glog/logging.h"
#include "host_common.h"

namespace chromemedia {
namespace codec {
using namespace host;

DeviceLyraDecoder::DeviceLyraDecoder(lyra_hip_ctx* ctx, int sample_rate_hz, int num_streams)
    : ctx_(ctx), sample_rate_hz_(sample_rate_hz), num_streams_(num_streams), all_ids_(Iota(num_streams)),
      state_(num_streams, lyra::DsState{0, 0, 0, 0, 0, 0, 0}),
      staged_(static_cast<size_t>(num_streams) * LYRA_HIP_MAX_PACKET_BYTES), staged_bytes_(num_streams, 0) {}

std::unique_ptr<DeviceLyraDecoder> DeviceLyraDecoder::Create(int sample_rate_hz, int num_channels,
                                                              const ghc::filesystem::path& model_path,
                                                              int num_streams, int device) {
  if (!ParamsSupported(sample_rate_hz, num_channels, num_streams)) return nullptr;
  lyra_hip_ctx* ctx = NewContext(model_path, device, num_streams);
  if (ctx == nullptr) {
    LOG(ERROR) << "New model could not be instantiated.";
    return nullptr;
  }
  if (lyra_hip_set_stream_priorities(ctx, 0, 2, 2) != 0) LOG(WARNING) << "stream priorities: " << lyra_hip_last_error(ctx);
  return std::unique_ptr<DeviceLyraDecoder>(new DeviceLyraDecoder(ctx, sample_rate_hz, num_streams));
}

DeviceLyraDecoder::~DeviceLyraDecoder() { lyra_hip_destroy(ctx_); }

bool DeviceLyraDecoder::is_comfort_noise(int stream) const {
  return stream >= 0 && stream < num_streams_ && state_[stream].fade == lyra::LOSSY_FADE;
}

bool DeviceLyraDecoder::SetEncodedPackets(absl::Span<const uint8_t> encoded) {
  return SetEncodedPackets(absl::MakeConstSpan(all_ids_), encoded);
}

bool DeviceLyraDecoder::SetEncodedPackets(absl::Span<const int32_t> streams, absl::Span<const uint8_t> encoded) {
  const int packet_size = CheckEncodedPackets(failed_, streams, encoded, num_streams_);   // (lyra::mixed_received's sizes)
  if (packet_size <= 0) return packet_size == 0;
  bool second = false;
  for (int32_t id : streams) {
    const int staged = staged_bytes_[id] != 0 ? 1 : 0;
    if (state_[id].wait + staged >= lyra::DS_FIFO_DEPTH) {
      LOG(ERROR) << "Stream " << id << " already holds " << lyra::DS_FIFO_DEPTH << " packets whose hop has not started: the "
                 << "device-side feature FIFO is full (LYRA_HIP_DECODE_SAMPLES_FIFO). No packet of this call was queued.";
      return false;
    }
    second = second || staged != 0;
  }
  if (second) {   // at most one packet per stream and device call: what is staged goes first, in a call of 0 samples
    if (!pending_.empty()) {
      LOG(ERROR) << "A second packet for a stream needs a device call of its own, which cannot overtake the "
                 << pending_.size() << " DecodeSamplesAsync() requests in flight: call WaitDecoded() first.";
      return false;
    }
    if (!FlushStaged()) return false;
  }
  for (size_t i = 0; i < streams.size(); ++i) {
    std::memcpy(staged_.data() + static_cast<size_t>(streams[i]) * LYRA_HIP_MAX_PACKET_BYTES,
                encoded.data() + i * packet_size, static_cast<size_t>(packet_size));
    staged_bytes_[streams[i]] = packet_size;
  }
  return true;
}

bool DeviceLyraDecoder::Begin(int num_samples) {
  const int n_int = lyra::ds_internal_samples(num_samples, sample_rate_hz_);
  if (lyra_hip_decode_samples_begin(ctx_, all_ids_.data(), num_streams_, staged_.data(), staged_bytes_.data(), num_samples,
                                    sample_rate_hz_) != 0) {
    failed_ = true;
    LOG(ERROR) << "Could not decode samples: " << lyra_hip_last_error(ctx_);
    return false;
  }
  for (int s = 0; s < num_streams_; ++s) {   // what the device's plan kernel does with the same inputs
    state_[s] = lyra::ds_plan(state_[s], staged_bytes_[s] != 0, n_int).s;
    staged_bytes_[s] = 0;
  }
  return true;
}

bool DeviceLyraDecoder::FlushStaged() {
  if (!Begin(0)) return false;
  if (lyra_hip_decode_samples_end(ctx_, nullptr) != 0) {
    failed_ = true;
    LOG(ERROR) << "Could not queue packets: " << lyra_hip_last_error(ctx_);
    return false;
  }
  return true;
}

std::optional<std::vector<int16_t>> DeviceLyraDecoder::DecodeSamples(int num_samples) {
  if (num_samples < 0) {
    LOG(ERROR) << kNegativeSamples;
    return std::nullopt;
  }
  std::vector<int16_t> out(static_cast<size_t>(num_streams_) * num_samples);
  if (!DecodeSamples(num_samples, absl::Span<int16_t>(out.data(), out.size()))) return std::nullopt;
  return out;
}

bool DeviceLyraDecoder::DecodeSamples(int num_samples, absl::Span<int16_t> out) {
  if (!pending_.empty()) {
    LOG(ERROR) << "DecodeSamples() while " << pending_.size() << " DecodeSamplesAsync() requests are in flight: call WaitDecoded() first.";
    return false;
  }
  return DecodeSamplesAsync(num_samples) && WaitDecoded(out);
}

bool DeviceLyraDecoder::DecodeSamplesAsync(int num_samples) {
  if (num_samples < 0) {
    LOG(ERROR) << kNegativeSamples;
    return false;
  }
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  if (lyra::ds_internal_samples(num_samples, sample_rate_hz_) < 0) {
    LOG(ERROR) << "A request of " << num_samples << " samples at " << sample_rate_hz_ << " Hz is outside the device decoder's "
               << "size rule: at most " << sample_rate_hz_ / 50 << " samples (one hop) and a whole number of 16 kHz samples. "
               << "Use BatchLyraDecoder for such requests.";
    return false;
  }
  if (pending_.size() >= 2) {
    LOG(ERROR) << "Two requests are already in flight: call WaitDecoded() first.";
    return false;
  }
  if (!Begin(num_samples)) return false;
  pending_.push_back(num_samples);
  return true;
}

bool DeviceLyraDecoder::WaitDecoded(absl::Span<int16_t> out) {
  if (pending_.empty()) {
    LOG(ERROR) << "WaitDecoded() without a request in flight.";
    return false;
  }
  const int n = pending_.front();
  if (out.size() != static_cast<size_t>(num_streams_) * n) {
    LOG(ERROR) << "Output span has " << out.size() << " samples, expected " << static_cast<size_t>(num_streams_) * n;
    return false;
  }
  pending_.erase(pending_.begin());
  if (lyra_hip_decode_samples_end(ctx_, out.data()) != 0) {
    failed_ = true;
    LOG(ERROR) << "Could not decode samples: " << lyra_hip_last_error(ctx_);
    return false;
  }
  return true;
}

}  // namespace codec
}  // namespace chromemedia
