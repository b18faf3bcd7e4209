// lyra_device_decoder_any.cc -- see lyra_device_decoder_any.h.
#include "lyra_device_decoder_any.h"

#include <cstring>

#include "../../include/lyra_hip_decode_samples_any.h"
#include "../csrc/stream_blob.h"
#include "glog/logging.h"
#include "host_common.h"

namespace chromemedia {
namespace codec {
using namespace host;

namespace {
// the class header of lyra_stream_state.cc: 0 u32 magic, 4 u32 kind, 8 i32 sample_rate_hz, 12 u32 zero
constexpr uint32_t kClassMagic = 0x4243594Cu;   // "LYCB"
constexpr uint32_t kKindDeviceDecoder = 2, kKindAnySizeDeviceDecoder = 3;
constexpr size_t kClassHeaderBytes = 16;
}  // namespace

AnySizeDeviceLyraDecoder::AnySizeDeviceLyraDecoder(lyra_hip_ctx* ctx, int sample_rate_hz, int num_streams)
    : ctx_(ctx), sample_rate_hz_(sample_rate_hz), num_streams_(num_streams), all_ids_(Iota(num_streams)),
      state_(num_streams, lyra::DsState{0, 0, 0, 0, 0, 0, 0}), left_(num_streams, 0),
      staged_(static_cast<size_t>(num_streams) * LYRA_HIP_MAX_PACKET_BYTES), staged_bytes_(num_streams, 0) {}

std::unique_ptr<AnySizeDeviceLyraDecoder> AnySizeDeviceLyraDecoder::Create(int sample_rate_hz, int num_channels,
                                                                            const ghc::filesystem::path& model_path,
                                                                            int num_streams, int device) {
  if (!ParamsSupported(sample_rate_hz, num_channels, num_streams)) return nullptr;
  lyra_hip_ctx* ctx = NewContext(model_path, device, num_streams);
  if (ctx == nullptr) {
    LOG(ERROR) << "New model could not be instantiated.";
    return nullptr;
  }
  if (lyra_hip_set_stream_priorities(ctx, 0, 2, 2) != 0) LOG(WARNING) << "stream priorities: " << lyra_hip_last_error(ctx);
  return std::unique_ptr<AnySizeDeviceLyraDecoder>(new AnySizeDeviceLyraDecoder(ctx, sample_rate_hz, num_streams));
}

AnySizeDeviceLyraDecoder::~AnySizeDeviceLyraDecoder() { lyra_hip_destroy(ctx_); }

bool AnySizeDeviceLyraDecoder::is_comfort_noise(int stream) const {
  return stream >= 0 && stream < num_streams_ && state_[stream].fade == lyra::LOSSY_FADE;
}

int AnySizeDeviceLyraDecoder::leftover_samples(int stream) const {
  return stream >= 0 && stream < num_streams_ ? left_[stream] : -1;
}

bool AnySizeDeviceLyraDecoder::SetEncodedPackets(absl::Span<const uint8_t> encoded) {
  return SetEncodedPackets(absl::MakeConstSpan(all_ids_), encoded);
}

bool AnySizeDeviceLyraDecoder::SetEncodedPackets(absl::Span<const int32_t> streams, absl::Span<const uint8_t> encoded) {
  const int packet_size = CheckEncodedPackets(failed_, streams, encoded, num_streams_);
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

bool AnySizeDeviceLyraDecoder::Begin(int num_samples) {
  if (lyra_hip_decode_samples_any_begin(ctx_, all_ids_.data(), num_streams_, staged_.data(), staged_bytes_.data(), num_samples,
                                        sample_rate_hz_) != 0) {
    failed_ = true;
    LOG(ERROR) << "Could not decode samples: " << lyra_hip_last_error(ctx_);
    return false;
  }
  const int rounds = lyra::ds_any_rounds(num_samples, sample_rate_hz_);
  for (int s = 0; s < num_streams_; ++s) {   // what the device's plan kernel does with the same inputs, round by round
    const lyra::DsaStep step = lyra::ds_any_step(left_[s], num_samples, sample_rate_hz_);
    left_[s] = step.left;
    for (int r = 0; r < (rounds > 0 ? rounds : 1); ++r)
      state_[s] = lyra::ds_plan(state_[s], r == 0 && staged_bytes_[s] != 0, lyra::ds_any_round_total(step.n_int, r)).s;
    staged_bytes_[s] = 0;
  }
  return true;
}

bool AnySizeDeviceLyraDecoder::FlushStaged() {
  if (!Begin(0)) return false;
  if (lyra_hip_decode_samples_any_end(ctx_, nullptr) != 0) {
    failed_ = true;
    LOG(ERROR) << "Could not queue packets: " << lyra_hip_last_error(ctx_);
    return false;
  }
  return true;
}

std::optional<std::vector<int16_t>> AnySizeDeviceLyraDecoder::DecodeSamples(int num_samples) {
  if (num_samples < 0) {
    LOG(ERROR) << kNegativeSamples;
    return std::nullopt;
  }
  std::vector<int16_t> out(static_cast<size_t>(num_streams_) * num_samples);
  if (!DecodeSamples(num_samples, absl::Span<int16_t>(out.data(), out.size()))) return std::nullopt;
  return out;
}

bool AnySizeDeviceLyraDecoder::DecodeSamples(int num_samples, absl::Span<int16_t> out) {
  if (!pending_.empty()) {
    LOG(ERROR) << "DecodeSamples() while " << pending_.size() << " DecodeSamplesAsync() requests are in flight: call WaitDecoded() first.";
    return false;
  }
  return DecodeSamplesAsync(num_samples) && WaitDecoded(out);
}

bool AnySizeDeviceLyraDecoder::DecodeSamplesAsync(int num_samples) {
  if (num_samples < 0) {
    LOG(ERROR) << kNegativeSamples;
    return false;
  }
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  if (!lyra::ds_any_valid(num_samples, sample_rate_hz_)) {
    LOG(ERROR) << "A request of " << num_samples << " samples at " << sample_rate_hz_ << " Hz is above the device decoder's "
               << lyra::DSA_MAX_HOPS << " hops per request (" << lyra::DSA_MAX_HOPS * (sample_rate_hz_ / 50)
               << " samples): ask for it in several requests.";
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

bool AnySizeDeviceLyraDecoder::WaitDecoded(absl::Span<int16_t> out) {
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
  if (lyra_hip_decode_samples_any_end(ctx_, out.data()) != 0) {
    failed_ = true;
    LOG(ERROR) << "Could not decode samples: " << lyra_hip_last_error(ctx_);
    return false;
  }
  return true;
}

// ---- ExportStream / ImportStream ---------------------------------------------------------------------------------------
bool AnySizeDeviceLyraDecoder::StreamIdle(const char* method, int stream) const {
  if (stream < 0 || stream >= num_streams_) {
    LOG(ERROR) << "Stream " << stream << " does not exist.";
    return false;
  }
  if (!failed_ && pending_.empty()) return true;
  LOG(ERROR) << method << "() on a failed decoder or while " << pending_.size()
             << " DecodeSamplesAsync() requests are in flight: call WaitDecoded() first.";
  return false;
}

std::optional<std::vector<uint8_t>> AnySizeDeviceLyraDecoder::ExportStream(int stream) {
  if (!StreamIdle("ExportStream", stream)) return std::nullopt;
  // the packet belongs to the stream: to the device first (the second-packet path)
  if (staged_bytes_[stream] != 0 && !FlushStaged()) return std::nullopt;
  std::vector<uint8_t> blob(kClassHeaderBytes + lyra_hip_stream_blob_bytes());
  const uint32_t header[4] = {kClassMagic, kKindAnySizeDeviceDecoder, static_cast<uint32_t>(sample_rate_hz_), 0};
  std::memcpy(blob.data(), header, sizeof header);
  const int32_t id = stream;
  if (lyra_hip_export_streams(ctx_, &id, 1, blob.data() + kClassHeaderBytes) != 0) {
    LOG(ERROR) << "Could not export stream " << stream << ": " << lyra_hip_last_error(ctx_);
    return std::nullopt;
  }
  return blob;
}

bool AnySizeDeviceLyraDecoder::ImportStream(int stream, absl::Span<const uint8_t> blob) {
  if (!StreamIdle("ImportStream", stream)) return false;
  if (blob.size() != kClassHeaderBytes + lyra_hip_stream_blob_bytes()) {
    LOG(ERROR) << "A stream blob has " << kClassHeaderBytes + lyra_hip_stream_blob_bytes() << " bytes, not " << blob.size() << ".";
    return false;
  }
  uint32_t header[4];
  std::memcpy(header, blob.data(), sizeof header);
  if (header[0] != kClassMagic || header[3] != 0) {
    LOG(ERROR) << "Not a stream blob of this library's classes.";
    return false;
  }
  if (header[1] != kKindAnySizeDeviceDecoder && header[1] != kKindDeviceDecoder) {
    LOG(ERROR) << "The blob was exported by a class of kind " << header[1] << ", this one takes kinds "
               << kKindAnySizeDeviceDecoder << " and " << kKindDeviceDecoder << ".";
    return false;
  }
  if (header[2] != static_cast<uint32_t>(sample_rate_hz_)) {
    LOG(ERROR) << "The blob's stream runs at " << header[2] << " Hz, this object at " << sample_rate_hz_
               << " Hz: a stream keeps its sample rate.";
    return false;
  }
  const int32_t id = stream;
  const uint8_t* dev_blob = blob.data() + kClassHeaderBytes;
  if (lyra_hip_import_streams(ctx_, &id, 1, dev_blob, LYRA_HIP_STATE_DECODER) != 0) {
    LOG(ERROR) << "Could not import stream " << stream << ": " << lyra_hip_last_error(ctx_);
    return false;
  }
  // the device's integers as the blob holds them (validated by the import) -> the host mirror
  std::memcpy(&state_[stream], dev_blob + lyra::sb::region_off(lyra::st::R_CNG) + lyra::DS_STATE, sizeof(lyra::DsState));
  int32_t left = 0;
  std::memcpy(&left, dev_blob + lyra::sb::region_off(lyra::st::R_RS_D) + lyra::DSA_LEFT_COUNT, sizeof left);
  left_[stream] = left;
  staged_bytes_[stream] = 0;
  return true;
}

}  // namespace codec
}  // namespace chromemedia
