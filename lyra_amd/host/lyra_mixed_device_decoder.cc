// lyra_mixed_device_decoder.cc -- see lyra_mixed_device_decoder.h.
#include "lyra_mixed_device_decoder.h"

#include <cstring>

#include "../../include/lyra_hip_decode_samples_streams.h"
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

MixedAnySizeDeviceLyraDecoder::MixedAnySizeDeviceLyraDecoder(lyra_hip_ctx* ctx, absl::Span<const int> sample_rates_hz)
    : ctx_(ctx), num_streams_(static_cast<int>(sample_rates_hz.size())), rates_(sample_rates_hz.begin(), sample_rates_hz.end()),
      state_(num_streams_, lyra::DsState{0, 0, 0, 0, 0, 0, 0}), left_(num_streams_, 0),
      staged_(static_cast<size_t>(num_streams_) * LYRA_HIP_MAX_PACKET_BYTES), staged_bytes_(num_streams_, 0),
      row_of_(num_streams_, -1) {}

std::unique_ptr<MixedAnySizeDeviceLyraDecoder> MixedAnySizeDeviceLyraDecoder::Create(absl::Span<const int> sample_rates_hz,
                                                                                      const ghc::filesystem::path& model_path,
                                                                                      int device) {
  if (sample_rates_hz.empty()) {
    LOG(ERROR) << "num_streams must be positive.";
    return nullptr;
  }
  const int n = static_cast<int>(sample_rates_hz.size());
  for (int rate : sample_rates_hz)
    if (!ParamsSupported(rate, 1, n)) return nullptr;
  lyra_hip_ctx* ctx = NewContext(model_path, device, n);
  if (ctx == nullptr) {
    LOG(ERROR) << "New model could not be instantiated.";
    return nullptr;
  }
  if (lyra_hip_set_stream_priorities(ctx, 0, 2, 2) != 0) LOG(WARNING) << "stream priorities: " << lyra_hip_last_error(ctx);
  return std::unique_ptr<MixedAnySizeDeviceLyraDecoder>(new MixedAnySizeDeviceLyraDecoder(ctx, sample_rates_hz));
}

MixedAnySizeDeviceLyraDecoder::~MixedAnySizeDeviceLyraDecoder() { lyra_hip_destroy(ctx_); }

bool MixedAnySizeDeviceLyraDecoder::is_comfort_noise(int stream) const {
  return stream >= 0 && stream < num_streams_ && state_[stream].fade == lyra::LOSSY_FADE;
}

int MixedAnySizeDeviceLyraDecoder::leftover_samples(int stream) const {
  return stream >= 0 && stream < num_streams_ ? left_[stream] : -1;
}

bool MixedAnySizeDeviceLyraDecoder::SetEncodedPackets(absl::Span<const int32_t> streams, absl::Span<const uint8_t> encoded) {
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

bool MixedAnySizeDeviceLyraDecoder::Begin(absl::Span<const int32_t> streams, absl::Span<const int> num_samples, long* total) {
  call_ids_.clear(); call_bytes_.clear(); call_rates_.clear(); call_sizes_.clear(); call_packets_.clear();
  auto add_row = [&](int32_t s, int n) {
    row_of_[s] = static_cast<int32_t>(call_ids_.size());
    call_ids_.push_back(s);
    call_bytes_.push_back(staged_bytes_[s]);
    call_rates_.push_back(rates_[s]);
    call_sizes_.push_back(n);
    const uint8_t* p = staged_.data() + static_cast<size_t>(s) * LYRA_HIP_MAX_PACKET_BYTES;
    call_packets_.insert(call_packets_.end(), p, p + LYRA_HIP_MAX_PACKET_BYTES);
  };
  for (size_t i = 0; i < streams.size(); ++i) add_row(streams[i], num_samples[i]);
  for (int s = 0; s < num_streams_; ++s)
    if (row_of_[s] < 0 && staged_bytes_[s] != 0) add_row(s, 0);
  for (int32_t s : call_ids_) row_of_[s] = -1;
  *total = lyra::dss_packed_offsets(call_sizes_.data(), static_cast<int>(call_sizes_.size()), nullptr);
  if (call_ids_.empty()) return true;   // nothing to play, nothing staged
  const int B = static_cast<int>(call_ids_.size());
  if (lyra_hip_decode_samples_streams_begin(ctx_, call_ids_.data(), B, call_packets_.data(), call_bytes_.data(),
                                            call_rates_.data(), call_sizes_.data()) != 0) {
    failed_ = true;
    LOG(ERROR) << "Could not decode samples: " << lyra_hip_last_error(ctx_);
    return false;
  }
  for (int b = 0; b < B; ++b) {   // what the device's plan kernel does with the same inputs, round by round
    const int s = call_ids_[b];
    const lyra::DsaStep step = lyra::ds_any_step(left_[s], call_sizes_[b], rates_[s]);
    left_[s] = step.left;
    const int rounds = lyra::ds_any_rounds(call_sizes_[b], rates_[s]);   // (the call's further rounds plan 0 samples: no-ops)
    for (int r = 0; r < (rounds > 0 ? rounds : 1); ++r)
      state_[s] = lyra::ds_plan(state_[s], r == 0 && call_bytes_[b] != 0, lyra::ds_any_round_total(step.n_int, r)).s;
    staged_bytes_[s] = 0;
  }
  return true;
}

bool MixedAnySizeDeviceLyraDecoder::FlushStaged() {
  long total = 0;
  if (!Begin(absl::Span<const int32_t>(), absl::Span<const int>(), &total)) return false;
  if (call_ids_.empty()) return true;
  if (lyra_hip_decode_samples_streams_end(ctx_, nullptr, nullptr, nullptr) != 0) {
    failed_ = true;
    LOG(ERROR) << "Could not queue packets: " << lyra_hip_last_error(ctx_);
    return false;
  }
  return true;
}

std::optional<std::vector<int16_t>> MixedAnySizeDeviceLyraDecoder::DecodeSamples(absl::Span<const int32_t> streams,
                                                                                 absl::Span<const int> num_samples) {
  size_t total = 0;
  for (int n : num_samples) total += n > 0 ? static_cast<size_t>(n) : 0;
  std::vector<int16_t> out(total);
  if (!DecodeSamples(streams, num_samples, absl::Span<int16_t>(out.data(), out.size()))) return std::nullopt;
  return out;
}

bool MixedAnySizeDeviceLyraDecoder::DecodeSamples(absl::Span<const int32_t> streams, absl::Span<const int> num_samples,
                                                  absl::Span<int16_t> out_packed) {
  if (!pending_.empty()) {
    LOG(ERROR) << "DecodeSamples() while " << pending_.size() << " DecodeSamplesAsync() requests are in flight: call WaitDecoded() first.";
    return false;
  }
  size_t total = 0;
  for (int n : num_samples) total += n > 0 ? static_cast<size_t>(n) : 0;
  if (out_packed.size() != total) {   // (before anything is begun: a refused request consumes nothing)
    LOG(ERROR) << "Output span has " << out_packed.size() << " samples, expected " << total;
    return false;
  }
  return DecodeSamplesAsync(streams, num_samples) && WaitDecoded(out_packed);
}

bool MixedAnySizeDeviceLyraDecoder::RowAcceptable(int32_t s, int n) const {
  if (s < 0 || s >= num_streams_) {
    LOG(ERROR) << "Stream " << s << " does not exist.";
  } else if (row_of_[s] >= 0) {
    LOG(ERROR) << "Stream " << s << " is named twice in one request.";
  } else if (n < 0) {
    LOG(ERROR) << kNegativeSamples;
  } else if (lyra::dss_size_verdict(rates_[s], n) != lyra::DSS_OK) {
    LOG(ERROR) << "A request of " << n << " samples at " << rates_[s] << " Hz (stream " << s << ") is above the device "
               << "decoder's " << lyra::DSA_MAX_HOPS << " hops per request (" << lyra::DSA_MAX_HOPS * (rates_[s] / 50)
               << " samples): ask for it in several requests.";
  } else {
    return true;
  }
  return false;
}

bool MixedAnySizeDeviceLyraDecoder::DecodeSamplesAsync(absl::Span<const int32_t> streams, absl::Span<const int> num_samples) {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  if (streams.size() != num_samples.size()) {
    LOG(ERROR) << streams.size() << " streams, but " << num_samples.size() << " request sizes.";
    return false;
  }
  size_t seen = 0;   // (row_of_ marks the streams seen so far: a stream named twice shows)
  while (seen < streams.size() && RowAcceptable(streams[seen], num_samples[seen])) row_of_[streams[seen++]] = 0;
  for (size_t i = 0; i < seen; ++i) row_of_[streams[i]] = -1;
  if (seen != streams.size()) return false;
  if (pending_.size() >= 2) {
    LOG(ERROR) << "Two requests are already in flight: call WaitDecoded() first.";
    return false;
  }
  long total = 0;
  if (!Begin(streams, num_samples, &total)) return false;
  pending_.push_back(call_ids_.empty() ? -1 : total);   // (-1: nothing went to the device)
  return true;
}

bool MixedAnySizeDeviceLyraDecoder::WaitDecoded(absl::Span<int16_t> out_packed) {
  if (pending_.empty()) {
    LOG(ERROR) << "WaitDecoded() without a request in flight.";
    return false;
  }
  const long total = pending_.front() < 0 ? 0 : pending_.front();
  if (out_packed.size() != static_cast<size_t>(total)) {
    LOG(ERROR) << "Output span has " << out_packed.size() << " samples, expected " << total;
    return false;
  }
  const bool on_device = pending_.front() >= 0;
  pending_.erase(pending_.begin());
  if (on_device && lyra_hip_decode_samples_streams_end(ctx_, total > 0 ? out_packed.data() : nullptr, nullptr, nullptr) != 0) {
    failed_ = true;
    LOG(ERROR) << "Could not decode samples: " << lyra_hip_last_error(ctx_);
    return false;
  }
  return true;
}

// ---- ExportStream / ImportStream ---------------------------------------------------------------------------------------
bool MixedAnySizeDeviceLyraDecoder::StreamIdle(const char* method, int stream) const {
  if (stream < 0 || stream >= num_streams_) {
    LOG(ERROR) << "Stream " << stream << " does not exist.";
    return false;
  }
  if (!failed_ && pending_.empty()) return true;
  LOG(ERROR) << method << "() on a failed decoder or while " << pending_.size()
             << " DecodeSamplesAsync() requests are in flight: call WaitDecoded() first.";
  return false;
}

std::optional<std::vector<uint8_t>> MixedAnySizeDeviceLyraDecoder::ExportStream(int stream) {
  if (!StreamIdle("ExportStream", stream)) return std::nullopt;
  // the packet belongs to the stream: to the device first (the second-packet path)
  if (staged_bytes_[stream] != 0 && !FlushStaged()) return std::nullopt;
  std::vector<uint8_t> blob(kClassHeaderBytes + lyra_hip_stream_blob_bytes());
  const uint32_t header[4] = {kClassMagic, kKindAnySizeDeviceDecoder, static_cast<uint32_t>(rates_[stream]), 0};
  std::memcpy(blob.data(), header, sizeof header);
  const int32_t id = stream;
  if (lyra_hip_export_streams(ctx_, &id, 1, blob.data() + kClassHeaderBytes) != 0) {
    LOG(ERROR) << "Could not export stream " << stream << ": " << lyra_hip_last_error(ctx_);
    return std::nullopt;
  }
  return blob;
}

bool MixedAnySizeDeviceLyraDecoder::ImportStream(int stream, absl::Span<const uint8_t> blob) {
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
  if (header[2] != static_cast<uint32_t>(rates_[stream])) {
    LOG(ERROR) << "The blob's stream runs at " << header[2] << " Hz, stream " << stream << " at " << rates_[stream]
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
