// lyra_stream_state.cc -- ExportStream / ImportStream of BatchLyraEncoder (lyra_batch_codec.h) and DeviceLyraDecoder
// (lyra_device_decoder.h): the C blob of lyra_hip_export_streams behind a class header
//   0 u32 kClassMagic   4 u32 kind (1 BatchLyraEncoder, 2 DeviceLyraDecoder)   8 i32 sample_rate_hz   12 u32 zero
// A translation unit of its own: the only one that needs the stream-state calls of the C ABI.
#include <cstring>

#include "../../include/lyra_hip.h"
#include "../csrc/stream_blob.h"
#include "glog/logging.h"
#include "lyra_batch_codec.h"
#include "lyra_device_decoder.h"

namespace chromemedia {
namespace codec {
namespace {

constexpr uint32_t kClassMagic = 0x4243594Cu;   // "LYCB"
constexpr uint32_t kKindEncoder = 1, kKindDeviceDecoder = 2;
constexpr size_t kClassHeaderBytes = 16;

bool StreamExists(int stream, int num_streams) {
  if (stream >= 0 && stream < num_streams) return true;
  LOG(ERROR) << "Stream " << stream << " does not exist.";
  return false;
}

std::optional<std::vector<uint8_t>> Export(lyra_hip_ctx* ctx, int stream, uint32_t kind, int sample_rate_hz) {
  std::vector<uint8_t> blob(kClassHeaderBytes + lyra_hip_stream_blob_bytes());
  const uint32_t header[4] = {kClassMagic, kind, static_cast<uint32_t>(sample_rate_hz), 0};
  std::memcpy(blob.data(), header, sizeof header);
  const int32_t id = stream;
  if (lyra_hip_export_streams(ctx, &id, 1, blob.data() + kClassHeaderBytes) != 0) {
    LOG(ERROR) << "Could not export stream " << stream << ": " << lyra_hip_last_error(ctx);
    return std::nullopt;
  }
  return blob;
}

bool Import(lyra_hip_ctx* ctx, int stream, absl::Span<const uint8_t> blob, uint32_t kind, int sample_rate_hz, unsigned sides) {
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
  if (header[1] != kind) {
    LOG(ERROR) << "The blob was exported by a class of kind " << header[1] << ", this one is of kind " << kind << ".";
    return false;
  }
  if (header[2] != static_cast<uint32_t>(sample_rate_hz)) {
    LOG(ERROR) << "The blob's stream runs at " << header[2] << " Hz, this object at " << sample_rate_hz
               << " Hz: a stream keeps its sample rate.";
    return false;
  }
  const int32_t id = stream;
  if (lyra_hip_import_streams(ctx, &id, 1, blob.data() + kClassHeaderBytes, sides) != 0) {
    LOG(ERROR) << "Could not import stream " << stream << ": " << lyra_hip_last_error(ctx);
    return false;
  }
  return true;
}

}  // namespace

// What ExportStream / ImportStream (`method`) check first: the stream exists and no hop is in flight.
bool BatchLyraEncoder::StreamIdle(const char* method, int stream) const {
  if (!StreamExists(stream, num_streams_)) return false;
  if (in_flight_.empty()) return true;
  LOG(ERROR) << method << "() while " << in_flight_.size() << " EncodeAsync() hops are in flight: call WaitEncoded() first.";
  return false;
}

std::optional<std::vector<uint8_t>> BatchLyraEncoder::ExportStream(int stream) {
  if (!StreamIdle("ExportStream", stream)) return std::nullopt;
  return Export(ctx_, stream, kKindEncoder, sample_rate_hz_);
}

bool BatchLyraEncoder::ImportStream(int stream, absl::Span<const uint8_t> blob) {
  if (!StreamIdle("ImportStream", stream)) return false;
  return Import(ctx_, stream, blob, kKindEncoder, sample_rate_hz_, LYRA_HIP_STATE_ENCODER);
}

// The same for the decoder: the stream exists, the decoder has not failed and no request is in flight.
bool DeviceLyraDecoder::StreamIdle(const char* method, int stream) const {
  if (!StreamExists(stream, num_streams_)) return false;
  if (!failed_ && pending_.empty()) return true;
  LOG(ERROR) << method << "() on a failed decoder or while " << pending_.size()
             << " DecodeSamplesAsync() requests are in flight: call WaitDecoded() first.";
  return false;
}

std::optional<std::vector<uint8_t>> DeviceLyraDecoder::ExportStream(int stream) {
  if (!StreamIdle("ExportStream", stream)) return std::nullopt;
  // the packet belongs to the stream: to the device first (the second-packet path)
  if (staged_bytes_[stream] != 0 && !FlushStaged()) return std::nullopt;
  return Export(ctx_, stream, kKindDeviceDecoder, sample_rate_hz_);
}

bool DeviceLyraDecoder::ImportStream(int stream, absl::Span<const uint8_t> blob) {
  if (!StreamIdle("ImportStream", stream)) return false;
  if (!Import(ctx_, stream, blob, kKindDeviceDecoder, sample_rate_hz_, LYRA_HIP_STATE_DECODER)) return false;
  // the device's seven integers as the blob holds them (validated by the import) -> the host mirror
  std::memcpy(&state_[stream], blob.data() + kClassHeaderBytes + lyra::sb::region_off(lyra::st::R_CNG) + lyra::DS_STATE,
              sizeof(lyra::DsState));
  staged_bytes_[stream] = 0;
  return true;
}

}  // namespace codec
}  // namespace chromemedia
