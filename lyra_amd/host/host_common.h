// host_common.h -- what BatchLyraEncoder, BatchLyraDecoder (lyra_batch_codec.cc) and DeviceLyraDecoder
// (lyra_device_decoder.cc) share.  Internal and header-only: no translation unit of its own, so every build line that lists
// the sources stays as it is.
#ifndef LYRA_AMD_HOST_HOST_COMMON_H_
#define LYRA_AMD_HOST_HOST_COMMON_H_
#include <cstdint>
#include <vector>

#include "../../include/lyra_hip.h"
#include "absl/types/span.h"
#include "glog/logging.h"
#include "include/ghc/filesystem.hpp"

namespace chromemedia {
namespace codec {
namespace host {

constexpr char kFailed[] =
    "This decoder failed in the middle of a request; its streams are out of step with the device. Create a new one.";
constexpr char kNegativeSamples[] = "Number of samples has to be non-negative.";

// lyra_config.h:56,131-143 (AreParamsSupported)
inline bool ParamsSupported(int sample_rate_hz, int num_channels, int num_streams) {
  if (sample_rate_hz != 8000 && sample_rate_hz != 16000 && sample_rate_hz != 32000 && sample_rate_hz != 48000) {
    LOG(ERROR) << "Sample rate " << sample_rate_hz << " Hz is not supported by codec.";
    return false;
  }
  if (num_channels != 1) {
    LOG(ERROR) << "Number of channels " << num_channels << " is not supported by codec. It needs to be 1.";
    return false;
  }
  if (num_streams < 1) {
    LOG(ERROR) << "num_streams must be positive.";
    return false;
  }
  return true;
}

inline lyra_hip_ctx* NewContext(const ghc::filesystem::path& model_path, int device, int num_streams) {
  lyra_hip_ctx* ctx = nullptr;
  if (lyra_hip_create(model_path.string().c_str(), device, num_streams, LYRA_HIP_REQUANT_DEFAULT, &ctx) != 0) {
    LOG(ERROR) << "lyra_hip_create failed: " << lyra_hip_last_error(nullptr);
    return nullptr;
  }
  return ctx;
}

inline std::vector<int32_t> Iota(int n) {
  std::vector<int32_t> v(n);
  for (int i = 0; i < n; ++i) v[i] = i;
  return v;
}

inline int PacketSizeToBits(int packet_size) {  // PacketSizeToNumQuantizedBits, lyra_config.h:99-106
  switch (packet_size) {
    case 8: return 64;
    case 15: return 120;
    case 23: return 184;
    default: return -1;
  }
}

// The head of both decoders' SetEncodedPackets(streams, encoded): the bytes of one packet when the call is well formed,
// 0 when there is nothing to do (no streams, no bytes), -1 when the call is refused.
inline int CheckEncodedPackets(bool failed, absl::Span<const int32_t> streams, absl::Span<const uint8_t> encoded,
                               int num_streams) {
  if (failed) {
    LOG(ERROR) << kFailed;
    return -1;
  }
  if (streams.empty()) return encoded.empty() ? 0 : -1;
  const int packet_size = static_cast<int>(encoded.size() / streams.size());
  if (encoded.size() % streams.size() != 0 || PacketSizeToBits(packet_size) < 0) {
    LOG(ERROR) << "The packet size (" << encoded.size() << " bytes for " << streams.size()
               << " streams) is not supported.";
    return -1;
  }
  for (int32_t id : streams)
    if (id < 0 || id >= num_streams) {
      LOG(ERROR) << "Stream " << id << " does not exist.";
      return -1;
    }
  return packet_size;
}

}  // namespace host
}  // namespace codec
}  // namespace chromemedia
#endif
