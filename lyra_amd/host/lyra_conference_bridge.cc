// lyra_conference_bridge.cc -- see lyra_conference_bridge.h.  Plain C++17 over the C ABI (include/lyra_hip_bridge.h); no HIP
// here.  A translation unit of its own: the calls it needs are not among those the other host classes are built against.
#include "lyra_conference_bridge.h"

#include <algorithm>
#include <cstring>

#include "../../include/lyra_hip_bridge.h"
#include "glog/logging.h"
#include "host_common.h"

namespace chromemedia {
namespace codec {
using namespace host;

static_assert(kBridgePacketRowBytes == LYRA_HIP_MAX_PACKET_BYTES, "packet row stride");

namespace {
int BitrateToBits(int bitrate) {   // BitrateToNumQuantizedBits, lyra_config.h: 3200 / 6000 / 9200 -> 64 / 120 / 184
  return bitrate == 3200 ? 64 : bitrate == 6000 ? 120 : bitrate == 9200 ? 184 : -1;
}
}  // namespace

LyraConferenceBridge::LyraConferenceBridge(lyra_hip_ctx* ctx, absl::Span<const BridgeStream> streams, bool skip_comfort_noise)
    : ctx_(ctx),
      flags_(skip_comfort_noise ? LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE : 0u),
      ids_(Iota(static_cast<int>(streams.size()))),
      rooms_(streams.size(), -1),
      muted_(streams.size(), 0),
      staged_(streams.size() * kBridgePacketRowBytes, 0),
      staged_bytes_(streams.size(), 0),
      noise_(streams.size(), 0),
      cn_(streams.size(), 0) {
  for (const BridgeStream& s : streams) {
    bits_.push_back(BitrateToBits(s.bitrate));
    dtx_.push_back(s.enable_dtx ? 1 : 0);
  }
}

lyra_hip_ctx* LyraConferenceBridge::NewBridgeContext(absl::Span<const BridgeStream> streams,
                                                     const ghc::filesystem::path& model_path, int device,
                                                     int extra_streams) {
  const int n = static_cast<int>(streams.size());
  if (n == 0) {
    LOG(ERROR) << "num_streams must be positive.";
    return nullptr;
  }
  for (const BridgeStream& s : streams)
    if (BitrateToBits(s.bitrate) < 0) {
      LOG(ERROR) << "Bitrate " << s.bitrate << " bps is not supported by codec.";
      return nullptr;
    }
  lyra_hip_ctx* ctx = NewContext(model_path, device, n + extra_streams);
  if (ctx == nullptr) LOG(ERROR) << "Could not create the bridge's context.";
  return ctx;
}

std::unique_ptr<LyraConferenceBridge> LyraConferenceBridge::Create(absl::Span<const BridgeStream> streams,
                                                                  const ghc::filesystem::path& model_path, int device,
                                                                  bool skip_comfort_noise) {
  lyra_hip_ctx* ctx = NewBridgeContext(streams, model_path, device);
  if (ctx == nullptr) return nullptr;
  return std::unique_ptr<LyraConferenceBridge>(new LyraConferenceBridge(ctx, streams, skip_comfort_noise));
}

int LyraConferenceBridge::BeginTick(lyra_hip_ctx* ctx, const int32_t* ids, int n, const uint8_t* packets,
                                    const int32_t* packet_bytes, const int32_t* rooms, const int32_t* muted, unsigned flags,
                                    const int32_t* bits, const int32_t* dtx) {
  return lyra_hip_bridge_begin(ctx, ids, n, packets, packet_bytes, rooms, muted, flags, bits, dtx);
}

int LyraConferenceBridge::EndTick(lyra_hip_ctx* ctx, uint8_t* rows, int32_t* lengths, int32_t* is_noise,
                                  int32_t* is_comfort_noise) {
  return lyra_hip_bridge_end(ctx, rows, lengths, is_noise, is_comfort_noise);
}

LyraConferenceBridge::~LyraConferenceBridge() { lyra_hip_destroy(ctx_); }

bool LyraConferenceBridge::SetRoom(int stream, int room) {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  if (!Exists(stream)) {
    LOG(ERROR) << "Stream " << stream << " does not exist.";
    return false;
  }
  if (room >= 0 && room != rooms_[stream] &&
      std::count(rooms_.begin(), rooms_.end(), room) >= LYRA_HIP_BRIDGE_MAX_ROOM) {
    LOG(ERROR) << "Room " << room << " already has " << LYRA_HIP_BRIDGE_MAX_ROOM << " members.";
    return false;
  }
  rooms_[stream] = room < 0 ? -1 : room;
  return true;
}

bool LyraConferenceBridge::SetMuted(int stream, bool muted) {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  if (!Exists(stream)) {
    LOG(ERROR) << "Stream " << stream << " does not exist.";
    return false;
  }
  muted_[stream] = muted ? 1 : 0;
  return true;
}

bool LyraConferenceBridge::set_bitrate(int stream, int bitrate) {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  if (!Exists(stream)) {
    LOG(ERROR) << "Stream " << stream << " does not exist.";
    return false;
  }
  const int bits = BitrateToBits(bitrate);
  if (bits < 0) {
    LOG(ERROR) << "Bitrate " << bitrate << " bps is not supported by codec.";
    return false;
  }
  bits_[stream] = bits;
  return true;
}

bool LyraConferenceBridge::ResetStream(int stream) {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  if (!Exists(stream)) {
    LOG(ERROR) << "Stream " << stream << " does not exist.";
    return false;
  }
  const int32_t id = ids_[stream];
  if (lyra_hip_reset_streams(ctx_, &id, 1) != 0) {
    LOG(ERROR) << "Unable to reset stream " << stream << ": " << lyra_hip_last_error(ctx_);
    failed_ = true;
    return false;
  }
  staged_bytes_[stream] = 0;
  noise_[stream] = cn_[stream] = 0;
  ForgetStream(stream);
  return true;
}

bool LyraConferenceBridge::SetEncodedPackets(absl::Span<const uint8_t> rows, absl::Span<const int32_t> lengths) {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  const size_t n = static_cast<size_t>(num_streams());
  if (lengths.size() != n || rows.size() != n * kBridgePacketRowBytes) {
    LOG(ERROR) << "SetEncodedPackets takes " << n << " rows of " << kBridgePacketRowBytes << " bytes and " << n
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
      LOG(ERROR) << "Stream " << s << " already has a packet for the next tick: one packet per stream and tick.";
      return false;
    }
  }
  for (size_t s = 0; s < n; ++s) {
    if (lengths[s] == 0) continue;
    std::memcpy(&staged_[s * kBridgePacketRowBytes], &rows[s * kBridgePacketRowBytes], static_cast<size_t>(lengths[s]));
    staged_bytes_[s] = lengths[s];
  }
  return true;
}

bool LyraConferenceBridge::SetEncodedPacket(int stream, absl::Span<const uint8_t> packet) {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  if (!Exists(stream)) {
    LOG(ERROR) << "Stream " << stream << " does not exist.";
    return false;
  }
  if (PacketSizeToBits(static_cast<int>(packet.size())) < 0) {
    LOG(ERROR) << "The packet size (" << packet.size() << " bytes) is not supported.";
    return false;
  }
  if (staged_bytes_[stream] != 0) {
    LOG(ERROR) << "Stream " << stream << " already has a packet for the next tick: one packet per stream and tick.";
    return false;
  }
  std::memcpy(&staged_[static_cast<size_t>(stream) * kBridgePacketRowBytes], packet.data(), packet.size());
  staged_bytes_[stream] = static_cast<int32_t>(packet.size());
  return true;
}

bool LyraConferenceBridge::TickAsync() {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  if (in_flight_ >= 2) {
    LOG(ERROR) << "Two ticks are already in flight: call WaitTick() first.";
    return false;
  }
  // (begin() copies every array at call time: rooms, mutes and bitrates set after it reach the next tick only)
  if (BeginTick(ctx_, ids_.data(), num_streams(), staged_.data(), staged_bytes_.data(), rooms_.data(), muted_.data(), flags_,
                bits_.data(), dtx_.data()) != 0) {
    LOG(ERROR) << "Unable to run the tick: " << lyra_hip_last_error(ctx_);
    failed_ = true;
    return false;
  }
  std::fill(staged_bytes_.begin(), staged_bytes_.end(), 0);   // the staging belongs to the tick begun
  ++in_flight_;
  return true;
}

bool LyraConferenceBridge::WaitTick(absl::Span<uint8_t> rows, absl::Span<int32_t> lengths) {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return false;
  }
  if (in_flight_ == 0) {
    LOG(ERROR) << "WaitTick() without a tick in flight.";
    return false;
  }
  const size_t n = static_cast<size_t>(num_streams());
  if (rows.size() != n * kBridgePacketRowBytes || lengths.size() != n) {
    LOG(ERROR) << "The output has to hold exactly " << n << " rows of " << kBridgePacketRowBytes << " bytes and " << n
               << " lengths, but holds " << rows.size() << " bytes and " << lengths.size() << " lengths.";
    return false;
  }
  --in_flight_;
  if (EndTick(ctx_, rows.data(), lengths.data(), noise_.data(), cn_.data()) != 0) {
    LOG(ERROR) << "Unable to run the tick: " << lyra_hip_last_error(ctx_);
    failed_ = true;   // the tick's packets are lost and the streams have moved on
    return false;
  }
  return true;
}

std::optional<std::pair<std::vector<uint8_t>, std::vector<int32_t>>> LyraConferenceBridge::Tick() {
  if (failed_) {
    LOG(ERROR) << kFailed;
    return std::nullopt;
  }
  if (in_flight_ != 0) {
    LOG(ERROR) << "Tick() while " << in_flight_ << " TickAsync() ticks are in flight: call WaitTick() first.";
    return std::nullopt;
  }
  if (!TickAsync()) return std::nullopt;
  std::pair<std::vector<uint8_t>, std::vector<int32_t>> out;
  out.first.resize(static_cast<size_t>(num_streams()) * kBridgePacketRowBytes);
  out.second.resize(static_cast<size_t>(num_streams()));
  if (!WaitTick(absl::Span<uint8_t>(out.first.data(), out.first.size()), absl::Span<int32_t>(out.second.data(), out.second.size())))
    return std::nullopt;
  return out;
}

bool LyraConferenceBridge::is_comfort_noise(int stream) const { return Exists(stream) && cn_[stream] != 0; }

bool LyraConferenceBridge::is_noise(int stream) const { return Exists(stream) && noise_[stream] != 0; }

}  // namespace codec
}  // namespace chromemedia
