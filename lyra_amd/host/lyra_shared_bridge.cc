// lyra_shared_bridge.cc -- see lyra_shared_bridge.h.  Plain C++17 over the C ABI (include/lyra_hip_shared_bridge.h); no HIP
// here.  A translation unit of its own: lyra_conference_bridge.cc and lyra_speaker_bridge.cc stay built against their calls.
#include "lyra_shared_bridge.h"

#include <algorithm>

#include "../../include/lyra_hip_shared_bridge.h"
#include "glog/logging.h"

namespace chromemedia {
namespace codec {

static_assert(kSharedBridgeMaxSpeakers == LYRA_HIP_SPEAKERS_MAX, "the selection's bound");

namespace {
int RoomBitrateToBits(int bitrate) { return bitrate == 3200 ? 64 : bitrate == 6000 ? 120 : bitrate == 9200 ? 184 : -1; }
}  // namespace

LyraSharedBridge::LyraSharedBridge(lyra_hip_ctx* ctx, absl::Span<const BridgeStream> streams, bool skip_comfort_noise,
                                   int max_speakers, int max_rooms, int default_bits, bool default_dtx)
    : LyraConferenceBridge(ctx, streams, skip_comfort_noise),
      ctx_(ctx),
      max_speakers_(max_speakers),
      room_bits_(static_cast<size_t>(max_rooms), default_bits),
      room_dtx_(static_cast<size_t>(max_rooms), default_dtx ? 1 : 0),
      levels_(streams.size(), 0),
      speaker_(streams.size(), 0),
      slot_(streams.size(), -1) {}

std::unique_ptr<LyraSharedBridge> LyraSharedBridge::Create(absl::Span<const BridgeStream> streams,
                                                          const ghc::filesystem::path& model_path, int device,
                                                          bool skip_comfort_noise, int max_speakers, int max_rooms,
                                                          BridgeStream room_default) {
  if (max_speakers < 1 || max_speakers > kSharedBridgeMaxSpeakers) {
    LOG(ERROR) << "max_speakers must lie in 1.." << kSharedBridgeMaxSpeakers << ", but is " << max_speakers << ".";
    return nullptr;
  }
  if (max_rooms < 1) {
    LOG(ERROR) << "max_rooms must be positive, but is " << max_rooms << ".";
    return nullptr;
  }
  const int bits = RoomBitrateToBits(room_default.bitrate);
  if (bits < 0) {
    LOG(ERROR) << "Bitrate " << room_default.bitrate << " bps is not supported by codec.";
    return nullptr;
  }
  lyra_hip_ctx* ctx = NewBridgeContext(streams, model_path, device, max_rooms * (1 + max_speakers));
  if (ctx == nullptr) return nullptr;
  return std::unique_ptr<LyraSharedBridge>(
      new LyraSharedBridge(ctx, streams, skip_comfort_noise, max_speakers, max_rooms, bits, room_default.enable_dtx));
}

bool LyraSharedBridge::SetRoom(int stream, int room) {
  if (room >= max_rooms()) {
    LOG(ERROR) << "Room " << room << " does not exist: the bridge has " << max_rooms() << " rooms.";
    return false;
  }
  return LyraConferenceBridge::SetRoom(stream, room);
}

bool LyraSharedBridge::SetRoomBitrate(int room, int bitrate) {
  const int bits = RoomBitrateToBits(bitrate);
  if (!RoomExists(room) || bits < 0) {
    LOG(ERROR) << "Room " << room << " does not exist, or bitrate " << bitrate << " bps is not supported by codec.";
    return false;
  }
  room_bits_[room] = bits;
  return true;
}

bool LyraSharedBridge::SetRoomDtx(int room, bool enable_dtx) {
  if (!RoomExists(room)) {
    LOG(ERROR) << "Room " << room << " does not exist.";
    return false;
  }
  room_dtx_[room] = enable_dtx ? 1 : 0;
  return true;
}

bool LyraSharedBridge::ResetRoom(int room) {
  if (!RoomExists(room)) {
    LOG(ERROR) << "Room " << room << " does not exist.";
    return false;
  }
  const int32_t label = room;
  std::vector<int32_t> ids;
  for (int c = 0; c <= max_speakers_; ++c) ids.push_back(num_streams() + room * (1 + max_speakers_) + c);
  if (lyra_hip_shared_reset_rooms(ctx_, &label, 1) != 0 || lyra_hip_reset_streams(ctx_, ids.data(), static_cast<int>(ids.size())) != 0) {
    LOG(ERROR) << "Unable to reset room " << room << ": " << lyra_hip_last_error(ctx_);
    return false;
  }
  return true;
}

int LyraSharedBridge::BeginTick(lyra_hip_ctx* ctx, const int32_t* ids, int n, const uint8_t* packets, const int32_t* packet_bytes,
                                const int32_t* rooms, const int32_t* muted, unsigned flags, const int32_t* /*bits*/,
                                const int32_t* /*dtx*/) {
  // the labels present, ascending; every room's block of 1 + N encoder rows with the room's settings
  labels_.assign(rooms, rooms + n);
  std::sort(labels_.begin(), labels_.end());
  labels_.erase(std::unique(labels_.begin(), labels_.end()), labels_.end());
  labels_.erase(labels_.begin(), std::lower_bound(labels_.begin(), labels_.end(), 0));
  enc_ids_.clear();
  enc_bits_.clear();
  enc_dtx_.clear();
  for (const int32_t room : labels_) {
    if (!RoomExists(room)) {   // (SetRoom refuses these: a label that reached the base class's SetRoom directly)
      LOG(ERROR) << "Room " << room << " does not exist: the bridge has " << max_rooms() << " rooms.";
      return -1;
    }
    for (int c = 0; c <= max_speakers_; ++c) {
      enc_ids_.push_back(n + room * (1 + max_speakers_) + c);
      enc_bits_.push_back(room_bits_[room]);
      enc_dtx_.push_back(room_dtx_[room]);
    }
  }
  return lyra_hip_shared_begin(ctx, ids, n, packets, packet_bytes, rooms, muted, flags ? LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE : 0u,
                               max_speakers_, labels_.data(), static_cast<int>(labels_.size()), enc_ids_.data(), enc_bits_.data(),
                               enc_dtx_.data());
}

int LyraSharedBridge::EndTick(lyra_hip_ctx* ctx, uint8_t* rows, int32_t* lengths, int32_t* is_noise, int32_t* is_comfort_noise) {
  return lyra_hip_shared_end(ctx, rows, lengths, is_noise, is_comfort_noise, levels_.data(), speaker_.data(), slot_.data());
}

void LyraSharedBridge::ForgetStream(int stream) {
  levels_[stream] = 0;
  speaker_[stream] = 0;
  slot_[stream] = -1;
}

}  // namespace codec
}  // namespace chromemedia
