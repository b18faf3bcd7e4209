// lyra_shared_bridge.h -- LyraSharedBridge: the loudest-N bridge (lyra_speaker_bridge.h) with SHARED ENCODERS, for large rooms.
// A room with max_speakers = N has 1 + N distinct mixes -- what every non-speaker hears, and one mix-minus per speaker -- so
// the bridge runs 1 + N encoders per room instead of one per participant and sends the same packet to everyone who hears the
// same mix (include/lyra_hip_shared_bridge.h).  The host logic -- staging, rooms, mutes, the two-deep pipeline, the failed-call
// latch -- is LyraConferenceBridge's; this class swaps the two device calls of a tick and keeps what they deliver.
//
// What changes for the caller: bitrate and DTX belong to a ROOM (SetRoomBitrate / SetRoomDtx), not to a listener -- the
// BridgeStream settings and set_bitrate() of the base class are ignored -- and room labels lie in [0, max_rooms).  Participant s
// is stream slot s of the context; room r's encoders are the slots num_streams + r * (1 + N) + 0 .. N behind them.
#ifndef LYRA_AMD_HOST_LYRA_SHARED_BRIDGE_H_
#define LYRA_AMD_HOST_LYRA_SHARED_BRIDGE_H_
#include <cstdint>
#include <memory>
#include <vector>

#include "lyra_conference_bridge.h"

namespace chromemedia {
namespace codec {

constexpr int kSharedBridgeMaxSpeakers = 8;   // LYRA_HIP_SPEAKERS_MAX

class LyraSharedBridge : public LyraConferenceBridge {
 public:
  // As LyraConferenceBridge::Create; nullptr as well if max_speakers lies outside [1, 8], max_rooms < 1, or the room default is
  // no bitrate of the codec.  Every room starts with `room_default`.  A tick needs (rooms in use) * (1 + max_speakers) <=
  // num_streams + max_rooms * (1 + max_speakers), the size of the context: true whenever the rooms are not mostly tiny.
  static std::unique_ptr<LyraSharedBridge> Create(absl::Span<const BridgeStream> streams, const ghc::filesystem::path& model_path,
                                                  int device = 0, bool skip_comfort_noise = false, int max_speakers = 3,
                                                  int max_rooms = 1, BridgeStream room_default = {6000, false});
  // false for a room >= max_rooms (or a stream that does not exist ...: as the base class)
  bool SetRoom(int stream, int room);
  // The outgoing bitrate / DTX switch of all 1 + max_speakers encoders of a room, from the NEXT tick begun.
  bool SetRoomBitrate(int room, int bitrate);
  bool SetRoomDtx(int room, bool enable_dtx);
  // The room's encoders start afresh and its speaker slots are free (drains the device; ticks in flight stay deliverable).
  bool ResetRoom(int room);
  // As of the last tick DELIVERED: the speaker slot the participant held (-1: none: it heard the room's common packet), whether
  // it was among its room's speakers, and the level of what it said.
  int slot(int stream) const { return Exists(stream) ? slot_[stream] : -1; }
  bool is_speaker(int stream) const { return Exists(stream) && speaker_[stream] != 0; }
  int64_t level(int stream) const { return Exists(stream) ? levels_[stream] : 0; }
  int room_bitrate(int room) const { return RoomExists(room) ? room_bits_[room] * 50 : 0; }
  bool room_dtx(int room) const { return RoomExists(room) && room_dtx_[room] != 0; }
  int max_speakers() const { return max_speakers_; }
  int max_rooms() const { return static_cast<int>(room_bits_.size()); }

 protected:
  int BeginTick(lyra_hip_ctx* ctx, const int32_t* ids, int n, const uint8_t* packets, const int32_t* packet_bytes,
                const int32_t* rooms, const int32_t* muted, unsigned flags, const int32_t* bits, const int32_t* dtx) override;
  int EndTick(lyra_hip_ctx* ctx, uint8_t* rows, int32_t* lengths, int32_t* is_noise, int32_t* is_comfort_noise) override;
  void ForgetStream(int stream) override;

 private:
  LyraSharedBridge(lyra_hip_ctx* ctx, absl::Span<const BridgeStream> streams, bool skip_comfort_noise, int max_speakers,
                   int max_rooms, int default_bits, bool default_dtx);
  bool RoomExists(int room) const { return room >= 0 && room < max_rooms(); }
  lyra_hip_ctx* ctx_;                    // the base class's, which owns it
  int max_speakers_;
  std::vector<int32_t> room_bits_, room_dtx_;   // [max_rooms]
  std::vector<int64_t> levels_;                 // of the last tick delivered
  std::vector<int32_t> speaker_, slot_;
  std::vector<int32_t> labels_, enc_ids_, enc_bits_, enc_dtx_;   // scratch of BeginTick
};

}  // namespace codec
}  // namespace chromemedia
#endif
