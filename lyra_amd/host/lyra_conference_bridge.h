// lyra_conference_bridge.h -- LyraConferenceBridge: what a media server does between its LyraDecoders and its LyraEncoders, for
// many participants in one GPU context.  Per 20 ms tick every participant delivers at most one packet, every participant hears
// the sum of the other sources of its room (mix-minus), and that mix is encoded for it at its own bitrate, with or without
// DTX.  One device call per tick for the whole batch (include/lyra_hip_bridge.h): decoded audio never leaves the device.
// MixedBatchLyraDecoder's conventions: nullptr / nullopt / false + LOG(ERROR), no exceptions.
//
// The bridge runs at 16 kHz, the codec's internal rate: packets carry no sample rate, endpoints resample.  Participant s is
// stream slot s of the context; a stream is a decoder (what it says) and an encoder (what it hears) at once.
#ifndef LYRA_AMD_HOST_LYRA_CONFERENCE_BRIDGE_H_
#define LYRA_AMD_HOST_LYRA_CONFERENCE_BRIDGE_H_
#include <cstdint>
#include <memory>
#include <optional>
#include <utility>
#include <vector>

#include "absl/types/span.h"
#include "include/ghc/filesystem.hpp"

struct lyra_hip_ctx;

namespace chromemedia {
namespace codec {

constexpr int kBridgePacketRowBytes = 23;   // LYRA_HIP_MAX_PACKET_BYTES

// What LyraEncoder::Create takes per outgoing stream (lyra_encoder.h: bitrate, enable_dtx); the rate is the bridge's 16 kHz.
struct BridgeStream {
  int bitrate;        // 3200, 6000 or 9200
  bool enable_dtx;
};

class LyraConferenceBridge {
 public:
  // nullptr if `streams` is empty or a bitrate is unsupported.  skip_comfort_noise: a participant whose decoder plays comfort
  // noise (its packets stopped coming) is no source of its room's mix.  Every stream starts in no room, unmuted.
  static std::unique_ptr<LyraConferenceBridge> Create(absl::Span<const BridgeStream> streams,
                                                      const ghc::filesystem::path& model_path, int device = 0,
                                                      bool skip_comfort_noise = false);
  virtual ~LyraConferenceBridge();
  // Membership, mute and the outgoing bitrate (LyraEncoder::set_bitrate) of one stream, from the NEXT tick begun; ticks in
  // flight keep what they were begun with.  room < 0: in no room (hears silence, is heard by nobody).  false for a stream
  // that does not exist, an unsupported bitrate, or a room that would exceed 32767 members.
  bool SetRoom(int stream, int room);
  bool SetMuted(int stream, bool muted);
  bool set_bitrate(int stream, int bitrate);
  // A newcomer takes the slot: decoder and encoder state of `stream` start afresh (drains the device; ticks in flight stay
  // deliverable), a packet staged for it is dropped, its flags read false.  Room, mute and bitrate stay as set.
  bool ResetStream(int stream);
  // Stages incoming packets for the NEXT tick begun, as MixedBatchLyraDecoder does: `rows` holds num_streams rows of 23 bytes,
  // lengths[s] bytes of row s are stream s's packet, 0: none.  A length other than 0 / 8 / 15 / 23 or a packet for a stream
  // that already has one staged refuses the WHOLE call: nothing is staged.
  bool SetEncodedPackets(absl::Span<const uint8_t> rows, absl::Span<const int32_t> lengths);
  bool SetEncodedPacket(int stream, absl::Span<const uint8_t> packet);
  // One tick: (rows [num_streams][23], zero behind each packet's bytes; lengths [num_streams], 0: the empty DTX packet).
  // Refused while TickAsync() ticks are in flight.
  std::optional<std::pair<std::vector<uint8_t>, std::vector<int32_t>>> Tick();
  // The same in two halves: TickAsync() consumes the staged packets, starts a tick and returns; WaitTick() delivers the OLDEST
  // tick started.  Up to two in flight.  A WaitTick() refused for a size consumes nothing.
  bool TickAsync();
  bool WaitTick(absl::Span<uint8_t> rows, absl::Span<int32_t> lengths);
  // As of the last tick DELIVERED: LyraDecoder::is_comfort_noise and the decoder-side estimator's is_noise() of the
  // participant's incoming stream.  false for a stream that does not exist.
  bool is_comfort_noise(int stream) const;
  bool is_noise(int stream) const;
  int room(int stream) const { return Exists(stream) ? rooms_[stream] : -1; }
  bool muted(int stream) const { return Exists(stream) && muted_[stream] != 0; }
  int bitrate(int stream) const { return Exists(stream) ? bits_[stream] * 50 : 0; }
  int sample_rate_hz() const { return 16000; }
  int num_streams() const { return static_cast<int>(ids_.size()); }
  int ticks_in_flight() const { return in_flight_; }

 protected:
  // For a bridge with another mix (lyra_speaker_bridge.h): the host logic above is this class's, and the device calls of a
  // tick go through the three hooks below.  NewBridgeContext is what Create checks and creates: nullptr + LOG(ERROR) if
  // `streams` is empty or a bitrate is unsupported.  extra_streams: stream slots behind the participants', for a subclass that
  // runs encoders of its own (lyra_shared_bridge.h).
  LyraConferenceBridge(lyra_hip_ctx* ctx, absl::Span<const BridgeStream> streams, bool skip_comfort_noise);
  static lyra_hip_ctx* NewBridgeContext(absl::Span<const BridgeStream> streams, const ghc::filesystem::path& model_path,
                                        int device, int extra_streams = 0);
  // begin() and end() of the C ABI's two-deep host form: 0 on success; the arrays hold num_streams entries.
  virtual int BeginTick(lyra_hip_ctx* ctx, const int32_t* ids, int n, const uint8_t* packets, const int32_t* packet_bytes,
                        const int32_t* rooms, const int32_t* muted, unsigned flags, const int32_t* bits, const int32_t* dtx);
  virtual int EndTick(lyra_hip_ctx* ctx, uint8_t* rows, int32_t* lengths, int32_t* is_noise, int32_t* is_comfort_noise);
  virtual void ForgetStream(int stream) { (void)stream; }   // ResetStream: what a subclass holds per stream reads false again
  bool Exists(int stream) const { return stream >= 0 && stream < num_streams(); }

 private:
  lyra_hip_ctx* ctx_;
  unsigned flags_;
  std::vector<int32_t> ids_;            // stream slots 0 .. num_streams - 1 of the context
  std::vector<int32_t> rooms_, muted_, bits_, dtx_;
  std::vector<uint8_t> staged_;         // [num_streams][23] packets for the next tick begun
  std::vector<int32_t> staged_bytes_;   // [num_streams] 0 = none
  std::vector<int32_t> noise_, cn_;     // flags of the last tick delivered
  int in_flight_ = 0;
  bool failed_ = false;                 // a device call failed: every further call is refused
};

}  // namespace codec
}  // namespace chromemedia
#endif
