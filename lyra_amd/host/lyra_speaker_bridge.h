// lyra_speaker_bridge.h -- LyraSpeakerBridge: LyraConferenceBridge (lyra_conference_bridge.h) with loudest-N selection, as
// production media servers mix: every participant hears the max_speakers loudest sources of its room (itself left out), and
// the server learns who is speaking.  The host logic -- staging, settings, the two-deep pipeline, the failed-call latch -- is
// the base class's; this class swaps the two device calls of a tick for those of include/lyra_hip_speakers.h and keeps the
// levels and speaker flags they deliver.  The selection is stateless: no smoothing across ticks.
#ifndef LYRA_AMD_HOST_LYRA_SPEAKER_BRIDGE_H_
#define LYRA_AMD_HOST_LYRA_SPEAKER_BRIDGE_H_
#include <cstdint>
#include <memory>
#include <vector>

#include "lyra_conference_bridge.h"

namespace chromemedia {
namespace codec {

constexpr int kBridgeMaxSpeakers = 8;   // LYRA_HIP_SPEAKERS_MAX

class LyraSpeakerBridge : public LyraConferenceBridge {
 public:
  // As LyraConferenceBridge::Create; nullptr as well if max_speakers lies outside [1, kBridgeMaxSpeakers].
  static std::unique_ptr<LyraSpeakerBridge> Create(absl::Span<const BridgeStream> streams,
                                                   const ghc::filesystem::path& model_path, int device = 0,
                                                   bool skip_comfort_noise = false, int max_speakers = 3);
  // As of the last tick DELIVERED: whether the participant was among its room's speakers, and the level of what it said (the
  // sum of squares of its 16 kHz hop, 320 samples).  false / 0 for a stream that does not exist or was reset since.
  bool is_speaker(int stream) const { return Exists(stream) && speaker_[stream] != 0; }
  int64_t level(int stream) const { return Exists(stream) ? levels_[stream] : 0; }
  int max_speakers() const { return max_speakers_; }

 protected:
  int BeginTick(lyra_hip_ctx* ctx, const int32_t* ids, int n, const uint8_t* packets, const int32_t* packet_bytes,
                const int32_t* rooms, const int32_t* muted, unsigned flags, const int32_t* bits, const int32_t* dtx) override;
  int EndTick(lyra_hip_ctx* ctx, uint8_t* rows, int32_t* lengths, int32_t* is_noise, int32_t* is_comfort_noise) override;
  void ForgetStream(int stream) override;

 private:
  LyraSpeakerBridge(lyra_hip_ctx* ctx, absl::Span<const BridgeStream> streams, bool skip_comfort_noise, int max_speakers);
  int max_speakers_;
  std::vector<int64_t> levels_;    // of the last tick delivered
  std::vector<int32_t> speaker_;
};

}  // namespace codec
}  // namespace chromemedia
#endif
