// lyra_speaker_bridge.cc -- see lyra_speaker_bridge.h.  Plain C++17 over the C ABI (include/lyra_hip_speakers.h); no HIP here.
// A translation unit of its own: lyra_conference_bridge.cc stays built against the calls it was built against.
#include "lyra_speaker_bridge.h"

#include "../../include/lyra_hip_speakers.h"
#include "glog/logging.h"

namespace chromemedia {
namespace codec {

static_assert(kBridgeMaxSpeakers == LYRA_HIP_SPEAKERS_MAX, "the selection's bound");

LyraSpeakerBridge::LyraSpeakerBridge(lyra_hip_ctx* ctx, absl::Span<const BridgeStream> streams, bool skip_comfort_noise,
                                     int max_speakers)
    : LyraConferenceBridge(ctx, streams, skip_comfort_noise),
      max_speakers_(max_speakers),
      levels_(streams.size(), 0),
      speaker_(streams.size(), 0) {}

std::unique_ptr<LyraSpeakerBridge> LyraSpeakerBridge::Create(absl::Span<const BridgeStream> streams,
                                                            const ghc::filesystem::path& model_path, int device,
                                                            bool skip_comfort_noise, int max_speakers) {
  if (max_speakers < 1 || max_speakers > kBridgeMaxSpeakers) {
    LOG(ERROR) << "max_speakers must lie in 1.." << kBridgeMaxSpeakers << ", but is " << max_speakers << ".";
    return nullptr;
  }
  lyra_hip_ctx* ctx = NewBridgeContext(streams, model_path, device);
  if (ctx == nullptr) return nullptr;
  return std::unique_ptr<LyraSpeakerBridge>(new LyraSpeakerBridge(ctx, streams, skip_comfort_noise, max_speakers));
}

int LyraSpeakerBridge::BeginTick(lyra_hip_ctx* ctx, const int32_t* ids, int n, const uint8_t* packets,
                                 const int32_t* packet_bytes, const int32_t* rooms, const int32_t* muted, unsigned flags,
                                 const int32_t* bits, const int32_t* dtx) {
  // (the base class's flag bit is the selection's: both are "skip comfort noise", bit 0)
  return lyra_hip_speakers_begin(ctx, ids, n, packets, packet_bytes, rooms, muted,
                                 flags ? LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE : 0u, bits, dtx, max_speakers_);
}

int LyraSpeakerBridge::EndTick(lyra_hip_ctx* ctx, uint8_t* rows, int32_t* lengths, int32_t* is_noise, int32_t* is_comfort_noise) {
  return lyra_hip_speakers_end(ctx, rows, lengths, is_noise, is_comfort_noise, levels_.data(), speaker_.data());
}

void LyraSpeakerBridge::ForgetStream(int stream) {
  levels_[stream] = 0;
  speaker_[stream] = 0;
}

}  // namespace codec
}  // namespace chromemedia
