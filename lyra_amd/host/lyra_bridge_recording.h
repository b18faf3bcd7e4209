// lyra_bridge_recording.h -- BridgeRecordingTimeParallel: a RECORDED meeting through the conference bridge in a few device
// calls instead of one per 20 ms tick (include/lyra_hip_bridge_spans.h).  What LyraConferenceBridge / LyraSpeakerBridge give
// tick by tick for the same streams, packets and script, byte for byte: the script is cut where any participant's room
// changes, and every segment is one time-parallel call that continues the streams of the one before.
// LyraConferenceBridge's conventions: nullopt + LOG(ERROR), no exceptions.
#ifndef LYRA_AMD_HOST_LYRA_BRIDGE_RECORDING_H_
#define LYRA_AMD_HOST_LYRA_BRIDGE_RECORDING_H_
#include <cstddef>
#include <cstdint>
#include <optional>
#include <utility>
#include <vector>

#include "absl/types/span.h"
#include "include/ghc/filesystem.hpp"
#include "lyra_conference_bridge.h"

namespace chromemedia {
namespace codec {

constexpr int kBridgeScriptFields = 3;   // per tick and stream: room (< 0: none), muted, bitrate -- what bridge_demo reads

// The first tick of every segment of a script [ticks][num_streams][3], in order: tick 0, and every tick at which some stream's
// room differs from the tick before (two negative labels are the same "no room").  Empty for ticks == 0.  Host only.
inline std::vector<int64_t> BridgeRecordingSegmentStarts(const int32_t* script, int64_t ticks, int num_streams) {
  std::vector<int64_t> starts;
  const size_t n = static_cast<size_t>(num_streams);
  for (int64_t t = 0; t < ticks; ++t) {
    bool cut = t == 0;
    for (size_t s = 0; s < n && !cut; ++s) {
      const int32_t before = script[(static_cast<size_t>(t - 1) * n + s) * kBridgeScriptFields];
      const int32_t now = script[(static_cast<size_t>(t) * n + s) * kBridgeScriptFields];
      cut = (before < 0 ? -1 : before) != (now < 0 ? -1 : now);
    }
    if (cut) starts.push_back(t);
  }
  return starts;
}

// packets [ticks][num_streams][23] and lengths [ticks][num_streams] (0: no packet from that stream on that tick; else 8 / 15 /
// 23) come in, script [ticks][num_streams][3] holds room, muted and outgoing bitrate of every stream as of every tick.
// max_speakers 0: the full mix of LyraConferenceBridge; 1 .. 8: the loudest-N selection of LyraSpeakerBridge.  num_lanes:
// stream slots beyond the participants' that the calls may use as scratch (more lanes, fewer steps; 0 runs a segment hop by
// hop on the participants' own streams).  Returns the outgoing rows [ticks][num_streams][23], zero behind each packet's bytes,
// and lengths [ticks][num_streams]; is_speaker, where given, receives [ticks][num_streams] flags (all zero for max_speakers 0).
// nullopt for no streams, an unsupported bitrate or packet size, spans that disagree about ticks and streams, max_speakers
// outside 0 .. 8, a negative lane count, or a device failure.
std::optional<std::pair<std::vector<uint8_t>, std::vector<int32_t>>> BridgeRecordingTimeParallel(
    absl::Span<const BridgeStream> streams, const ghc::filesystem::path& model_path, absl::Span<const uint8_t> packets,
    absl::Span<const int32_t> lengths, absl::Span<const int32_t> script, bool skip_comfort_noise, int max_speakers,
    int num_lanes, int device = 0, std::vector<int32_t>* is_speaker = nullptr);

}  // namespace codec
}  // namespace chromemedia
#endif
