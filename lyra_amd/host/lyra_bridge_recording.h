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

// The first tick of every call BridgeMeetingTimeParallel makes, in order: tick 0, and every tick in front of which the entries
// of the schedule so far (one per present stream and stretch of constant membership and presence; the C ABI's
// LYRA_HIP_MEETING_MAX_ENTRIES) would exceed max_entries.  present: [ticks][num_streams], or null: everyone always.  Empty for
// ticks == 0.  Host only.
inline std::vector<int64_t> BridgeMeetingCallStarts(const int32_t* script, const int32_t* present, int64_t ticks, int num_streams,
                                                    int64_t max_entries) {
  std::vector<int64_t> starts;
  const size_t n = static_cast<size_t>(num_streams);
  auto where = [&](int64_t t, size_t s) -> int64_t {   // -2: absent, -1: in no room, else the room
    const size_t at = static_cast<size_t>(t) * n + s;
    if (present != nullptr && present[at] == 0) return -2;
    return script[at * kBridgeScriptFields] < 0 ? -1 : script[at * kBridgeScriptFields];
  };
  int64_t entries = 0;
  for (int64_t t = 0; t < ticks; ++t) {
    bool change = t == 0;
    int64_t here = 0;
    for (size_t s = 0; s < n; ++s) {
      change = change || where(t, s) != where(t - 1, s);
      here += where(t, s) != -2;
    }
    if (!change) continue;
    if (t == 0 || entries + here > max_entries) {
      starts.push_back(t);
      entries = 0;
    }
    entries += here;
  }
  return starts;
}

// The same recording with a SCHEDULE (include/lyra_hip_spans_meeting.h): present [ticks][num_streams] says on which ticks a
// stream takes part (empty: everyone always); on the others it is no row of the tick -- nothing is decoded or encoded for it,
// its state does not advance, and its outgoing row is zeros with length 0.  Rooms may change from tick to tick as before.
// Spans and stays are derived from the script's room column and `present`, every stream's packets, lengths, mutes and
// bitrates are compacted to its present ticks, and the whole meeting is ONE device call (more only where the schedule has more
// than LYRA_HIP_MEETING_MAX_ENTRIES entries: BridgeMeetingCallStarts).  Byte for byte what the tick bridges give when absent
// streams are left out of a tick's rows.  nullopt as BridgeRecordingTimeParallel, and for a `present` of another size.
std::optional<std::pair<std::vector<uint8_t>, std::vector<int32_t>>> BridgeMeetingTimeParallel(
    absl::Span<const BridgeStream> streams, const ghc::filesystem::path& model_path, absl::Span<const uint8_t> packets,
    absl::Span<const int32_t> lengths, absl::Span<const int32_t> script, absl::Span<const int32_t> present,
    bool skip_comfort_noise, int max_speakers, int num_lanes, int device = 0, std::vector<int32_t>* is_speaker = nullptr);

}  // namespace codec
}  // namespace chromemedia
#endif
