// lyra_bridge_recording.cc -- see lyra_bridge_recording.h.  Plain C++17 over the C ABI (include/lyra_hip_bridge_spans.h); no HIP
// here.  A translation unit of its own, like the other bridge classes.
#include "lyra_bridge_recording.h"

#include <algorithm>
#include <cstring>

#include "../../include/lyra_hip_bridge_spans.h"
#include "../../include/lyra_hip_spans_meeting.h"
#include "glog/logging.h"
#include "host_common.h"

namespace chromemedia {
namespace codec {
using namespace host;

namespace {
int RecordingBitrateToBits(int bitrate) { return bitrate == 3200 ? 64 : bitrate == 6000 ? 120 : bitrate == 9200 ? 184 : -1; }
}  // namespace

std::optional<std::pair<std::vector<uint8_t>, std::vector<int32_t>>> BridgeRecordingTimeParallel(
    absl::Span<const BridgeStream> streams, const ghc::filesystem::path& model_path, absl::Span<const uint8_t> packets,
    absl::Span<const int32_t> lengths, absl::Span<const int32_t> script, bool skip_comfort_noise, int max_speakers,
    int num_lanes, int device, std::vector<int32_t>* is_speaker) {
  constexpr size_t kRow = kBridgePacketRowBytes;
  const size_t n = streams.size();
  if (n == 0) {
    LOG(ERROR) << "num_streams must be positive.";
    return std::nullopt;
  }
  if (max_speakers < 0 || max_speakers > LYRA_HIP_SPEAKERS_MAX || num_lanes < 0) {
    LOG(ERROR) << "max_speakers " << max_speakers << " (0 .. " << LYRA_HIP_SPEAKERS_MAX << ") or num_lanes " << num_lanes
               << " is out of range.";
    return std::nullopt;
  }
  const size_t ticks = lengths.size() / n;
  if (lengths.size() != ticks * n || packets.size() != ticks * n * kRow || script.size() != ticks * n * kBridgeScriptFields) {
    LOG(ERROR) << "The packets (" << packets.size() << " bytes), lengths (" << lengths.size() << ") and script ("
               << script.size() << " words) disagree about ticks and streams (" << n << ").";
    return std::nullopt;
  }
  for (const BridgeStream& s : streams)
    if (RecordingBitrateToBits(s.bitrate) < 0) {
      LOG(ERROR) << "Bitrate " << s.bitrate << " bps is not supported by codec.";
      return std::nullopt;
    }
  for (size_t i = 0; i < ticks * n; ++i) {
    if (lengths[i] != 0 && PacketSizeToBits(lengths[i]) < 0) {
      LOG(ERROR) << "The packet size (" << lengths[i] << " bytes, tick " << i / n << ", stream " << i % n << ") is not supported.";
      return std::nullopt;
    }
    if (RecordingBitrateToBits(script[i * kBridgeScriptFields + 2]) < 0) {
      LOG(ERROR) << "Bitrate " << script[i * kBridgeScriptFields + 2] << " bps (tick " << i / n << ", stream " << i % n
                 << ") is not supported by codec.";
      return std::nullopt;
    }
  }
  std::pair<std::vector<uint8_t>, std::vector<int32_t>> out;
  out.first.assign(ticks * n * kRow, 0);
  out.second.assign(ticks * n, 0);
  if (is_speaker) is_speaker->assign(ticks * n, 0);
  if (ticks == 0) return out;
  lyra_hip_ctx* ctx = NewContext(model_path, device, static_cast<int>(n) + num_lanes);
  if (ctx == nullptr) {
    LOG(ERROR) << "Could not create the recording's context.";
    return std::nullopt;
  }
  std::vector<int32_t> lanes(static_cast<size_t>(num_lanes)), dtx(n), rooms(n);
  for (int l = 0; l < num_lanes; ++l) lanes[static_cast<size_t>(l)] = static_cast<int32_t>(n) + l;
  for (size_t s = 0; s < n; ++s) dtx[s] = streams[s].enable_dtx ? 1 : 0;
  std::vector<int64_t> starts = BridgeRecordingSegmentStarts(script.data(), static_cast<int64_t>(ticks), static_cast<int>(n));
  starts.push_back(static_cast<int64_t>(ticks));
  // per segment: participant s owns frames s * len .. (s + 1) * len - 1 of the frame-major buffers
  std::vector<lyra_hip_span> spans(n);
  std::vector<uint8_t> in_rows, out_rows;
  std::vector<int32_t> in_len, muted, bits, out_len, spk;
  bool ok = true;
  for (size_t g = 0; ok && g + 1 < starts.size(); ++g) {
    const size_t t0 = static_cast<size_t>(starts[g]), len = static_cast<size_t>(starts[g + 1]) - t0, frames = n * len;
    in_rows.assign(frames * kRow, 0);
    out_rows.assign(frames * kRow, 0);
    in_len.assign(frames, 0);
    muted.assign(frames, 0);
    bits.assign(frames, 0);
    out_len.assign(frames, 0);
    spk.assign(frames, 0);
    for (size_t s = 0; s < n; ++s) {
      spans[s] = lyra_hip_span{static_cast<int32_t>(s), static_cast<int64_t>(s * len), static_cast<int64_t>(len)};
      rooms[s] = script[(t0 * n + s) * kBridgeScriptFields];
      for (size_t t = 0; t < len; ++t) {
        const size_t at = (t0 + t) * n + s, f = s * len + t;
        std::memcpy(&in_rows[f * kRow], &packets[at * kRow], static_cast<size_t>(lengths[at]));
        in_len[f] = lengths[at];
        muted[f] = script[at * kBridgeScriptFields + 1] != 0;
        bits[f] = RecordingBitrateToBits(script[at * kBridgeScriptFields + 2]);
      }
    }
    if (lyra_hip_spans_bridge(ctx, spans.data(), static_cast<int>(n), lanes.data(), num_lanes, rooms.data(), in_rows.data(),
                              in_len.data(), muted.data(), skip_comfort_noise ? LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE : 0u,
                              bits.data(), dtx.data(), max_speakers, out_rows.data(), out_len.data(), nullptr, nullptr, nullptr,
                              nullptr, nullptr, max_speakers ? spk.data() : nullptr) != 0) {
      LOG(ERROR) << "Unable to run ticks " << t0 << " .. " << t0 + len - 1 << ": " << lyra_hip_last_error(ctx);
      ok = false;
      break;
    }
    for (size_t s = 0; s < n; ++s)
      for (size_t t = 0; t < len; ++t) {
        const size_t at = (t0 + t) * n + s, f = s * len + t;
        std::memcpy(&out.first[at * kRow], &out_rows[f * kRow], kRow);
        out.second[at] = out_len[f];
        if (is_speaker) (*is_speaker)[at] = spk[f];
      }
  }
  lyra_hip_destroy(ctx);
  if (!ok) return std::nullopt;
  return out;
}

std::optional<std::pair<std::vector<uint8_t>, std::vector<int32_t>>> BridgeMeetingTimeParallel(
    absl::Span<const BridgeStream> streams, const ghc::filesystem::path& model_path, absl::Span<const uint8_t> packets,
    absl::Span<const int32_t> lengths, absl::Span<const int32_t> script, absl::Span<const int32_t> present,
    bool skip_comfort_noise, int max_speakers, int num_lanes, int device, std::vector<int32_t>* is_speaker) {
  constexpr size_t kRow = kBridgePacketRowBytes;
  const size_t n = streams.size();
  if (n == 0) {
    LOG(ERROR) << "num_streams must be positive.";
    return std::nullopt;
  }
  if (max_speakers < 0 || max_speakers > LYRA_HIP_SPEAKERS_MAX || num_lanes < 0) {
    LOG(ERROR) << "max_speakers " << max_speakers << " (0 .. " << LYRA_HIP_SPEAKERS_MAX << ") or num_lanes " << num_lanes
               << " is out of range.";
    return std::nullopt;
  }
  const size_t ticks = lengths.size() / n;
  if (lengths.size() != ticks * n || packets.size() != ticks * n * kRow || script.size() != ticks * n * kBridgeScriptFields ||
      (!present.empty() && present.size() != ticks * n)) {
    LOG(ERROR) << "The packets (" << packets.size() << " bytes), lengths (" << lengths.size() << "), script (" << script.size()
               << " words) and presence (" << present.size() << ") disagree about ticks and streams (" << n << ").";
    return std::nullopt;
  }
  auto here = [&](size_t t, size_t s) { return present.empty() || present[t * n + s] != 0; };
  for (const BridgeStream& s : streams)
    if (RecordingBitrateToBits(s.bitrate) < 0) {
      LOG(ERROR) << "Bitrate " << s.bitrate << " bps is not supported by codec.";
      return std::nullopt;
    }
  for (size_t i = 0; i < ticks * n; ++i) {
    if (!here(i / n, i % n)) continue;   // what an absent stream's rows hold is not read
    if (lengths[i] != 0 && PacketSizeToBits(lengths[i]) < 0) {
      LOG(ERROR) << "The packet size (" << lengths[i] << " bytes, tick " << i / n << ", stream " << i % n << ") is not supported.";
      return std::nullopt;
    }
    if (RecordingBitrateToBits(script[i * kBridgeScriptFields + 2]) < 0) {
      LOG(ERROR) << "Bitrate " << script[i * kBridgeScriptFields + 2] << " bps (tick " << i / n << ", stream " << i % n
                 << ") is not supported by codec.";
      return std::nullopt;
    }
  }
  std::pair<std::vector<uint8_t>, std::vector<int32_t>> out;
  out.first.assign(ticks * n * kRow, 0);
  out.second.assign(ticks * n, 0);
  if (is_speaker) is_speaker->assign(ticks * n, 0);
  if (ticks == 0) return out;
  lyra_hip_ctx* ctx = NewContext(model_path, device, static_cast<int>(n) + num_lanes);
  if (ctx == nullptr) {
    LOG(ERROR) << "Could not create the meeting's context.";
    return std::nullopt;
  }
  std::vector<int32_t> lanes(static_cast<size_t>(num_lanes)), dtx(n);
  for (int l = 0; l < num_lanes; ++l) lanes[static_cast<size_t>(l)] = static_cast<int32_t>(n) + l;
  for (size_t s = 0; s < n; ++s) dtx[s] = streams[s].enable_dtx ? 1 : 0;
  std::vector<int64_t> starts = BridgeMeetingCallStarts(script.data(), present.empty() ? nullptr : present.data(),
                                                        static_cast<int64_t>(ticks), static_cast<int>(n), LYRA_HIP_MEETING_MAX_ENTRIES);
  starts.push_back(static_cast<int64_t>(ticks));
  std::vector<lyra_hip_span> spans(n);
  std::vector<lyra_hip_meeting_stay> stays;
  std::vector<size_t> where;   // by frame: tick * n + stream
  std::vector<uint8_t> in_rows, out_rows;
  std::vector<int32_t> in_len, muted, bits, out_len, spk;
  bool ok = true;
  for (size_t g = 0; ok && g + 1 < starts.size(); ++g) {
    const size_t t0 = static_cast<size_t>(starts[g]), t1 = static_cast<size_t>(starts[g + 1]);
    // stream s owns the frames of its present ticks, stream after stream; a stay is a run of present ticks in one room
    stays.clear();
    where.clear();
    for (size_t s = 0; s < n; ++s) {
      const size_t first = where.size();
      for (size_t t = t0; t < t1; ++t) {
        if (!here(t, s)) continue;
        const int32_t room = script[(t * n + s) * kBridgeScriptFields] < 0 ? -1 : script[(t * n + s) * kBridgeScriptFields];
        if (!stays.empty() && stays.back().participant == static_cast<int32_t>(s) && stays.back().room == room &&
            stays.back().first_tick + stays.back().n_ticks == static_cast<int64_t>(t - t0))
          ++stays.back().n_ticks;
        else
          stays.push_back(lyra_hip_meeting_stay{static_cast<int32_t>(s), room, static_cast<int64_t>(t - t0), 1});
        where.push_back(t * n + s);
      }
      spans[s] = lyra_hip_span{static_cast<int32_t>(s), static_cast<int64_t>(first), static_cast<int64_t>(where.size() - first)};
    }
    const size_t frames = where.size();
    if (frames == 0) continue;   // nobody is present on these ticks
    in_rows.assign(frames * kRow, 0);
    out_rows.assign(frames * kRow, 0);
    in_len.assign(frames, 0);
    muted.assign(frames, 0);
    bits.assign(frames, 0);
    out_len.assign(frames, 0);
    spk.assign(frames, 0);
    for (size_t f = 0; f < frames; ++f) {
      const size_t at = where[f];
      std::memcpy(&in_rows[f * kRow], &packets[at * kRow], static_cast<size_t>(lengths[at]));
      in_len[f] = lengths[at];
      muted[f] = script[at * kBridgeScriptFields + 1] != 0;
      bits[f] = RecordingBitrateToBits(script[at * kBridgeScriptFields + 2]);
    }
    if (lyra_hip_spans_meeting(ctx, spans.data(), static_cast<int>(n), lanes.data(), num_lanes, stays.data(),
                               static_cast<int>(stays.size()), in_rows.data(), in_len.data(), muted.data(),
                               skip_comfort_noise ? LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE : 0u, bits.data(), dtx.data(), max_speakers,
                               out_rows.data(), out_len.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                               max_speakers ? spk.data() : nullptr) != 0) {
      LOG(ERROR) << "Unable to run ticks " << t0 << " .. " << t1 - 1 << ": " << lyra_hip_last_error(ctx);
      ok = false;
      break;
    }
    for (size_t f = 0; f < frames; ++f) {
      const size_t at = where[f];
      std::memcpy(&out.first[at * kRow], &out_rows[f * kRow], kRow);
      out.second[at] = out_len[f];
      if (is_speaker) (*is_speaker)[at] = spk[f];
    }
  }
  lyra_hip_destroy(ctx);
  if (!ok) return std::nullopt;
  return out;
}

}  // namespace codec
}  // namespace chromemedia
