// bridge_demo.cc -- drives LyraConferenceBridge (lyra_conference_bridge.h) through a scripted call:
//   bridge_demo <model_dir> <streams.txt> <script.i32> <packets_in.bin> <lengths_in.i32> <packets_out.bin> <lengths_out.i32>
//               <mode> <skip_comfort_noise> [--max-speakers=N --speakers-out=<speakers_out.i32>
//               [--shared-encoders [--slots-out=<slots_out.i32>]]]
// streams.txt: one line "bitrate enable_dtx" per stream.  script: [ticks][num_streams][3] int32 -- room (< 0: none), muted,
// bitrate of every stream as of that tick, applied before the tick is begun.  packets_in: [ticks][num_streams][23] bytes;
// lengths_in: [ticks][num_streams] int32, 0 = no packet from that stream on that tick.  Writes every tick's outgoing packets
// [num_streams][23] and lengths [num_streams] int32.
// mode 0: Tick() per tick.  mode 1: the same call through TickAsync / WaitTick, two ticks deep (tick t + 1 is begun before tick
// t is waited for); it must write the same two files.  mode 2: the whole recording time-parallel through
// BridgeRecordingTimeParallel (lyra_bridge_recording.h), one device call per stretch of constant membership, on
// --lanes=L lent stream slots (default 64); it must write the same files again, with --max-speakers=N too (not with
// --shared-encoders).
// mode 3: the whole recording through BridgeMeetingTimeParallel: ONE device call whatever the membership does, --lanes as mode 2.
// --present=<present.i32>: [ticks][num_streams] int32, 0 = the stream takes no part in that tick: it is no row of the tick,
// nothing is decoded or encoded for it, and its outgoing row is zeros with length 0.  Mode 3 hands the file to
// BridgeMeetingTimeParallel.  Modes 0 and 1 leave absent streams out of the tick's rows -- LyraConferenceBridge has every stream
// as a row of every tick, so with --present they run the ticks through the C ABI's begin / end forms themselves (mode 1 two
// deep) -- and must write the same files as mode 3.  Mode 2 and --shared-encoders take no --present.
// --max-speakers=N: the same call through LyraSpeakerBridge (lyra_speaker_bridge.h), every room mixed from its N loudest
// sources; every delivered tick's speaker flags [num_streams] int32 go to the file of --speakers-out.
// --shared-encoders (with --max-speakers): the same call through LyraSharedBridge (lyra_shared_bridge.h), 1 + N encoders per
// room.  Bitrate and DTX belong to a room there: before every tick each room takes the script's bitrate, and the streams.txt
// DTX switch, of its FIRST member (the lowest stream number); the other members' entries are not used.  The bridge gets as many
// rooms as the script's largest label + 1.  --slots-out: every delivered tick's speaker slots [num_streams] int32 (-1: none).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/lyra_hip_bridge.h"
#include "../../include/lyra_hip_speakers.h"
#include "lyra_bridge_recording.h"
#include "lyra_conference_bridge.h"
#include "lyra_shared_bridge.h"
#include "lyra_speaker_bridge.h"

using namespace chromemedia::codec;

namespace {

constexpr int kRow = kBridgePacketRowBytes;

template <class T>
bool ReadFile(const char* path, std::vector<T>* out) {
  std::ifstream in(path, std::ios::binary);
  if (!in) return false;
  std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (raw.size() % sizeof(T) != 0) return false;
  out->resize(raw.size() / sizeof(T));
  if (!raw.empty()) std::memcpy(out->data(), raw.data(), raw.size());
  return true;
}

int Fail(const char* what) {
  std::fprintf(stderr, "bridge_demo: %s\n", what);
  return 1;
}

int BitrateBits(int bitrate) { return bitrate == 3200 ? 64 : bitrate == 6000 ? 120 : bitrate == 9200 ? 184 : -1; }

// Modes 0 and 1 with --present: every tick's rows are the streams present on it, through lyra_hip_bridge_begin / _end or
// lyra_hip_speakers_begin / _end (two ticks deep when `pipelined`); a tick with nobody present is no call.  Fills
// out_rows [ticks][n][23], out_lens and flags [ticks][n]; what belongs to an absent stream stays zero.
bool RunPresentTicks(const char* model_dir, const std::vector<BridgeStream>& streams, const std::vector<int32_t>& script,
                     const std::vector<uint8_t>& packets, const std::vector<int32_t>& lengths, const std::vector<int32_t>& present,
                     bool pipelined, bool skip_comfort_noise, int max_speakers, std::vector<uint8_t>* out_rows,
                     std::vector<int32_t>* out_lens, std::vector<int32_t>* flags) {
  const size_t n = streams.size(), ticks = lengths.size() / n;
  out_rows->assign(ticks * n * kRow, 0);
  out_lens->assign(ticks * n, 0);
  flags->assign(ticks * n, 0);
  lyra_hip_ctx* ctx = nullptr;
  if (lyra_hip_create(model_dir, 0, static_cast<int>(n), LYRA_HIP_REQUANT_DEFAULT, &ctx) != 0) return false;
  std::vector<std::vector<size_t>> in_flight;   // the rows (tick * n + stream) of the ticks begun and not yet ended, oldest first
  bool ok = true;
  auto end_oldest = [&]() {
    const std::vector<size_t> rows = in_flight.front();
    in_flight.erase(in_flight.begin());
    const size_t B = rows.size();
    std::vector<uint8_t> pk(B * kRow);
    std::vector<int32_t> len(B), spk(B, 0);
    const int rc = max_speakers ? lyra_hip_speakers_end(ctx, pk.data(), len.data(), nullptr, nullptr, nullptr, spk.data())
                                : lyra_hip_bridge_end(ctx, pk.data(), len.data(), nullptr, nullptr);
    if (rc != 0) return false;
    for (size_t b = 0; b < B; ++b) {
      std::memcpy(&(*out_rows)[rows[b] * kRow], &pk[b * kRow], kRow);
      (*out_lens)[rows[b]] = len[b];
      (*flags)[rows[b]] = spk[b];
    }
    return true;
  };
  for (size_t t = 0; ok && t < ticks; ++t) {
    std::vector<size_t> rows;
    for (size_t s = 0; s < n; ++s)
      if (present[t * n + s] != 0) rows.push_back(t * n + s);
    const size_t B = rows.size();
    if (B == 0) continue;
    std::vector<int32_t> ids(B), len(B), rooms(B), muted(B), bits(B), dtx(B);
    std::vector<uint8_t> pk(B * kRow, 0);
    for (size_t b = 0; ok && b < B; ++b) {
      const size_t at = rows[b];
      ids[b] = static_cast<int32_t>(at % n);
      len[b] = lengths[at];
      if (len[b] < 0 || len[b] > kRow) ok = false;
      else std::memcpy(&pk[b * kRow], &packets[at * kRow], static_cast<size_t>(len[b]));
      rooms[b] = script[at * 3];
      muted[b] = script[at * 3 + 1] != 0;
      bits[b] = BitrateBits(script[at * 3 + 2]);
      dtx[b] = streams[at % n].enable_dtx ? 1 : 0;
      if (bits[b] < 0) ok = false;
    }
    if (!ok) break;
    const unsigned fl = skip_comfort_noise ? LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE : 0u;
    const int rc = max_speakers ? lyra_hip_speakers_begin(ctx, ids.data(), static_cast<int>(B), pk.data(), len.data(), rooms.data(),
                                                          muted.data(), fl, bits.data(), dtx.data(), max_speakers)
                                : lyra_hip_bridge_begin(ctx, ids.data(), static_cast<int>(B), pk.data(), len.data(), rooms.data(),
                                                        muted.data(), fl, bits.data(), dtx.data());
    if (rc != 0) {
      ok = false;
      break;
    }
    in_flight.push_back(rows);
    if (in_flight.size() > (pipelined ? 1u : 0u)) ok = end_oldest();
  }
  while (ok && !in_flight.empty()) ok = end_oldest();
  if (!ok) std::fprintf(stderr, "bridge_demo: %s\n", lyra_hip_last_error(ctx));
  lyra_hip_destroy(ctx);
  return ok;
}

}  // namespace

int main(int argc_all, char** argv_all) {
  // options first: what is left is the nine positional arguments
  int max_speakers = 0;
  const char* speakers_path = nullptr;
  const char* slots_path = nullptr;
  const char* present_path = nullptr;
  bool shared_encoders = false;
  int lanes = 64;
  std::vector<char*> positional;
  for (int i = 0; i < argc_all; ++i) {
    if (std::strncmp(argv_all[i], "--max-speakers=", 15) == 0) max_speakers = std::atoi(argv_all[i] + 15);
    else if (std::strncmp(argv_all[i], "--speakers-out=", 15) == 0) speakers_path = argv_all[i] + 15;
    else if (std::strncmp(argv_all[i], "--slots-out=", 12) == 0) slots_path = argv_all[i] + 12;
    else if (std::strcmp(argv_all[i], "--shared-encoders") == 0) shared_encoders = true;
    else if (std::strncmp(argv_all[i], "--lanes=", 8) == 0) lanes = std::atoi(argv_all[i] + 8);
    else if (std::strncmp(argv_all[i], "--present=", 10) == 0) present_path = argv_all[i] + 10;
    else positional.push_back(argv_all[i]);
  }
  const int argc = static_cast<int>(positional.size());
  char** argv = positional.data();
  const bool select = max_speakers != 0 || speakers_path != nullptr;
  if (argc != 10 || (select && (max_speakers == 0 || speakers_path == nullptr)) || (shared_encoders && !select) ||
      (slots_path && !shared_encoders)) {
    std::fprintf(stderr, "usage: bridge_demo <model_dir> <streams.txt> <script.i32> <packets_in.bin> <lengths_in.i32> "
                         "<packets_out.bin> <lengths_out.i32> <mode 0|1|2|3> <skip_comfort_noise 0|1> "
                         "[--max-speakers=N --speakers-out=<speakers_out.i32> [--shared-encoders [--slots-out=<slots_out.i32>]]] "
                         "[--lanes=L] [--present=<present.i32>]\n");
    return 2;
  }
  std::vector<BridgeStream> streams;
  {
    std::ifstream f(argv[2]);
    int bitrate, dtx;
    while (f >> bitrate >> dtx) streams.push_back({bitrate, dtx != 0});
  }
  const size_t n = streams.size();
  std::vector<int32_t> script, lengths;
  std::vector<uint8_t> packets;
  if (n == 0 || !ReadFile(argv[3], &script) || !ReadFile(argv[4], &packets) || !ReadFile(argv[5], &lengths))
    return Fail("unreadable input");
  const size_t ticks = lengths.size() / n;
  if (lengths.size() != ticks * n || script.size() != ticks * n * 3 || packets.size() != ticks * n * kRow)
    return Fail("the input files disagree about ticks and streams");
  const int mode = std::atoi(argv[8]);
  std::vector<int32_t> present;
  if (present_path) {
    if (mode == 2 || shared_encoders) return Fail("--present goes with modes 0, 1 and 3, without shared encoders");
    if (!ReadFile(present_path, &present) || present.size() != ticks * n) return Fail("the presence file disagrees about ticks and streams");
  }
  auto write_all = [&](const std::vector<uint8_t>& rows_out, const std::vector<int32_t>& lens_out, const std::vector<int32_t>& flags) {
    std::ofstream out_pk(argv[6], std::ios::binary), out_len(argv[7], std::ios::binary);
    out_pk.write(reinterpret_cast<const char*>(rows_out.data()), static_cast<std::streamsize>(rows_out.size()));
    out_len.write(reinterpret_cast<const char*>(lens_out.data()), static_cast<std::streamsize>(lens_out.size() * sizeof(int32_t)));
    if (speakers_path) {
      std::ofstream out_spk(speakers_path, std::ios::binary);
      out_spk.write(reinterpret_cast<const char*>(flags.data()), static_cast<std::streamsize>(flags.size() * sizeof(int32_t)));
    }
  };
  if (mode == 3) {   // the meeting as a whole, schedule and all
    if (shared_encoders) return Fail("mode 3 has no shared encoders");
    std::vector<int32_t> flags;
    auto got = BridgeMeetingTimeParallel(absl::MakeConstSpan(streams), argv[1], absl::MakeConstSpan(packets),
                                         absl::MakeConstSpan(lengths), absl::MakeConstSpan(script), absl::MakeConstSpan(present),
                                         std::atoi(argv[9]) != 0, max_speakers, lanes, 0, &flags);
    if (!got) return Fail("BridgeMeetingTimeParallel failed");
    write_all(got->first, got->second, flags);
    return 0;
  }
  if (present_path) {   // modes 0 and 1 with absent streams left out of the rows
    std::vector<uint8_t> rows_out;
    std::vector<int32_t> lens_out, flags;
    if (!RunPresentTicks(argv[1], streams, script, packets, lengths, present, mode != 0, std::atoi(argv[9]) != 0, max_speakers,
                         &rows_out, &lens_out, &flags))
      return Fail("a tick failed");
    write_all(rows_out, lens_out, flags);
    return 0;
  }
  if (mode == 2) {   // the recording as a whole
    if (shared_encoders) return Fail("mode 2 has no shared encoders");
    std::vector<int32_t> flags;
    auto got = BridgeRecordingTimeParallel(absl::MakeConstSpan(streams), argv[1], absl::MakeConstSpan(packets),
                                           absl::MakeConstSpan(lengths), absl::MakeConstSpan(script), std::atoi(argv[9]) != 0,
                                           max_speakers, lanes, 0, &flags);
    if (!got) return Fail("BridgeRecordingTimeParallel failed");
    std::ofstream out_pk(argv[6], std::ios::binary), out_len(argv[7], std::ios::binary);
    out_pk.write(reinterpret_cast<const char*>(got->first.data()), static_cast<std::streamsize>(got->first.size()));
    out_len.write(reinterpret_cast<const char*>(got->second.data()), static_cast<std::streamsize>(got->second.size() * sizeof(int32_t)));
    if (speakers_path) {
      std::ofstream out_spk(speakers_path, std::ios::binary);
      out_spk.write(reinterpret_cast<const char*>(flags.data()), static_cast<std::streamsize>(flags.size() * sizeof(int32_t)));
    }
    return 0;
  }
  const bool pipelined = mode != 0;
  std::unique_ptr<LyraConferenceBridge> bridge;
  LyraSpeakerBridge* speakers = nullptr;
  LyraSharedBridge* shared = nullptr;
  if (shared_encoders) {
    int max_rooms = 1;
    for (size_t i = 0; i < ticks * n; ++i) max_rooms = std::max(max_rooms, script[i * 3] + 1);
    auto b = LyraSharedBridge::Create(absl::MakeConstSpan(streams), argv[1], 0, std::atoi(argv[9]) != 0, max_speakers, max_rooms);
    shared = b.get();
    bridge = std::move(b);
  } else if (select) {
    auto b = LyraSpeakerBridge::Create(absl::MakeConstSpan(streams), argv[1], 0, std::atoi(argv[9]) != 0, max_speakers);
    speakers = b.get();
    bridge = std::move(b);
  } else {
    bridge = LyraConferenceBridge::Create(absl::MakeConstSpan(streams), argv[1], 0, std::atoi(argv[9]) != 0);
  }
  if (!bridge) return Fail("Create failed");
  std::ofstream out_pk(argv[6], std::ios::binary), out_len(argv[7], std::ios::binary), out_spk;
  std::ofstream out_slots;
  if (speakers || shared) out_spk.open(speakers_path, std::ios::binary);
  if (slots_path) out_slots.open(slots_path, std::ios::binary);
  auto write_speakers = [&]() {   // as of the tick just delivered
    if (!speakers && !shared) return;
    std::vector<int32_t> flags(n), slots(n, -1);
    for (size_t s = 0; s < n; ++s) {
      flags[s] = (speakers ? speakers->is_speaker(static_cast<int>(s)) : shared->is_speaker(static_cast<int>(s))) ? 1 : 0;
      if (shared) slots[s] = shared->slot(static_cast<int>(s));
    }
    out_spk.write(reinterpret_cast<const char*>(flags.data()), static_cast<std::streamsize>(flags.size() * sizeof(int32_t)));
    if (slots_path) out_slots.write(reinterpret_cast<const char*>(slots.data()), static_cast<std::streamsize>(slots.size() * sizeof(int32_t)));
  };
  std::vector<uint8_t> rows(n * kRow);
  std::vector<int32_t> lens(n);
  auto deliver = [&]() {
    if (!bridge->WaitTick(absl::Span<uint8_t>(rows.data(), rows.size()), absl::Span<int32_t>(lens.data(), lens.size()))) return false;
    out_pk.write(reinterpret_cast<const char*>(rows.data()), static_cast<std::streamsize>(rows.size()));
    out_len.write(reinterpret_cast<const char*>(lens.data()), static_cast<std::streamsize>(lens.size() * sizeof(int32_t)));
    write_speakers();
    return true;
  };
  for (size_t t = 0; t < ticks; ++t) {
    for (size_t s = n; shared && s-- > 0;) {   // descending: the room's FIRST member is the last to set it
      const int32_t* row = &script[(t * n + s) * 3];
      if (row[0] >= 0 && (!shared->SetRoomBitrate(row[0], row[2]) || !shared->SetRoomDtx(row[0], streams[s].enable_dtx)))
        return Fail("the script names a room setting the bridge refuses");
    }
    for (size_t s = 0; s < n; ++s) {
      const int32_t* row = &script[(t * n + s) * 3];
      if (!bridge->SetRoom(static_cast<int>(s), row[0]) || !bridge->SetMuted(static_cast<int>(s), row[1] != 0) ||
          !bridge->set_bitrate(static_cast<int>(s), row[2]))
        return Fail("the script names a setting the bridge refuses");
    }
    if (!bridge->SetEncodedPackets(absl::MakeConstSpan(&packets[t * n * kRow], n * kRow), absl::MakeConstSpan(&lengths[t * n], n)))
      return Fail("SetEncodedPackets failed");
    if (!pipelined) {
      auto got = bridge->Tick();
      if (!got) return Fail("Tick failed");
      out_pk.write(reinterpret_cast<const char*>(got->first.data()), static_cast<std::streamsize>(got->first.size()));
      out_len.write(reinterpret_cast<const char*>(got->second.data()), static_cast<std::streamsize>(got->second.size() * sizeof(int32_t)));
      write_speakers();
      continue;
    }
    if (!bridge->TickAsync()) return Fail("TickAsync failed");
    if (t >= 1 && !deliver()) return Fail("WaitTick failed");
  }
  if (pipelined)
    while (bridge->ticks_in_flight() > 0)
      if (!deliver()) return Fail("WaitTick failed");
  return 0;
}
