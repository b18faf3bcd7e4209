// archive_demo.cc -- an archive of recordings at ANY of the four rates, transcoded in one call per direction:
//   archive_demo [--lanes=<n>] [--dtx] [--decode-rates=<hz,hz,...>] <model_dir> <bitrate> <out_dir> <a.wav> [<b.wav> ...]
// Every WAV is mono at 8, 16, 32 or 48 kHz, each at its own rate.  The files are encoded and decoded twice, in memory:
//   time-parallel   EncodeWavsAnyRateTimeParallel / DecodeFeaturesAnyRateTimeParallel (lyra_file_codec.h): every file one span of
//                   one call, its samples packed back to back (include/lyra_hip_spans_packed.h), <n> lanes (default
//                   kDefaultSpanLanes);
//   hop by hop      MixedBatchLyraEncoder / MixedBatchLyraDecoder, one stream per file; a file that has ended is fed silence
//                   and its output is dropped.
// --decode-rates: the rate of each decoded WAV, one per file or one for all (default: the file's own).  --dtx: encoder_main's
// --enable_dtx for every file; noise hops carry no packet.
// Writes <out_dir>/<stem>_decoded.wav and, without --dtx (a DTX stream has no framing), <out_dir>/<stem>.lyra, both from the
// time-parallel result, and prints one line: hops per rate and "encode equal|DIFFER decode equal|DIFFER".  Exit code 8 if
// either differs.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "lyra_file_codec.h"
#include "lyra_mixed_decoder.h"
#include "lyra_mixed_encoder.h"

using namespace chromemedia::codec;
namespace fs = ghc::filesystem;

int main(int argc, char** argv) {
  int lanes = kDefaultSpanLanes;
  bool dtx = false;
  std::vector<int> decode_rates;
  for (; argc > 1 && std::string(argv[1]).rfind("--", 0) == 0; --argc, ++argv) {
    const std::string flag = argv[1];
    if (flag.rfind("--lanes=", 0) == 0) {
      lanes = std::atoi(flag.c_str() + 8);
    } else if (flag == "--dtx") {
      dtx = true;
    } else if (flag.rfind("--decode-rates=", 0) == 0) {
      for (size_t at = 15; at < flag.size();) {
        decode_rates.push_back(std::atoi(flag.c_str() + at));
        const size_t comma = flag.find(',', at);
        at = comma == std::string::npos ? flag.size() : comma + 1;
      }
    } else {
      argc = 0;   // unknown flag: usage
      break;
    }
  }
  const int n = argc - 4;
  if (n < 1 || lanes < 0 || (decode_rates.size() > 1 && (int)decode_rates.size() != n)) {
    std::fprintf(stderr, "usage: archive_demo [--lanes=n] [--dtx] [--decode-rates=hz,hz,...] model_dir bitrate out_dir a.wav "
                         "[b.wav ...]\n  (--decode-rates: one rate per file, or one for all)\n");
    return 2;
  }
  const fs::path model_dir = argv[1], out_dir = argv[3];
  const int bitrate = std::atoi(argv[2]);
  std::vector<fs::path> wavs;
  std::vector<std::vector<int16_t>> pcm((size_t)n);
  std::vector<int> rates((size_t)n);
  for (int i = 0; i < n; ++i) {
    wavs.push_back(argv[4 + i]);
    int ch = 0;
    if (!ReadWav16(wavs[i], &pcm[i], &ch, &rates[i]) || ch != 1) return 3;
  }
  if (decode_rates.empty()) decode_rates = rates;
  if (decode_rates.size() == 1) decode_rates.assign((size_t)n, decode_rates[0]);

  // time-parallel: one call per direction
  std::vector<std::vector<uint8_t>> packets, packets_seq((size_t)n);
  std::vector<std::vector<int32_t>> sizes, sizes_seq((size_t)n);
  std::vector<std::vector<int16_t>> tp, seq((size_t)n);
  if (!EncodeWavsAnyRateTimeParallel(pcm, rates, bitrate, dtx, model_dir, &packets, &sizes, lanes)) return 4;
  if (!DecodeFeaturesAnyRateTimeParallel(packets, sizes, decode_rates, model_dir, &tp, lanes)) return 5;

  // hop by hop: one stream per file
  std::vector<MixedBatchLyraEncoder::EncoderParams> params;
  for (int i = 0; i < n; ++i) params.push_back({rates[i], bitrate, dtx});
  auto encoder = MixedBatchLyraEncoder::Create(absl::MakeConstSpan(params), 1, model_dir);
  auto decoder = MixedBatchLyraDecoder::Create(absl::MakeConstSpan(decode_rates), 1, model_dir);
  if (!encoder) return 4;
  if (!decoder) return 5;
  size_t max_hops = 0, hops_at[4] = {0, 0, 0, 0};
  std::vector<size_t> hops((size_t)n);
  for (int i = 0; i < n; ++i) {
    hops[i] = pcm[i].size() / (size_t)(rates[i] / 50);
    max_hops = std::max(max_hops, hops[i]);
    hops_at[rates[i] == 8000 ? 0 : rates[i] == 16000 ? 1 : rates[i] == 32000 ? 2 : 3] += hops[i];
  }
  std::vector<int16_t> frame;
  for (size_t h = 0; h < max_hops; ++h) {
    frame.clear();
    for (int i = 0; i < n; ++i) {
      const size_t hop = (size_t)rates[i] / 50;
      if (h < hops[i]) frame.insert(frame.end(), pcm[i].begin() + h * hop, pcm[i].begin() + (h + 1) * hop);
      else frame.insert(frame.end(), hop, 0);
    }
    const auto rows = encoder->Encode(absl::MakeConstSpan(frame));
    if (!rows) return 4;
    std::vector<int32_t> lengths = encoder->packet_lengths();
    for (int i = 0; i < n; ++i) {
      if (h >= hops[i]) { lengths[i] = 0; continue; }   // the ended file's packet is dropped: its decoder stream conceals
      packets_seq[i].insert(packets_seq[i].end(), rows->begin() + i * kMixedPacketRowBytes,
                            rows->begin() + i * kMixedPacketRowBytes + lengths[i]);
      sizes_seq[i].push_back(lengths[i]);
    }
    if (!decoder->SetEncodedPackets(absl::MakeConstSpan(*rows), absl::MakeConstSpan(lengths))) return 5;
    const auto decoded = decoder->DecodeHop();
    if (!decoded) return 5;
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
      const size_t hop = (size_t)decode_rates[i] / 50;
      if (h < hops[i]) seq[i].insert(seq[i].end(), decoded->begin() + at, decoded->begin() + at + hop);
      at += hop;
    }
  }

  for (int i = 0; i < n; ++i) {
    const std::string stem = wavs[i].stem().string();
    if (!WriteWav16(out_dir / (stem + "_decoded.wav"), tp[i], 1, decode_rates[i])) return 6;
    if (dtx) continue;
    std::ofstream out((out_dir / (stem + ".lyra")).string(), std::ios_base::binary | std::ios_base::trunc);
    if (!out.is_open()) return 6;
    out.write(reinterpret_cast<const char*>(packets[i].data()), packets[i].size());
  }
  size_t empty = 0;
  for (const auto& v : sizes)
    for (int32_t b : v) empty += b == 0;
  const bool enc_same = packets == packets_seq && sizes == sizes_seq, dec_same = tp == seq;
  std::printf("archive round trip: hops at 8 kHz %zu, 16 kHz %zu, 32 kHz %zu, 48 kHz %zu, %zu empty packets; time-parallel and hop by "
              "hop: encode %s decode %s\n", hops_at[0], hops_at[1], hops_at[2], hops_at[3], empty, enc_same ? "equal" : "DIFFER",
              dec_same ? "equal" : "DIFFER");
  return enc_same && dec_same ? 0 : 8;
}
