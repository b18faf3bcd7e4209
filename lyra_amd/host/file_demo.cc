// file_demo.cc -- batched encoder_main / decoder_main (cli_example/encoder_main.cc, decoder_main.cc):
//   file_demo [--time-parallel[=<lanes>]] [--decode-rate=<hz>] [--dtx] [--bitrate-schedule=<k>] <model_dir> <bitrate> <out_dir>
//             <a.wav> [<b.wav> ...]
// writes <out_dir>/<stem>.lyra and <out_dir>/<stem>_decoded.wav for every input, all files transcoded together.
// The encoder's sample rate is the WAVs' (8, 16, 32 or 48 kHz, one per batch); --decode-rate: that of the decoded WAVs (16000).
// --time-parallel: through EncodeFilesTimeParallel / DecodeFilesTimeParallel (long files cut into chunks that run side by
// side; the same bytes).
// --dtx: encoder_main's --enable_dtx; noise hops append nothing to the .lyra file.  Such a file carries no framing (the
// reference's format), so it is not decoded: only <stem>.lyra is written.
// --dtx --time-parallel: the encode's packets and sizes are also decoded in memory, time-parallel (lyra_hip_decode_spans_lossy)
// and hop by hop (BatchLyraDecoder); the two must give the same samples, else exit code 8.  One line on stdout says so.
// --bitrate-schedule=<k> --time-parallel: the bitrate cycles 3200 -> 6000 -> 9200 every k hops for every file (<bitrate> is not
// used).  The schedule runs in memory time-parallel (lyra_hip_encode_spans_mixed, lyra_hip_decode_spans_lossy_mixed) and hop by
// hop (BatchLyraEncoder with set_bitrate before each hop, BatchLyraDecoder::SetEncodedPackets with that hop's size); packets and
// samples must be the same, else exit code 8.  One line on stdout says so.  The .lyra format has no framing: no file is written.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "lyra_batch_codec.h"
#include "lyra_file_codec.h"

using namespace chromemedia::codec;
namespace fs = ghc::filesystem;

// --selftest-wav <in.wav> <out.wav>: read with ReadWav16, write back with WriteWav16 (CPU only; used by the tests)
static int SelftestWav(const char* in, const char* out) {
  std::vector<int16_t> samples;
  int ch = 0, rate = 0;
  if (!ReadWav16(in, &samples, &ch, &rate)) return 6;
  std::printf("%d %d %zu\n", ch, rate, samples.size());
  return WriteWav16(out, samples, ch, rate) ? 0 : 7;
}

// --bitrate-schedule: see the head of the file.  Returns the exit code.
static int MixedRoundTrip(const std::vector<fs::path>& wavs, int every, int decode_rate, const fs::path& model_dir, int lanes) {
  const int n = (int)wavs.size();
  std::vector<std::vector<int16_t>> pcm(wavs.size()), tp, seq(wavs.size());
  int rate = 0;
  for (size_t i = 0; i < wavs.size(); ++i) {
    int ch = 0, r = 0;
    if (!ReadWav16(wavs[i], &pcm[i], &ch, &r) || ch != 1 || (i && r != rate)) return 4;
    rate = r;
  }
  const size_t hop = (size_t)rate / 50, out_hop = (size_t)decode_rate / 50;
  size_t max_hops = 0;
  std::vector<std::vector<int>> bitrates(wavs.size());
  const int cycle[3] = {3200, 6000, 9200};
  for (size_t i = 0; i < wavs.size(); ++i) {
    for (size_t h = 0; h < pcm[i].size() / hop; ++h) bitrates[i].push_back(cycle[(h / (size_t)every) % 3]);
    max_hops = std::max(max_hops, bitrates[i].size());
  }
  // time-parallel
  std::vector<std::vector<uint8_t>> packets, packets_seq(wavs.size());
  std::vector<std::vector<int32_t>> sizes, sizes_seq(wavs.size());
  if (!EncodeWavsTimeParallel(pcm, 1, rate, bitrates, false, false, model_dir, &packets, &sizes, lanes)) return 4;
  if (!DecodeFeaturesTimeParallel(packets, sizes, decode_rate, model_dir, &tp, lanes)) return 5;
  // hop by hop: a file that has ended is fed silence and its packets are dropped
  auto encoder = BatchLyraEncoder::Create(rate, 1, 3200, false, model_dir, n);
  auto decoder = BatchLyraDecoder::Create(decode_rate, 1, model_dir, n);
  if (!encoder || !decoder) return 4;
  std::vector<int16_t> frame((size_t)n * hop);
  for (size_t h = 0; h < max_hops; ++h) {
    const int bitrate = cycle[(h / (size_t)every) % 3];
    if (!encoder->set_bitrate(bitrate)) return 4;
    for (int i = 0; i < n; ++i) {
      if (h < bitrates[i].size()) std::copy_n(pcm[i].begin() + h * hop, hop, frame.begin() + i * hop);
      else std::fill_n(frame.begin() + i * hop, hop, 0);
    }
    const auto encoded = encoder->Encode(absl::MakeConstSpan(frame));
    if (!encoded) return 4;
    const size_t size = (size_t)encoder->packet_size();
    std::vector<int32_t> ids;
    std::vector<uint8_t> fed;
    for (int i = 0; i < n; ++i) {
      if (h >= bitrates[i].size()) continue;
      packets_seq[i].insert(packets_seq[i].end(), encoded->begin() + i * size, encoded->begin() + (i + 1) * size);
      sizes_seq[i].push_back((int32_t)size);
      ids.push_back(i);
      fed.insert(fed.end(), encoded->begin() + i * size, encoded->begin() + (i + 1) * size);
    }
    if (!decoder->SetEncodedPackets(absl::MakeConstSpan(ids), absl::MakeConstSpan(fed))) return 5;
    const auto decoded = decoder->DecodeSamples((int)out_hop);
    if (!decoded) return 5;
    for (int i : ids) seq[i].insert(seq[i].end(), decoded->begin() + i * out_hop, decoded->begin() + (i + 1) * out_hop);
  }
  size_t hops = 0, by_size[3] = {0, 0, 0};
  for (const auto& v : sizes)
    for (int32_t b : v) { ++hops; by_size[b == 8 ? 0 : b == 15 ? 1 : 2] += 1; }
  const bool enc_same = packets == packets_seq && sizes == sizes_seq, dec_same = tp == seq;
  std::printf("mixed round trip: %zu hops, x8 %zu x15 %zu x23 %zu packets, time-parallel and hop by hop: encode %s decode %s\n", hops,
              by_size[0], by_size[1], by_size[2], enc_same ? "equal" : "DIFFER", dec_same ? "equal" : "DIFFER");
  return enc_same && dec_same ? 0 : 8;
}

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "--selftest-wav") return SelftestWav(argv[2], argv[3]);
  int lanes = -1;   // < 0: hop by hop
  int decode_rate = 16000;
  bool dtx = false;
  int schedule = 0;   // > 0: the bitrate changes every `schedule` hops
  for (; argc > 1 && std::string(argv[1]).rfind("--", 0) == 0; --argc, ++argv) {
    const std::string flag = argv[1];
    if (flag.rfind("--time-parallel", 0) == 0) {
      lanes = flag.size() > 16 && flag[15] == '=' ? std::atoi(flag.c_str() + 16) : kDefaultSpanLanes;
    } else if (flag.rfind("--decode-rate=", 0) == 0) {
      decode_rate = std::atoi(flag.c_str() + 14);
    } else if (flag == "--dtx") {
      dtx = true;
    } else if (flag.rfind("--bitrate-schedule=", 0) == 0) {
      schedule = std::atoi(flag.c_str() + 19);
      if (schedule <= 0) argc = 0;
    } else {
      argc = 0;   // unknown flag: usage
      break;
    }
  }
  if (argc < 5 || (schedule && (lanes < 0 || dtx))) {
    std::fprintf(stderr, "usage: file_demo [--time-parallel[=lanes]] [--decode-rate=hz] [--dtx] [--bitrate-schedule=hops] model_dir "
                         "bitrate out_dir a.wav [b.wav ...]\n  (--bitrate-schedule needs --time-parallel and excludes --dtx)\n");
    return 2;
  }
  const fs::path model_dir = argv[1], out_dir = argv[3];
  const int bitrate = std::atoi(argv[2]);
  std::vector<fs::path> wavs, lyras, decoded;
  for (int i = 4; i < argc; ++i) {
    fs::path w = argv[i];
    wavs.push_back(w);
    lyras.push_back(out_dir / (w.stem().string() + ".lyra"));
    decoded.push_back(out_dir / (w.stem().string() + "_decoded.wav"));
  }
  if (schedule) return MixedRoundTrip(wavs, schedule, decode_rate, model_dir, lanes);
  if (EncodeFiles(wavs, lyras, 1234, false, false, model_dir)) return 3;      // unsupported bitrate
  if (EncodeFiles(wavs, lyras, bitrate, true, false, model_dir)) return 3;    // preprocessing is outside this build
  if (lanes >= 0) {
    if (!EncodeFilesTimeParallel(wavs, lyras, bitrate, false, dtx, model_dir, lanes)) return 4;
    if (!dtx && !DecodeFilesTimeParallel(lyras, decoded, decode_rate, bitrate, model_dir, lanes)) return 5;
    if (dtx) {
      std::vector<std::vector<int16_t>> pcm(wavs.size()), tp, seq;
      int rate = 0;
      for (size_t i = 0; i < wavs.size(); ++i) {
        int ch = 0, r = 0;
        if (!ReadWav16(wavs[i], &pcm[i], &ch, &r) || ch != 1 || (i && r != rate)) return 4;
        rate = r;
      }
      std::vector<std::vector<uint8_t>> packets;
      std::vector<std::vector<int32_t>> sizes;
      if (!EncodeWavsTimeParallel(pcm, 1, rate, bitrate, false, true, model_dir, &packets, lanes, 0, &sizes)) return 4;
      const int packet_size = bitrate == 3200 ? 8 : bitrate == 6000 ? 15 : 23;
      if (!DecodeFeaturesTimeParallel(packets, sizes, packet_size, decode_rate, model_dir, &tp, lanes)) return 5;
      if (!DecodeFeaturesBatch(packets, sizes, packet_size, decode_rate, model_dir, &seq)) return 5;
      size_t hops = 0, empty = 0;
      for (const auto& v : sizes)
        for (int32_t b : v) { ++hops; empty += b == 0; }
      const bool same = tp == seq;
      std::printf("dtx round trip: %zu hops, %zu empty packets, time-parallel and hop-by-hop decode %s\n", hops, empty,
                  same ? "equal" : "DIFFER");
      if (!same) return 8;
    }
    return 0;
  }
  if (!EncodeFiles(wavs, lyras, bitrate, false, dtx, model_dir)) return 4;
  if (!dtx && !DecodeFiles(lyras, decoded, decode_rate, bitrate, model_dir)) return 5;
  return 0;
}
