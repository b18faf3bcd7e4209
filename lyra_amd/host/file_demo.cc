// file_demo.cc -- batched encoder_main / decoder_main (cli_example/encoder_main.cc, decoder_main.cc):
//   file_demo [--time-parallel[=<lanes>]] [--decode-rate=<hz>] [--dtx] <model_dir> <bitrate> <out_dir> <a.wav> [<b.wav> ...]
// writes <out_dir>/<stem>.lyra and <out_dir>/<stem>_decoded.wav for every input, all files transcoded together.
// The encoder's sample rate is the WAVs' (8, 16, 32 or 48 kHz, one per batch); --decode-rate: that of the decoded WAVs (16000).
// --time-parallel: through EncodeFilesTimeParallel / DecodeFilesTimeParallel (long files cut into chunks that run side by
// side; the same bytes).
// --dtx: encoder_main's --enable_dtx; noise hops append nothing to the .lyra file.  Such a file carries no framing (the
// reference's format), so it is not decoded: only <stem>.lyra is written.
// --dtx --time-parallel: the encode's packets and sizes are also decoded in memory, time-parallel (lyra_hip_decode_spans_lossy)
// and hop by hop (BatchLyraDecoder); the two must give the same samples, else exit code 8.  One line on stdout says so.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

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

int main(int argc, char** argv) {
  if (argc == 4 && std::string(argv[1]) == "--selftest-wav") return SelftestWav(argv[2], argv[3]);
  int lanes = -1;   // < 0: hop by hop
  int decode_rate = 16000;
  bool dtx = false;
  for (; argc > 1 && std::string(argv[1]).rfind("--", 0) == 0; --argc, ++argv) {
    const std::string flag = argv[1];
    if (flag.rfind("--time-parallel", 0) == 0) {
      lanes = flag.size() > 16 && flag[15] == '=' ? std::atoi(flag.c_str() + 16) : kDefaultSpanLanes;
    } else if (flag.rfind("--decode-rate=", 0) == 0) {
      decode_rate = std::atoi(flag.c_str() + 14);
    } else if (flag == "--dtx") {
      dtx = true;
    } else {
      argc = 0;   // unknown flag: usage
      break;
    }
  }
  if (argc < 5) {
    std::fprintf(stderr, "usage: file_demo [--time-parallel[=lanes]] [--decode-rate=hz] [--dtx] model_dir bitrate out_dir a.wav [b.wav ...]\n");
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
