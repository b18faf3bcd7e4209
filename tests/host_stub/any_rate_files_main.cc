// any_rate_files_main.cc -- TEST INFRASTRUCTURE (tests/test_spans_packed_cpu.py): the any-rate file functions of
// lyra_amd/host/lyra_file_codec.h behind a small main, because archive_demo's hop-by-hop half needs MixedBatchLyraEncoder /
// MixedBatchLyraDecoder, whose C calls the CPU stand-ins of tests/host_stub do not have.
//   any_rate_files_main <bitrate> <out_dir> <decode rate,decode rate,...> <a.wav> ...
// writes <out_dir>/<stem>.lyra and <out_dir>/<stem>_decoded.wav; exit 4: the encode failed, 5: the decode failed.
#include <cstdlib>
#include <string>
#include <vector>

#include "lyra_file_codec.h"

using namespace chromemedia::codec;
namespace fs = ghc::filesystem;

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const int bitrate = std::atoi(argv[1]);
  const fs::path out_dir = argv[2];
  std::vector<int> rates;
  const std::string csv = argv[3];
  for (size_t at = 0; at < csv.size();) {
    rates.push_back(std::atoi(csv.c_str() + at));
    const size_t comma = csv.find(',', at);
    at = comma == std::string::npos ? csv.size() : comma + 1;
  }
  std::vector<fs::path> wavs, lyras, decoded;
  for (int i = 4; i < argc; ++i) {
    wavs.push_back(argv[i]);
    lyras.push_back(out_dir / (wavs.back().stem().string() + ".lyra"));
    decoded.push_back(out_dir / (wavs.back().stem().string() + "_decoded.wav"));
  }
  if (!EncodeFilesAnyRateTimeParallel(wavs, lyras, bitrate, false, "unused_model_dir", 64)) return 4;
  if (!DecodeFilesAnyRateTimeParallel(lyras, decoded, rates, bitrate, "unused_model_dir", 64)) return 5;
  return 0;
}
