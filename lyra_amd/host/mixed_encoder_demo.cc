// mixed_encoder_demo.cc -- drives MixedBatchLyraEncoder (lyra_mixed_encoder.h) through a scripted session in which every
// stream has its own sample rate, bitrate and DTX setting and bitrates switch while the session runs:
//   mixed_encoder_demo <model_dir> <params.txt> <switches.txt> <pcm_in.s16> <packets_out.bin> <lengths_out.i32>
// params.txt, one line per stream:        <sample_rate_hz> <bitrate> <dtx 0|1>
// switches.txt, one line per switch:      <hop> <stream> <bitrate>      set_bitrate(stream, bitrate) before hop <hop> is begun
// pcm_in: [hops][packed hop] int16, a packed hop = the streams' sample_rate / 50 samples back to back.  Writes every hop's
// packets [num_streams][23] and lengths [num_streams].
// LYRA_DEMO_PIPELINED=1: the same session through EncodeAsync / WaitEncoded, two hops deep (hop t + 1 is begun before hop t is
// waited for); it must write the same two files.
//   mixed_encoder_demo --bench <model_dir> <params.txt> <hops> <windows> [mixed|classes]
// times sessions of <hops> hops, two deep, on synthetic audio, <windows> times each and alternating, through
//   "mixed"    one MixedBatchLyraEncoder for the whole table, and
//   "classes"  one BatchLyraEncoder per (sample rate, DTX) class of the table, at the bitrate of the class's first stream
//              (a BatchLyraEncoder has one bitrate), driven round robin,
// and prints one JSON line per window.  With a last argument only that engine is created and timed (the other one's contexts
// and streams are then absent from the process).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "lyra_batch_codec.h"
#include "lyra_mixed_encoder.h"

using namespace chromemedia::codec;
using Params = MixedBatchLyraEncoder::EncoderParams;

namespace {

bool ReadParams(const char* path, std::vector<Params>* out) {
  std::ifstream f(path);
  int rate, bitrate, dtx;
  while (f >> rate >> bitrate >> dtx) out->push_back(Params{rate, bitrate, dtx != 0});
  return !out->empty();
}

// deterministic audio for the timed sessions: a few tones per stream under noise, every fourth stream quiet
void FillHop(const std::vector<Params>& p, int hop, std::vector<int16_t>* pcm) {
  size_t k = 0;
  uint32_t x = 0x9E3779B9u * static_cast<uint32_t>(hop + 1);
  for (size_t s = 0; s < p.size(); ++s) {
    const int n = p[s].sample_rate_hz / 50, amp = (s & 3) == 3 ? 20 : 6000;
    for (int i = 0; i < n; ++i) {
      x = x * 1664525u + 1013904223u;
      (*pcm)[k++] = static_cast<int16_t>(static_cast<int>(x >> 16) % (2 * amp + 1) - amp);
    }
  }
}

double Seconds() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int Bench(int argc, char** argv) {
  if (argc != 6 && argc != 7) { std::fprintf(stderr, "usage: see mixed_encoder_demo.cc\n"); return 2; }
  const std::string only = argc == 7 ? argv[6] : "";
  if (!only.empty() && only != "mixed" && only != "classes") return 2;
  const bool use[2] = {only != "classes", only != "mixed"};   // [mixed, classes]
  const std::string model_dir = argv[2];
  std::vector<Params> params;
  if (!ReadParams(argv[3], &params)) return 3;
  const int hops = std::atoi(argv[4]), windows = std::atoi(argv[5]);
  if (hops < 2 || windows < 1) return 3;
  const int n = static_cast<int>(params.size());
  std::unique_ptr<MixedBatchLyraEncoder> mixed;
  if (use[0] && !(mixed = MixedBatchLyraEncoder::Create(absl::MakeConstSpan(params), 1, model_dir))) return 1;
  // the classes, in order of first appearance; members in stream order
  std::vector<std::pair<int, bool>> keys;
  std::map<std::pair<int, bool>, std::vector<int>> members;
  for (int s = 0; s < n; ++s) {
    const auto key = std::make_pair(params[s].sample_rate_hz, params[s].enable_dtx);
    if (!members.count(key)) keys.push_back(key);
    members[key].push_back(s);
  }
  std::vector<std::unique_ptr<BatchLyraEncoder>> objs;
  for (const auto& key : keys) {
    if (!use[1]) break;
    objs.push_back(BatchLyraEncoder::Create(key.first, 1, params[members[key][0]].bitrate, key.second, model_dir,
                                            static_cast<int>(members[key].size())));
    if (!objs.back()) return 1;
  }
  size_t hop_samples = 0;
  std::vector<size_t> start(n);
  for (int s = 0; s < n; ++s) { start[s] = hop_samples; hop_samples += params[s].sample_rate_hz / 50; }
  // two hops of audio, alternating; the classes' copies hold the same samples per stream
  std::vector<int16_t> pcm[2] = {std::vector<int16_t>(hop_samples), std::vector<int16_t>(hop_samples)};
  std::vector<std::vector<int16_t>> cls[2];
  for (int h = 0; h < 2; ++h) {
    FillHop(params, h, &pcm[h]);
    for (const auto& key : keys) {
      std::vector<int16_t> a;
      for (int s : members[key]) a.insert(a.end(), pcm[h].begin() + start[s], pcm[h].begin() + start[s] + key.first / 50);
      cls[h].push_back(std::move(a));
    }
  }
  auto run_mixed = [&]() {
    if (!mixed->EncodeAsync(absl::MakeConstSpan(pcm[0]))) return false;
    for (int t = 0; t < hops; ++t) {
      if (t + 1 < hops && !mixed->EncodeAsync(absl::MakeConstSpan(pcm[(t + 1) & 1]))) return false;
      if (!mixed->WaitEncoded()) return false;
    }
    return true;
  };
  auto run_classes = [&]() {
    for (size_t k = 0; k < objs.size(); ++k)
      if (!objs[k]->EncodeAsync(absl::MakeConstSpan(cls[0][k]))) return false;
    for (int t = 0; t < hops; ++t) {
      if (t + 1 < hops)
        for (size_t k = 0; k < objs.size(); ++k)
          if (!objs[k]->EncodeAsync(absl::MakeConstSpan(cls[(t + 1) & 1][k]))) return false;
      for (auto& o : objs)
        if (!o->WaitEncoded()) return false;
    }
    return true;
  };
  if ((use[0] && !run_mixed()) || (use[1] && !run_classes())) return 4;   // warm-up: allocations, code objects
  for (int w = 0; w < windows; ++w)
    for (int engine = 0; engine < 2; ++engine) {
      if (!use[engine]) continue;
      const double t0 = Seconds();
      if (!(engine == 0 ? run_mixed() : run_classes())) return 4;
      const double dt = Seconds() - t0;
      std::printf("{\"engine\": \"%s\", \"streams\": %d, \"classes\": %zu, \"hops\": %d, \"window\": %d, \"seconds\": %.6f, "
                  "\"frames_per_s\": %.1f}\n", engine == 0 ? "mixed" : "classes", n, keys.size(), hops, w, dt,
                  static_cast<double>(n) * hops / dt);
      std::fflush(stdout);
    }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--bench") == 0) return Bench(argc, argv);
  if (argc != 7) { std::fprintf(stderr, "usage: see mixed_encoder_demo.cc\n"); return 2; }
  const char* e = std::getenv("LYRA_DEMO_PIPELINED");
  const int mode = e ? std::atoi(e) : 0;
  if (mode < 0 || mode > 1) { std::fprintf(stderr, "LYRA_DEMO_PIPELINED must be 0 or 1\n"); return 2; }
  std::vector<Params> params;
  if (!ReadParams(argv[2], &params)) return 3;
  std::multimap<int, std::pair<int, int>> switches;   // hop -> (stream, bitrate)
  {
    std::ifstream f(argv[3]);
    int hop, stream, bitrate;
    while (f >> hop >> stream >> bitrate) switches.insert({hop, {stream, bitrate}});
  }
  std::ifstream in(argv[4], std::ios::binary);
  std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  std::vector<int16_t> pcm(raw.size() / 2);
  std::memcpy(pcm.data(), raw.data(), pcm.size() * 2);
  auto enc = MixedBatchLyraEncoder::Create(absl::MakeConstSpan(params), 1, argv[1]);
  if (!enc) { std::fprintf(stderr, "creation failed\n"); return 1; }
  const int n = enc->num_streams();
  size_t frame = 0;
  for (int s = 0; s < n; ++s) frame += enc->sample_rate_hz(s) / 50;
  if (pcm.size() % frame != 0) return 3;
  const int hops = static_cast<int>(pcm.size() / frame);
  std::ofstream pk_out(argv[5], std::ios::binary), len_out(argv[6], std::ios::binary);
  auto begin = [&](int t) {   // the switches scripted for hop t, then the hop
    const auto range = switches.equal_range(t);
    for (auto it = range.first; it != range.second; ++it)
      if (!enc->set_bitrate(it->second.first, it->second.second)) return false;
    return enc->EncodeAsync(absl::MakeConstSpan(pcm.data() + static_cast<size_t>(t) * frame, frame));
  };
  auto write = [&](const std::vector<uint8_t>& packets) {
    pk_out.write(reinterpret_cast<const char*>(packets.data()), packets.size());
    len_out.write(reinterpret_cast<const char*>(enc->packet_lengths().data()), n * 4);
  };
  if (mode == 1) {
    if (hops > 0 && !begin(0)) return 4;
    for (int t = 0; t < hops; ++t) {
      if (t + 1 < hops && !begin(t + 1)) return 4;
      if (enc->hops_in_flight() != (t + 1 < hops ? 2 : 1)) return 7;
      auto packets = enc->WaitEncoded();
      if (!packets) return 4;
      write(*packets);
    }
    return 0;
  }
  for (int t = 0; t < hops; ++t) {
    const auto range = switches.equal_range(t);
    for (auto it = range.first; it != range.second; ++it)
      if (!enc->set_bitrate(it->second.first, it->second.second)) return 4;
    auto packets = enc->Encode(absl::MakeConstSpan(pcm.data() + static_cast<size_t>(t) * frame, frame));
    if (!packets) return 4;
    write(*packets);
  }
  return 0;
}
