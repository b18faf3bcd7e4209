// mixed_decoder_demo.cc -- drives MixedBatchLyraDecoder (lyra_mixed_decoder.h) through a scripted session in which every stream
// has its own sample rate, packets change size from hop to hop and some hops arrive without a packet:
//   mixed_decoder_demo <model_dir> <rates.txt> <packets_in.bin> <lengths_in.i32> <pcm_out.s16> <flags_out.i32>
// rates.txt: one sample rate per line and stream.  packets_in: [hops][num_streams][23] bytes; lengths_in: [hops][num_streams]
// int32, 0 = no packet for that stream on that hop.  Writes every hop's packed samples (the streams' sample_rate / 50 samples
// back to back) and every hop's is_comfort_noise flags [num_streams] int32.
// LYRA_DEMO_PIPELINED=1: the same session through DecodeHopAsync / WaitDecoded, two hops deep (hop t + 1 is begun before hop t
// is waited for); it must write the same two files.
//   mixed_decoder_demo --bench <model_dir> <rates.txt> <hops> <windows> [engines]
// times sessions of <hops> hops, two deep, on random packets of 15 bytes under Gilbert loss (10 %, mean burst 2), <windows>
// times each and alternating, through the engines named in the comma-separated list [engines] (default: all three):
//   "mixed"    one MixedBatchLyraDecoder for the whole table,
//   "batch"    one BatchLyraDecoder per sample rate of the table, driven round robin,
//   "device"   one DeviceLyraDecoder per sample rate of the table, driven round robin, requests of one hop,
// and prints one JSON line per window.  Only the engines named are created (the others' contexts are absent from the process).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "lyra_batch_codec.h"
#include "lyra_device_decoder.h"
#include "lyra_mixed_decoder.h"

using namespace chromemedia::codec;

namespace {

constexpr int kRow = kMixedDecoderPacketRowBytes;

bool ReadRates(const char* path, std::vector<int>* out) {
  std::ifstream f(path);
  int rate;
  while (f >> rate) out->push_back(rate);
  return !out->empty();
}

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

double Seconds() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The streams of one sample rate behind one uniform decoder object (BatchLyraDecoder or DeviceLyraDecoder)
template <class Decoder>
struct RateClass {
  std::unique_ptr<Decoder> dec;
  int rate = 0;
  std::vector<int> members;                       // stream indices of the table
  std::vector<std::vector<int32_t>> received;     // [schedule hop]: members (local indices) that got a packet
  std::vector<std::vector<uint8_t>> packets;      // [schedule hop]: their packets, 15 bytes each
  std::vector<int16_t> out;
};

template <class Decoder>
bool RunClasses(std::vector<RateClass<Decoder>>& cls, int hops, int period) {
  auto begin = [&](int t) {
    for (auto& k : cls) {
      const int h = t % period;
      if (!k.received[h].empty() &&
          !k.dec->SetEncodedPackets(absl::MakeConstSpan(k.received[h]), absl::MakeConstSpan(k.packets[h])))
        return false;
      if (!k.dec->DecodeSamplesAsync(k.rate / 50)) return false;
    }
    return true;
  };
  if (!begin(0)) return false;
  for (int t = 0; t < hops; ++t) {
    if (t + 1 < hops && !begin(t + 1)) return false;
    for (auto& k : cls)
      if (!k.dec->WaitDecoded(absl::Span<int16_t>(k.out.data(), k.out.size()))) return false;
  }
  return true;
}

int Bench(int argc, char** argv) {
  if (argc != 6 && argc != 7) { std::fprintf(stderr, "usage: see mixed_decoder_demo.cc\n"); return 2; }
  const std::string list = argc == 7 ? argv[6] : "mixed,batch,device";
  const char* names[3] = {"mixed", "batch", "device"};
  bool use[3] = {false, false, false};
  for (size_t pos = 0; pos <= list.size();) {
    const size_t end = std::min(list.find(',', pos), list.size());
    const std::string name = list.substr(pos, end - pos);
    int e = 0;
    while (e < 3 && name != names[e]) ++e;
    if (e == 3) { std::fprintf(stderr, "unknown engine '%s'\n", name.c_str()); return 2; }
    use[e] = true;
    pos = end + 1;
  }
  const std::string model_dir = argv[2];
  std::vector<int> rates;
  if (!ReadRates(argv[3], &rates)) return 3;
  const int hops = std::atoi(argv[4]), windows = std::atoi(argv[5]);
  if (hops < 2 || windows < 1) return 3;
  const int n = static_cast<int>(rates.size());
  constexpr int kPeriod = 64, kBytes = 15;
  // the schedule: Gilbert loss per stream (good -> bad 1/18, bad -> good 1/2: 10 % lost, mean burst 2), random packet bytes
  std::vector<std::vector<uint8_t>> rows(kPeriod, std::vector<uint8_t>(static_cast<size_t>(n) * kRow, 0));
  std::vector<std::vector<int32_t>> lengths(kPeriod, std::vector<int32_t>(n, 0));
  {
    uint32_t x = 0x2545F491u;
    auto next = [&]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    std::vector<char> bad(n, 0);
    for (int h = 0; h < kPeriod; ++h)
      for (int s = 0; s < n; ++s) {
        bad[s] = bad[s] ? (next() % 2 == 0) : (next() % 18 == 0);
        if (bad[s]) continue;
        lengths[h][s] = kBytes;
        for (int j = 0; j < kBytes; ++j) rows[h][static_cast<size_t>(s) * kRow + j] = static_cast<uint8_t>(next());
      }
  }
  std::vector<int> keys;
  std::map<int, std::vector<int>> members;
  for (int s = 0; s < n; ++s) {
    if (!members.count(rates[s])) keys.push_back(rates[s]);
    members[rates[s]].push_back(s);
  }
  auto fill = [&](auto& cls) {
    for (auto& k : cls) {
      k.received.resize(kPeriod);
      k.packets.resize(kPeriod);
      k.out.resize(k.members.size() * static_cast<size_t>(k.rate / 50));
      for (int h = 0; h < kPeriod; ++h)
        for (size_t i = 0; i < k.members.size(); ++i) {
          const int s = k.members[i];
          if (lengths[h][s] == 0) continue;
          k.received[h].push_back(static_cast<int32_t>(i));
          k.packets[h].insert(k.packets[h].end(), rows[h].begin() + static_cast<size_t>(s) * kRow,
                              rows[h].begin() + static_cast<size_t>(s) * kRow + kBytes);
        }
    }
  };
  std::unique_ptr<MixedBatchLyraDecoder> mixed;
  if (use[0] && !(mixed = MixedBatchLyraDecoder::Create(absl::MakeConstSpan(rates), 1, model_dir))) return 1;
  std::vector<RateClass<BatchLyraDecoder>> batch;
  std::vector<RateClass<DeviceLyraDecoder>> device;
  for (int rate : keys) {
    const int count = static_cast<int>(members[rate].size());
    if (use[1]) {
      batch.emplace_back();
      batch.back().rate = rate;
      batch.back().members = members[rate];
      if (!(batch.back().dec = BatchLyraDecoder::Create(rate, 1, model_dir, count))) return 1;
    }
    if (use[2]) {
      device.emplace_back();
      device.back().rate = rate;
      device.back().members = members[rate];
      if (!(device.back().dec = DeviceLyraDecoder::Create(rate, 1, model_dir, count))) return 1;
    }
  }
  fill(batch);
  fill(device);
  std::vector<int16_t> out(use[0] ? mixed->hop_samples() : 0);
  auto run_mixed = [&]() {
    auto begin = [&](int t) {
      const int h = t % kPeriod;
      return mixed->SetEncodedPackets(absl::MakeConstSpan(rows[h]), absl::MakeConstSpan(lengths[h])) && mixed->DecodeHopAsync();
    };
    if (!begin(0)) return false;
    for (int t = 0; t < hops; ++t) {
      if (t + 1 < hops && !begin(t + 1)) return false;
      if (!mixed->WaitDecoded(absl::Span<int16_t>(out.data(), out.size()))) return false;
    }
    return true;
  };
  auto run = [&](int engine) {
    return engine == 0 ? run_mixed() : engine == 1 ? RunClasses(batch, hops, kPeriod) : RunClasses(device, hops, kPeriod);
  };
  for (int engine = 0; engine < 3; ++engine)
    if (use[engine] && !run(engine)) return 4;   // warm-up: allocations, code objects
  for (int w = 0; w < windows; ++w)
    for (int engine = 0; engine < 3; ++engine) {
      if (!use[engine]) continue;
      const double t0 = Seconds();
      if (!run(engine)) return 4;
      const double dt = Seconds() - t0;
      std::printf("{\"engine\": \"%s\", \"streams\": %d, \"rates\": %zu, \"hops\": %d, \"window\": %d, \"seconds\": %.6f, "
                  "\"frames_per_s\": %.1f}\n", names[engine], n, keys.size(), hops, w, dt, static_cast<double>(n) * hops / dt);
      std::fflush(stdout);
    }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--bench") == 0) return Bench(argc, argv);
  if (argc != 7) { std::fprintf(stderr, "usage: see mixed_decoder_demo.cc\n"); return 2; }
  const char* e = std::getenv("LYRA_DEMO_PIPELINED");
  const int mode = e ? std::atoi(e) : 0;
  if (mode < 0 || mode > 1) { std::fprintf(stderr, "LYRA_DEMO_PIPELINED must be 0 or 1\n"); return 2; }
  std::vector<int> rates;
  if (!ReadRates(argv[2], &rates)) return 3;
  std::vector<uint8_t> packets;
  std::vector<int32_t> lengths;
  if (!ReadFile(argv[3], &packets) || !ReadFile(argv[4], &lengths)) return 3;
  auto dec = MixedBatchLyraDecoder::Create(absl::MakeConstSpan(rates), 1, argv[1]);
  if (!dec) { std::fprintf(stderr, "creation failed\n"); return 1; }
  const size_t n = static_cast<size_t>(dec->num_streams());
  if (lengths.size() % n != 0 || packets.size() != lengths.size() * kRow) return 3;
  const int hops = static_cast<int>(lengths.size() / n);
  std::ofstream pcm_out(argv[5], std::ios::binary), flags_out(argv[6], std::ios::binary);
  auto stage = [&](int t) {
    return dec->SetEncodedPackets(absl::MakeConstSpan(packets.data() + static_cast<size_t>(t) * n * kRow, n * kRow),
                                  absl::MakeConstSpan(lengths.data() + static_cast<size_t>(t) * n, n));
  };
  auto write = [&](const std::vector<int16_t>& pcm) {
    pcm_out.write(reinterpret_cast<const char*>(pcm.data()), pcm.size() * 2);
    for (size_t s = 0; s < n; ++s) {
      const int32_t flag = dec->is_comfort_noise(static_cast<int>(s)) ? 1 : 0;
      flags_out.write(reinterpret_cast<const char*>(&flag), 4);
    }
  };
  if (mode == 1) {
    std::vector<int16_t> pcm(dec->hop_samples());
    if (hops > 0 && !(stage(0) && dec->DecodeHopAsync())) return 4;
    for (int t = 0; t < hops; ++t) {
      if (t + 1 < hops && !(stage(t + 1) && dec->DecodeHopAsync())) return 4;
      if (dec->hops_in_flight() != (t + 1 < hops ? 2 : 1)) return 7;
      if (!dec->WaitDecoded(absl::Span<int16_t>(pcm.data(), pcm.size()))) return 4;
      write(pcm);
    }
    return 0;
  }
  for (int t = 0; t < hops; ++t) {
    if (!stage(t)) return 4;
    auto pcm = dec->DecodeHop();
    if (!pcm) return 4;
    write(*pcm);
  }
  return 0;
}
