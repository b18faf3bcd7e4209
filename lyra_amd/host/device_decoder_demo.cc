// device_decoder_demo.cc -- decoder_demo's scripted session (same arguments, same script format, same three output files)
// with DeviceLyraDecoder (lyra_device_decoder.h) in BatchLyraDecoder's place:
//   device_decoder_demo <model_dir> <script.txt> <pcm_in.s16> <sample_rate> <bitrate> <dtx 0|1> <num_streams>
//                       <packets_out.bin> <lengths_out.i32> <pcm_out.s16>
// LYRA_DEMO_PIPELINED=1: DecodeSamplesAsync(request k + 1) is issued before WaitDecoded(k).  A request the decoder refuses
// (outside its size rule) ends the program with exit code 6, as a failed DecodeSamples ends decoder_demo.
// LYRA_DEMO_ANY_SIZE=1: AnySizeDeviceLyraDecoder (lyra_device_decoder_any.h) instead: requests of any size up to four hops.
// LYRA_DEMO_MIXED_ANY_SIZE=1: another program altogether,
//   device_decoder_demo <model_dir> <pcm_in.s16> <num_streams> <hops>
// <pcm_in.s16> holds [hops][num_streams][320] samples at 16 kHz.  Stream s decodes at 8 / 16 / 32 / 48 kHz (s % 4) under its
// back end's callback of 160 / 256 / 441 / 1024 frames.  ONE MixedAnySizeDeviceLyraDecoder (lyra_mixed_device_decoder.h) serves
// all of them, one request per round of callbacks; one AnySizeDeviceLyraDecoder per (rate, size) class gets the same packets
// and the same requests (each with all <num_streams> slots, of which it uses its class's: a stream keeps its number, which
// seeds its comfort noise).  Every sample, is_comfort_noise() and leftover_samples() are compared: exit code 8 on a difference,
// else "mixed any-size: <n> samples equal".
//
//   device_decoder_demo --bench <model_dir> <sample_rate> <num_streams> <hops> <loss_percent> <reps>
// times one session -- 10 ms requests, a packet every second request, two-state (Gilbert) loss with mean burst 2, host
// buffers -- through BatchLyraDecoder and through DeviceLyraDecoder, blocking and pipelined, the four forms alternated
// `reps` times after one untimed pass of each; one JSON line with the median and the min..max of decoded hops per second.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <memory>
#include <optional>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "lyra_batch_codec.h"
#include "lyra_device_decoder.h"
#include "lyra_device_decoder_any.h"
#include "lyra_mixed_device_decoder.h"

using namespace chromemedia::codec;

namespace {

// packets [hops][n][ps], received [hops][n]; every hop: the received packets, then two requests of 10 ms
template <class Dec>
bool Session(Dec* dec, int n, int ps, int n10, int hops, const std::vector<uint8_t>& packets, const std::vector<uint8_t>& received,
             bool pipelined, std::vector<int16_t>* out) {
  std::vector<int32_t> ids;
  std::vector<uint8_t> delivered;
  int waiting = 0;
  absl::Span<int16_t> span(out->data(), out->size());
  for (int t = 0; t < hops; ++t) {
    ids.clear();
    delivered.clear();
    for (int s = 0; s < n; ++s)
      if (received[(size_t)t * n + s]) {
        ids.push_back(s);
        const uint8_t* p = packets.data() + ((size_t)t * n + s) * ps;
        delivered.insert(delivered.end(), p, p + ps);
      }
    if (!ids.empty() && !dec->SetEncodedPackets(absl::MakeConstSpan(ids), absl::MakeConstSpan(delivered))) return false;
    for (int k = 0; k < 2; ++k) {
      if (!pipelined) {
        if (!dec->DecodeSamples(n10, span)) return false;
        continue;
      }
      if (waiting == 2) { if (!dec->WaitDecoded(span)) return false; --waiting; }
      if (!dec->DecodeSamplesAsync(n10)) return false;
      ++waiting;
    }
  }
  for (; waiting > 0; --waiting)
    if (!dec->WaitDecoded(span)) return false;
  return true;
}

int Bench(int argc, char** argv) {
  if (argc != 8) { std::fprintf(stderr, "usage: see device_decoder_demo.cc\n"); return 2; }
  const std::string model_dir = argv[2];
  const int rate = std::atoi(argv[3]), n = std::atoi(argv[4]), hops = std::atoi(argv[5]), reps = std::atoi(argv[7]);
  const double loss = std::atof(argv[6]) / 100.0;
  const int hop = rate / 50, ps = 15;
  std::mt19937 rng(5);
  std::vector<uint8_t> packets((size_t)hops * n * ps), received((size_t)hops * n, 1);
  {   // packets of a real encoder over a tone + noise; the decoder's work does not depend on what they say
    auto enc = BatchLyraEncoder::Create(rate, 1, 6000, false, model_dir, n);
    if (!enc) return 1;
    std::vector<int16_t> pcm((size_t)n * hop);
    for (int t = 0; t < hops; ++t) {
      for (auto& v : pcm) v = (int16_t)((int)(rng() % 4001) - 2000);
      auto p = enc->Encode(absl::MakeConstSpan(pcm));
      if (!p || (int)p->size() != n * ps) return 4;
      std::memcpy(packets.data() + (size_t)t * n * ps, p->data(), p->size());
    }
  }
  if (loss > 0) {
    std::uniform_real_distribution<double> u(0, 1);
    const double p_lost = loss / (2.0 * (1.0 - loss)), p_back = 0.5;
    for (int s = 0; s < n; ++s) {
      bool rx = true;
      for (int t = 0; t < hops; ++t) {
        received[(size_t)t * n + s] = rx;
        rx = rx ? u(rng) >= p_lost : u(rng) < p_back;
      }
    }
  }
  auto batch = BatchLyraDecoder::Create(rate, 1, model_dir, n);
  auto device = DeviceLyraDecoder::Create(rate, 1, model_dir, n);
  if (!batch || !device) return 1;
  std::vector<int16_t> out((size_t)n * (hop / 2));
  const char* names[4] = {"batch_blocking", "batch_pipelined", "device_blocking", "device_pipelined"};
  std::vector<double> fps[4];
  for (int rep = 0; rep <= reps; ++rep)   // pass 0 warms every form up and is not counted
    for (int f = 0; f < 4; ++f) {
      const auto t0 = std::chrono::steady_clock::now();
      const bool ok = f < 2 ? Session(batch.get(), n, ps, hop / 2, hops, packets, received, f == 1, &out)
                            : Session(device.get(), n, ps, hop / 2, hops, packets, received, f == 3, &out);
      const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (!ok) return 6;
      if (rep) fps[f].push_back((double)n * hops / dt);
    }
  std::printf("{\"bench\": \"decode_samples_host\", \"streams\": %d, \"rate\": %d, \"loss\": %.2f, \"hops\": %d, \"reps\": %d", n, rate,
              loss, hops, reps);
  for (int f = 0; f < 4; ++f) {
    std::sort(fps[f].begin(), fps[f].end());
    std::printf(", \"%s\": {\"frames_per_s_median\": %.0f, \"min\": %.0f, \"max\": %.0f}", names[f], fps[f][fps[f].size() / 2],
                fps[f].front(), fps[f].back());
  }
  std::printf("}\n");
  return 0;
}

// The same session under an audio back end's callback of `cb` frames (any size up to four hops): every hop the received
// packets, then the callbacks whose samples the packets handed over so far cover.  A hop without a callback is followed by a
// second packet for its streams, which cannot overtake requests in flight: the pipelined form drains first.
template <class Dec>
bool CallbackSession(Dec* dec, int n, int ps, int hop, int cb, int hops, const std::vector<uint8_t>& packets,
                     const std::vector<uint8_t>& received, bool pipelined, std::vector<int16_t>* out) {
  std::vector<int32_t> ids;
  std::vector<uint8_t> delivered;
  int waiting = 0;
  long played = 0;
  bool idle_hop = false;
  absl::Span<int16_t> span(out->data(), (size_t)n * cb);
  for (int t = 0; t < hops; ++t) {
    ids.clear();
    delivered.clear();
    for (int s = 0; s < n; ++s)
      if (received[(size_t)t * n + s]) {
        ids.push_back(s);
        const uint8_t* p = packets.data() + ((size_t)t * n + s) * ps;
        delivered.insert(delivered.end(), p, p + ps);
      }
    if (idle_hop)
      for (; waiting > 0; --waiting)
        if (!dec->WaitDecoded(span)) return false;
    if (!ids.empty() && !dec->SetEncodedPackets(absl::MakeConstSpan(ids), absl::MakeConstSpan(delivered))) return false;
    idle_hop = true;
    while (played + cb <= (long)(t + 1) * hop) {
      played += cb;
      idle_hop = false;
      if (!pipelined) {
        if (!dec->DecodeSamples(cb, span)) return false;
        continue;
      }
      if (waiting == 2) { if (!dec->WaitDecoded(span)) return false; --waiting; }
      if (!dec->DecodeSamplesAsync(cb)) return false;
      ++waiting;
    }
  }
  for (; waiting > 0; --waiting)
    if (!dec->WaitDecoded(span)) return false;
  return true;
}

//   device_decoder_demo --bench-any <model_dir> <sample_rate> <num_streams> <hops> <loss_percent> <reps> <callback_frames>
// Bench's session and loss model under callbacks of <callback_frames>, through BatchLyraDecoder and AnySizeDeviceLyraDecoder.
int BenchAny(int argc, char** argv) {
  if (argc != 9) { std::fprintf(stderr, "usage: see device_decoder_demo.cc\n"); return 2; }
  const std::string model_dir = argv[2];
  const int rate = std::atoi(argv[3]), n = std::atoi(argv[4]), hops = std::atoi(argv[5]), reps = std::atoi(argv[7]);
  const int cb = std::atoi(argv[8]);
  const double loss = std::atof(argv[6]) / 100.0;
  const int hop = rate / 50, ps = 15;
  if (cb <= 0 || cb > 4 * hop) return 2;
  std::mt19937 rng(5);
  std::vector<uint8_t> packets((size_t)hops * n * ps), received((size_t)hops * n, 1);
  {
    auto enc = BatchLyraEncoder::Create(rate, 1, 6000, false, model_dir, n);
    if (!enc) return 1;
    std::vector<int16_t> pcm((size_t)n * hop);
    for (int t = 0; t < hops; ++t) {
      for (auto& v : pcm) v = (int16_t)((int)(rng() % 4001) - 2000);
      auto p = enc->Encode(absl::MakeConstSpan(pcm));
      if (!p || (int)p->size() != n * ps) return 4;
      std::memcpy(packets.data() + (size_t)t * n * ps, p->data(), p->size());
    }
  }
  if (loss > 0) {
    std::uniform_real_distribution<double> u(0, 1);
    const double p_lost = loss / (2.0 * (1.0 - loss)), p_back = 0.5;
    for (int s = 0; s < n; ++s) {
      bool rx = true;
      for (int t = 0; t < hops; ++t) {
        received[(size_t)t * n + s] = rx;
        rx = rx ? u(rng) >= p_lost : u(rng) < p_back;
      }
    }
  }
  // The receiver's jitter buffer: callbacks that do not line up with the hops let every loss episode leave part of a
  // concealed hop in front of the next packet, so the decoder's queue grows (the reference's does, without bound); a packet
  // that would be the fourth to wait is dropped as late.  Decided here, on the shared plan functions, so that both decoders
  // get the same script -- each object runs its blocking and its pipelined session of every pass, 2 * (reps + 1) in a row.
  long late = 0;
  const int sessions = 2 * (reps + 1);
  std::vector<uint8_t> script((size_t)sessions * hops * n);
  for (int s = 0; s < n; ++s) {
    lyra::DsState st = {0, 0, 0, 0, 0, 0, 0};
    int left = 0;
    for (int rep = 0; rep < sessions; ++rep) {
      long played = 0;
      for (int t = 0; t < hops; ++t) {
        bool rx = received[(size_t)t * n + s] != 0;
        if (rx && st.wait >= lyra::DS_FIFO_DEPTH - 1) { rx = false; ++late; }
        script[((size_t)rep * hops + t) * n + s] = rx;
        bool first = true;
        for (; played + cb <= (long)(t + 1) * hop; played += cb, first = false) {
          const lyra::DsaStep step = lyra::ds_any_step(left, cb, rate);
          left = step.left;
          for (int r = 0, R = lyra::ds_any_rounds(cb, rate); r < R; ++r)
            st = lyra::ds_plan(st, rx && first && r == 0, lyra::ds_any_round_total(step.n_int, r)).s;
        }
        if (first) st = lyra::ds_plan(st, rx, 0).s;   // (no callback in this hop: the packet waits)
      }
    }
  }
  auto batch = BatchLyraDecoder::Create(rate, 1, model_dir, n);
  auto device = AnySizeDeviceLyraDecoder::Create(rate, 1, model_dir, n);
  if (!batch || !device) return 1;
  std::vector<int16_t> out((size_t)n * cb);
  const char* names[4] = {"batch_blocking", "batch_pipelined", "any_size_blocking", "any_size_pipelined"};
  std::vector<double> fps[4];
  for (int rep = 0; rep <= reps; ++rep)   // pass 0 warms every form up and is not counted
    for (int f = 0; f < 4; ++f) {
      const auto t0 = std::chrono::steady_clock::now();
      const size_t sess = (size_t)rep * 2 + (f & 1);
      received.assign(script.begin() + sess * hops * n, script.begin() + (sess + 1) * hops * n);
      const bool ok = f < 2 ? CallbackSession(batch.get(), n, ps, hop, cb, hops, packets, received, f == 1, &out)
                            : CallbackSession(device.get(), n, ps, hop, cb, hops, packets, received, f == 3, &out);
      const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (!ok) return 6;
      if (rep) fps[f].push_back((double)n * hops / dt);
    }
  std::printf("{\"bench\": \"decode_samples_any_host\", \"streams\": %d, \"rate\": %d, \"callback\": %d, \"loss\": %.2f, \"hops\": %d, "
              "\"reps\": %d, \"late_packets_dropped\": %ld", n, rate, cb, loss, hops, reps, late);
  for (int f = 0; f < 4; ++f) {
    std::sort(fps[f].begin(), fps[f].end());
    std::printf(", \"%s\": {\"frames_per_s_median\": %.0f, \"min\": %.0f, \"max\": %.0f}", names[f], fps[f][fps[f].size() / 2],
                fps[f].front(), fps[f].back());
  }
  std::printf("}\n");
  return 0;
}

template <class Dec>
int Script(char** argv) {
  const std::string model_dir = argv[1];
  const int rate = std::atoi(argv[4]), bitrate = std::atoi(argv[5]), dtx = std::atoi(argv[6]), n = std::atoi(argv[7]);
  std::ifstream script(argv[2]);
  std::ifstream in(argv[3], std::ios::binary);
  std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  std::vector<int16_t> pcm(raw.size() / 2);
  std::memcpy(pcm.data(), raw.data(), pcm.size() * 2);
  auto enc = BatchLyraEncoder::Create(rate, 1, bitrate, dtx != 0, model_dir, n);
  auto dec = Dec::Create(rate, 1, model_dir, n);
  if (!enc || !dec) { std::fprintf(stderr, "creation failed\n"); return 1; }
  std::ofstream pk_out(argv[8], std::ios::binary), len_out(argv[9], std::ios::binary), pcm_out(argv[10], std::ios::binary);
  const char* e = std::getenv("LYRA_DEMO_PIPELINED");
  const bool pipelined = e && std::atoi(e) != 0;
  const size_t frame = static_cast<size_t>(n) * (rate / 50);
  std::vector<int> waiting;   // sizes of the requests begun and not yet delivered (at most two)
  auto deliver_oldest = [&]() {
    std::vector<int16_t> out(static_cast<size_t>(n) * waiting.front());
    if (!dec->WaitDecoded(absl::Span<int16_t>(out.data(), out.size()))) return false;
    pcm_out.write(reinterpret_cast<const char*>(out.data()), out.size() * 2);
    waiting.erase(waiting.begin());
    return true;
  };
  std::string line;
  size_t off = 0;
  while (std::getline(script, line)) {
    if (line.empty()) continue;
    std::istringstream ls(line);
    std::string mask;
    ls >> mask;
    if (static_cast<int>(mask.size()) != n || off + frame > pcm.size()) return 3;
    auto packets = enc->Encode(absl::MakeConstSpan(pcm.data() + off, frame));
    off += frame;
    if (!packets) return 4;
    pk_out.write(reinterpret_cast<const char*>(packets->data()), packets->size());
    len_out.write(reinterpret_cast<const char*>(enc->packet_lengths().data()), n * 4);
    std::vector<int32_t> ids;
    std::vector<uint8_t> delivered;
    const int ps = enc->packet_size();
    for (int s = 0; s < n; ++s)
      if (mask[s] == '1' && enc->packet_lengths()[s] > 0) {
        ids.push_back(s);
        delivered.insert(delivered.end(), packets->begin() + s * ps, packets->begin() + (s + 1) * ps);
      }
    if (!ids.empty() && !dec->SetEncodedPackets(absl::MakeConstSpan(ids), absl::MakeConstSpan(delivered))) return 5;
    int k;
    while (ls >> k) {
      if (pipelined) {
        if (waiting.size() == 2 && !deliver_oldest()) return 6;
        if (!dec->DecodeSamplesAsync(k)) return 6;
        waiting.push_back(k);
        if (dec->requests_in_flight() != static_cast<int>(waiting.size())) return 7;
      } else {
        auto out = dec->DecodeSamples(k);
        if (!out || out->size() != static_cast<size_t>(n) * k) return 6;
        pcm_out.write(reinterpret_cast<const char*>(out->data()), out->size() * 2);
      }
    }
  }
  while (!waiting.empty())
    if (!deliver_oldest()) return 6;
  return 0;
}

int MixedAnySize(int argc, char** argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: see device_decoder_demo.cc\n"); return 2; }
  const std::string model_dir = argv[1];
  const int n = std::atoi(argv[3]), hops = std::atoi(argv[4]);
  static const int kRate[4] = {8000, 16000, 32000, 48000}, kCallback[4] = {160, 256, 441, 1024};
  if (n < 4 || n % 4 != 0 || hops < 1) return 2;
  std::ifstream in(argv[2], std::ios::binary);
  std::vector<char> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  std::vector<int16_t> pcm(raw.size() / 2);
  std::memcpy(pcm.data(), raw.data(), pcm.size() * 2);
  if (pcm.size() < (size_t)hops * n * 320) return 3;
  std::vector<int> rates(n);
  for (int s = 0; s < n; ++s) rates[s] = kRate[s % 4];
  auto enc = BatchLyraEncoder::Create(16000, 1, 6000, false, model_dir, n);
  auto mixed = MixedAnySizeDeviceLyraDecoder::Create(absl::MakeConstSpan(rates), model_dir);
  std::unique_ptr<AnySizeDeviceLyraDecoder> uniform[4];
  for (int c = 0; c < 4; ++c) uniform[c] = AnySizeDeviceLyraDecoder::Create(kRate[c], 1, model_dir, n);
  if (!enc || !mixed || !uniform[0] || !uniform[1] || !uniform[2] || !uniform[3]) { std::fprintf(stderr, "creation failed\n"); return 1; }
  long played[4] = {0, 0, 0, 0}, compared = 0, requests = 0;
  for (int t = 0; t < hops; ++t) {
    auto packets = enc->Encode(absl::MakeConstSpan(pcm.data() + (size_t)t * n * 320, (size_t)n * 320));
    if (!packets) return 4;
    const int ps = enc->packet_size();
    // stream 1 loses hops 4 .. 15 (into comfort noise and back), the others a hop now and then
    std::vector<int32_t> ids, class_ids[4];
    std::vector<uint8_t> delivered, class_delivered[4];
    for (int s = 0; s < n; ++s) {
      const bool lost = s == 1 ? (t >= 4 && t < 16) : (t * 7 + s * 3) % 10 == 0;
      if (lost) continue;
      ids.push_back(s);
      class_ids[s % 4].push_back(s);
      delivered.insert(delivered.end(), packets->begin() + s * ps, packets->begin() + (s + 1) * ps);
      class_delivered[s % 4].insert(class_delivered[s % 4].end(), packets->begin() + s * ps, packets->begin() + (s + 1) * ps);
    }
    if (!ids.empty() && !mixed->SetEncodedPackets(absl::MakeConstSpan(ids), absl::MakeConstSpan(delivered))) return 5;
    for (int c = 0; c < 4; ++c)
      if (!class_ids[c].empty() &&
          !uniform[c]->SetEncodedPackets(absl::MakeConstSpan(class_ids[c]), absl::MakeConstSpan(class_delivered[c])))
        return 5;
    for (;;) {   // rounds of callbacks: every class whose next callback fits into the playout time of the packets so far
      bool due[4];
      std::vector<int32_t> streams;
      std::vector<int> sizes;
      for (int c = 0; c < 4; ++c) due[c] = played[c] + kCallback[c] <= (long)(t + 1) * (kRate[c] / 50);
      for (int s = 0; s < n; ++s)
        if (due[s % 4]) { streams.push_back(s); sizes.push_back(kCallback[s % 4]); }
      if (streams.empty()) break;
      auto got = mixed->DecodeSamples(absl::MakeConstSpan(streams), absl::MakeConstSpan(sizes));
      if (!got) return 6;
      ++requests;
      std::optional<std::vector<int16_t>> want[4];
      for (int c = 0; c < 4; ++c)
        if (due[c]) {
          want[c] = uniform[c]->DecodeSamples(kCallback[c]);
          if (!want[c]) return 6;
          played[c] += kCallback[c];
        }
      size_t at = 0;
      for (int32_t s : streams) {
        const int c = s % 4, cb = kCallback[c];
        if (std::memcmp(got->data() + at, want[c]->data() + (size_t)s * cb, (size_t)cb * 2) != 0) {
          std::fprintf(stderr, "hop %d, stream %d (%d Hz, %d frames): samples differ\n", t, s, kRate[c], cb);
          return 8;
        }
        at += cb;
        compared += cb;
      }
      for (int s = 0; s < n; ++s)
        if (mixed->is_comfort_noise(s) != uniform[s % 4]->is_comfort_noise(s) ||
            mixed->leftover_samples(s) != uniform[s % 4]->leftover_samples(s)) {
          std::fprintf(stderr, "hop %d, stream %d: is_comfort_noise or leftover_samples differ\n", t, s);
          return 8;
        }
    }
  }
  std::printf("mixed any-size: %ld samples equal in %ld requests, %d streams, %d hops\n", compared, requests, n, hops);
  return compared > 0 ? 0 : 8;
}

}  // namespace

int main(int argc, char** argv) {
  { const char* mixed = std::getenv("LYRA_DEMO_MIXED_ANY_SIZE");
    if (mixed && std::atoi(mixed) != 0) return MixedAnySize(argc, argv); }
  if (argc > 1 && std::strcmp(argv[1], "--bench") == 0) return Bench(argc, argv);
  if (argc > 1 && std::strcmp(argv[1], "--bench-any") == 0) return BenchAny(argc, argv);
  if (argc != 11) { std::fprintf(stderr, "usage: see device_decoder_demo.cc\n"); return 2; }
  const char* any = std::getenv("LYRA_DEMO_ANY_SIZE");
  return any && std::atoi(any) != 0 ? Script<AnySizeDeviceLyraDecoder>(argv) : Script<DeviceLyraDecoder>(argv);
}
