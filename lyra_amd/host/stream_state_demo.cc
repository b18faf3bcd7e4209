// stream_state_demo.cc -- moves live streams between objects of the public classes and checks that they go on as streams
// that never moved (tests/test_gpu_stream_state.py):   stream_state_demo <model_dir> <sample_rate>
//  1. three DeviceLyraDecoder objects: `stay` and `from` run the same session (10 ms requests, a packet every second request,
//     scripted loss with bursts long enough for comfort noise); mid-session every stream of `from` is exported and imported
//     into `to` under a permuted index; `stay` and `to` continue on the same inputs and must deliver the same samples.  Then
//     a sequence whose outcome depends on the host mirror ImportStream rebuilt: a second packet before the next request,
//     then packets until the FIFO is full -- the same calls must succeed and be refused on both, and the audio stay equal.
//  2. the same with three BatchLyraEncoder objects with DTX: packets and packet lengths.
//  3. refusals: a blob of the other class, of another rate, a truncated one, and calls with requests / hops in flight.
// Prints one line per part; exit code 0 only if every comparison held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "lyra_batch_codec.h"
#include "lyra_device_decoder.h"

using namespace chromemedia::codec;

namespace {
constexpr int N = 6, PS = 15;
const int kPerm[N] = {4, 2, 5, 0, 3, 1};
#define CHECK_OR(cond, code) do { if (!(cond)) { std::fprintf(stderr, "stream_state_demo: %s (line %d)\n", #cond, __LINE__); return code; } } while (0)

bool Lost(int t, int s) {   // s 0: a 14-hop burst (comfort noise at the move), s 1: 5 hops (mid-fade), others: scattered
  if (s == 0) return t >= 16 && t < 30;
  if (s == 1) return (t >= 25 && t < 30) || t % 11 == 3;
  return (t * 7 + s * 13) % 10 == 0 || (s == 4 && t % 17 >= 14);
}

void Audio(std::mt19937* rng, int t, int hop, std::vector<int16_t>* pcm) {   // tone bursts over faint noise: DTX sees both
  for (int s = 0; s < N; ++s)
    for (int i = 0; i < hop; ++i) {
      const bool loud = ((t + 3 * s) / 9) % 2 == 0;
      const int tone = loud ? (int)(6000.0 * std::sin(0.05 * (s + 1) * (t * hop + i))) : 0;
      (*pcm)[(size_t)s * hop + i] = (int16_t)(tone + (int)((*rng)() % 61) - 30);
    }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: stream_state_demo <model_dir> <sample_rate>\n"); return 2; }
  const std::string model = argv[1];
  const int rate = std::atoi(argv[2]), hop = rate / 50, n10 = rate / 100, T1 = 30, T2 = 40;
  std::mt19937 rng(11);
  // ---- packets of a real encoder ----
  std::vector<uint8_t> packets((size_t)(T1 + T2 + 8) * N * PS);
  std::vector<int16_t> pcm((size_t)N * hop);
  {
    auto enc = BatchLyraEncoder::Create(rate, 1, 6000, false, model, N);
    CHECK_OR(enc, 1);
    for (int t = 0; t < T1 + T2 + 8; ++t) {
      Audio(&rng, t, hop, &pcm);
      auto p = enc->Encode(absl::MakeConstSpan(pcm));
      CHECK_OR(p && (int)p->size() == N * PS, 1);
      std::memcpy(packets.data() + (size_t)t * N * PS, p->data(), p->size());
    }
  }
  // ---- 1. decoders ----
  auto stay = DeviceLyraDecoder::Create(rate, 1, model, N);
  auto from = DeviceLyraDecoder::Create(rate, 1, model, N);
  auto to = DeviceLyraDecoder::Create(rate, 1, model, N + 3);
  CHECK_OR(stay && from && to, 1);
  std::vector<int16_t> a((size_t)N * n10), b((size_t)(N + 3) * n10);
  auto feed = [&](DeviceLyraDecoder* d, int t, bool permuted) {
    std::vector<int32_t> ids;
    std::vector<uint8_t> del;
    for (int s = 0; s < N; ++s)
      if (!Lost(t, s)) {
        ids.push_back(permuted ? kPerm[s] : s);
        const uint8_t* p = packets.data() + ((size_t)t * N + s) * PS;
        del.insert(del.end(), p, p + PS);
      }
    return ids.empty() || d->SetEncodedPackets(absl::MakeConstSpan(ids), absl::MakeConstSpan(del));
  };
  auto same_rows = [&]() {
    for (int s = 0; s < N; ++s)
      if (std::memcmp(a.data() + (size_t)s * n10, b.data() + (size_t)kPerm[s] * n10, (size_t)n10 * 2) != 0) return false;
    return true;
  };
  for (int t = 0; t < T1; ++t) {
    CHECK_OR(feed(stay.get(), t, false) && feed(from.get(), t, false), 3);
    for (int k = 0; k < 2; ++k) {
      if (t == T1 - 1 && k == 1) break;   // the move comes in the middle of a hop
      CHECK_OR(stay->DecodeSamples(n10, absl::Span<int16_t>(a.data(), a.size())), 3);
      CHECK_OR(from->DecodeSamples(n10, absl::Span<int16_t>(a.data(), a.size())), 3);
    }
  }
  CHECK_OR(stay->is_comfort_noise(0) && !stay->is_comfort_noise(2), 3);
  CHECK_OR(feed(stay.get(), T1, false) && feed(from.get(), T1, false), 3);   // staged packets travel with the stream
  for (int s = 0; s < N; ++s) {
    auto blob = from->ExportStream(s);
    CHECK_OR(blob, 4);
    CHECK_OR(to->ImportStream(kPerm[s], absl::MakeConstSpan(*blob)), 4);
    CHECK_OR(to->is_comfort_noise(kPerm[s]) == stay->is_comfort_noise(s), 4);
  }
  CHECK_OR(stay->DecodeSamples(n10, absl::Span<int16_t>(a.data(), a.size())) && to->DecodeSamples(n10, absl::Span<int16_t>(b.data(), b.size())) && same_rows(), 5);
  for (int t = T1; t < T1 + T2; ++t) {
    if (t > T1) CHECK_OR(feed(stay.get(), t, false) && feed(to.get(), t, true), 5);
    for (int k = 0; k < 2; ++k) {
      CHECK_OR(stay->DecodeSamples(n10, absl::Span<int16_t>(a.data(), a.size())) && to->DecodeSamples(n10, absl::Span<int16_t>(b.data(), b.size())), 5);
      CHECK_OR(same_rows(), 5);
    }
  }
  std::printf("decoders: %d streams moved mid-session, %d hops equal afterwards\n", N, T2);
  {   // the host mirror: packets for stream 3 until both refuse, which must happen at the same packet
    int accepted_a = 0, accepted_b = 0;
    for (int k = 0; k < 8; ++k) {
      const int32_t ia = 3, ib = kPerm[3];
      const uint8_t* p = packets.data() + ((size_t)(T1 + T2 + k) * N + 3) * PS;
      const bool ra = stay->SetEncodedPackets(absl::MakeConstSpan(&ia, 1), absl::MakeConstSpan(p, PS));
      const bool rb = to->SetEncodedPackets(absl::MakeConstSpan(&ib, 1), absl::MakeConstSpan(p, PS));
      CHECK_OR(ra == rb, 6);
      accepted_a += ra; accepted_b += rb;
    }
    CHECK_OR(accepted_a == accepted_b && accepted_a >= 2 && accepted_a <= LYRA_HIP_DECODE_SAMPLES_FIFO, 6);
    for (int k = 0; k < 2 * (LYRA_HIP_DECODE_SAMPLES_FIFO + 2); ++k) {
      CHECK_OR(stay->DecodeSamples(n10, absl::Span<int16_t>(a.data(), a.size())) && to->DecodeSamples(n10, absl::Span<int16_t>(b.data(), b.size())) && same_rows(), 6);
    }
    std::printf("host mirror: %d packets accepted before the full FIFO refused one, on both\n", accepted_a);
  }
  // ---- 2. encoders with DTX ----
  auto estay = BatchLyraEncoder::Create(rate, 1, 6000, true, model, N);
  auto efrom = BatchLyraEncoder::Create(rate, 1, 6000, true, model, N);
  auto eto = BatchLyraEncoder::Create(rate, 1, 6000, true, model, N);
  CHECK_OR(estay && efrom && eto, 1);
  std::vector<int16_t> perm_pcm((size_t)N * hop);
  int empty = 0, full = 0;
  for (int t = 0; t < T1 + T2; ++t) {
    Audio(&rng, t, hop, &pcm);
    auto pa = estay->Encode(absl::MakeConstSpan(pcm));
    CHECK_OR(pa, 7);
    if (t < T1) {
      CHECK_OR(efrom->Encode(absl::MakeConstSpan(pcm)), 7);
      if (t == T1 - 1)
        for (int s = 0; s < N; ++s) {
          auto blob = efrom->ExportStream(s);
          CHECK_OR(blob && eto->ImportStream(kPerm[s], absl::MakeConstSpan(*blob)), 7);
        }
      continue;
    }
    for (int s = 0; s < N; ++s) std::memcpy(perm_pcm.data() + (size_t)kPerm[s] * hop, pcm.data() + (size_t)s * hop, (size_t)hop * 2);
    auto pb = eto->Encode(absl::MakeConstSpan(perm_pcm));
    CHECK_OR(pb, 7);
    for (int s = 0; s < N; ++s) {
      CHECK_OR(estay->packet_lengths()[s] == eto->packet_lengths()[kPerm[s]], 8);
      CHECK_OR(std::memcmp(pa->data() + (size_t)s * PS, pb->data() + (size_t)kPerm[s] * PS, PS) == 0, 8);
      (estay->packet_lengths()[s] ? full : empty)++;
    }
  }
  CHECK_OR(empty > 10 && full > 10, 8);
  std::printf("encoders: %d streams moved, %d packets and %d empty packets equal afterwards\n", N, full, empty);
  // ---- 3. refusals ----
  auto eblob = estay->ExportStream(0);
  auto dblob = stay->ExportStream(0);
  CHECK_OR(eblob && dblob, 9);
  CHECK_OR(!to->ImportStream(0, absl::MakeConstSpan(*eblob)) && !eto->ImportStream(0, absl::MakeConstSpan(*dblob)), 9);
  CHECK_OR(!to->ImportStream(0, absl::MakeConstSpan(dblob->data(), dblob->size() - 1)), 9);
  CHECK_OR(!to->ImportStream(N + 3, absl::MakeConstSpan(*dblob)) && !stay->ExportStream(-1), 9);
  {
    auto other = DeviceLyraDecoder::Create(rate == 16000 ? 48000 : 16000, 1, model, 2);
    CHECK_OR(other && !other->ImportStream(0, absl::MakeConstSpan(*dblob)), 9);
  }
  CHECK_OR(stay->DecodeSamplesAsync(n10), 9);
  CHECK_OR(!stay->ExportStream(0) && !stay->ImportStream(0, absl::MakeConstSpan(*dblob)), 9);
  CHECK_OR(stay->WaitDecoded(absl::Span<int16_t>(a.data(), a.size())) && stay->ExportStream(0), 9);
  Audio(&rng, 0, hop, &pcm);
  CHECK_OR(estay->EncodeAsync(absl::MakeConstSpan(pcm)), 9);
  CHECK_OR(!estay->ExportStream(0) && !estay->ImportStream(0, absl::MakeConstSpan(*eblob)), 9);
  CHECK_OR(estay->WaitEncoded() && estay->ImportStream(0, absl::MakeConstSpan(*eblob)), 9);
  std::printf("refusals: other class, other rate, wrong size, bad index, requests in flight\n");
  return 0;
}
