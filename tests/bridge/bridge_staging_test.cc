// bridge_staging_test.cc -- a program of its own over lyra_amd/csrc/bridge_staging.h (no GPU, no library), built with
// -fsanitize=address,undefined by tests/test_bridge_cpu.py.  For every kind of tick, B in {1, 2, 37, max_streams} with
// max_streams in {1, 64, 289262}, and E in {0, 1 + N, the largest n_rooms * (1 + N) <= max_streams} for N in {1, 8}:
//   - no two arrays of a direction overlap, and none reaches past the direction's total;
//   - every int32 array is 4-byte aligned, the levels 8-byte aligned;
//   - a kind has exactly the arrays its tick has;
//   - the totals are the bytes the begin() calls have always moved, written out here as formulas of n and E;
//   - both totals are within what a slot of a context of max_streams holds.
// Prints one line per failure and "ok" at the end.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "bridge_staging.h"

using namespace bridge_staging;

namespace {

struct Arr {
  const char* name;
  size_t word, bytes, align;   // offset in 4-byte words (NONE: absent), size, required alignment
  bool wanted;                 // this kind of tick has it
};

int failures = 0;

void fail(const char* what, const char* name, int kind, size_t B, size_t E) {
  std::printf("FAIL %s: %s (kind %d, B %zu, E %zu)\n", what, name, kind, B, E);
  ++failures;
}

void check_direction(const char* dir, std::vector<Arr> arrs, size_t total, int kind, size_t B, size_t E) {
  std::vector<Arr> present;
  for (const Arr& a : arrs) {
    if ((a.word != NONE) != a.wanted) fail("presence", a.name, kind, B, E);
    if (a.word == NONE) continue;
    if ((a.word * 4) % a.align) fail("alignment", a.name, kind, B, E);
    if (a.word * 4 + a.bytes > total) fail("past the total", a.name, kind, B, E);
    present.push_back(a);
  }
  std::sort(present.begin(), present.end(), [](const Arr& a, const Arr& b) { return a.word < b.word; });
  for (size_t i = 1; i < present.size(); ++i)
    if (present[i - 1].word * 4 + present[i - 1].bytes > present[i].word * 4) fail(dir, present[i].name, kind, B, E);
}

void check(Kind kind, size_t B, size_t E, size_t max_streams) {
  const Layout L = layout(kind, B, E);
  const size_t n = B, pk = 23;
  const bool sel = kind != FULL, shr = kind == SHARED;
  check_direction("overlap going up",
                  {{"ids", L.ids, n * 4, 4, true},
                   {"packet_bytes", L.packet_bytes, n * 4, 4, true},
                   {"order", L.order, n * 4, 4, true},
                   {"muted", L.muted, n * 4, 4, true},
                   {"room_start", L.room_start, (n + 1) * 4, 4, true},
                   {"num_bits", L.num_bits, n * 4, 4, !shr},
                   {"dtx", L.dtx, n * 4, 4, !shr},
                   {"room_keys", L.room_keys, n * 4, 4, shr},
                   {"enc_ids", L.enc_ids, E * 4, 4, shr},
                   {"enc_bits", L.enc_bits, E * 4, 4, shr},
                   {"enc_dtx", L.enc_dtx, E * 4, 4, shr},
                   {"in_packets", L.in_packets, n * pk, 1, true}},
                  L.in_bytes, kind, B, E);
  check_direction("overlap coming down",
                  {{"out_packet_bytes", L.out_packet_bytes, n * 4, 4, true},
                   {"is_noise", L.is_noise, n * 4, 4, true},
                   {"is_comfort_noise", L.is_comfort_noise, n * 4, 4, true},
                   {"is_speaker", L.is_speaker, n * 4, 4, sel},
                   {"levels", L.levels, n * 8, 8, sel},
                   {"slot_of", L.slot_of, n * 4, 4, shr},
                   {"out_packets", L.out_packets, n * pk, 1, true}},
                  L.out_bytes, kind, B, E);
  // the common prefix of what comes down: one end() serves every kind
  const Layout F = layout(FULL, B, 0);
  if (L.out_packet_bytes != F.out_packet_bytes || L.is_noise != F.is_noise || L.is_comfort_noise != F.is_comfort_noise)
    fail("prefix", "coming down", kind, B, E);
  if (sel && (L.is_speaker != layout(SPEAKERS, B, 0).is_speaker || L.levels != layout(SPEAKERS, B, 0).levels))
    fail("prefix", "selection outputs", kind, B, E);
  // the bytes each kind has always moved
  const size_t want_in = shr ? (6 * n + 1 + 3 * E) * 4 + n * 23 : (7 * n + 1) * 4 + n * 23;
  const size_t want_out = (shr ? 7 : sel ? 6 : 3) * n * 4 + n * 23;
  if (L.in_bytes != want_in) fail("total", "going up", kind, B, E);
  if (L.out_bytes != want_out) fail("total", "coming down", kind, B, E);
  // ... and what a slot has always held
  const size_t m = max_streams;
  if (slot_in_bytes(m) != (9 * m + 1) * 4 + m * 23 || slot_out_bytes(m) != 7 * m * 4 + m * 23) fail("total", "slot", kind, B, E);
  if (L.in_bytes > slot_in_bytes(m)) fail("slot", "going up", kind, B, E);
  if (L.out_bytes > slot_out_bytes(m)) fail("slot", "coming down", kind, B, E);
}

}  // namespace

int main() {
  long cases = 0;
  for (size_t max_streams : {(size_t)1, (size_t)64, (size_t)289262})
    for (size_t B : {(size_t)1, (size_t)2, (size_t)37, max_streams}) {
      if (B > max_streams) continue;
      for (size_t N : {(size_t)1, (size_t)8})
        for (size_t E : {(size_t)0, 1 + N, max_streams / (1 + N) * (1 + N)}) {
          if (E > max_streams) continue;   // (refused by begin(): more encoder rows than streams)
          for (Kind kind : {FULL, SPEAKERS, SHARED}) {
            check(kind, B, E, max_streams);
            ++cases;
          }
        }
    }
  std::printf("%ld cases, %d failures\n", cases, failures);
  if (failures || cases < 100) return 1;
  std::printf("ok\n");
  return 0;
}
