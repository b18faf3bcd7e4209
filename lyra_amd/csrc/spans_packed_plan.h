// spans_packed_plan.h -- the packed external-rate layout of the span calls with a rate per span
// (include/lyra_hip_spans_packed.h), on integers only: where each span's samples lie in one flat buffer, and which offsets a
// call accepts.  A span of n frames at rate r takes n * (r / 50) samples from its base; bases are multiples of 8 samples (16
// bytes: the resampler's vector loads) and every hop -- 160 / 320 / 640 / 960 -- is a multiple of 160, so the back-to-back
// layout keeps that by itself.  The kernel carries a base in units of 8 samples in a 32-bit word (SpanRsRow::pad[1]), hence
// the bound on a base: below PK_MAX_BASE = 2^34 samples, 32 GiB of int16.
// Host-only C++ that api.hip and a plain compiler share (tests/test_spans_packed_cpu.py drives it under a sanitizer).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace lyra {
namespace spk {

constexpr long long PK_ALIGN = 8;                      // samples
constexpr long long PK_MAX_BASE = 8LL * 2147483648LL;  // bases lie below it

enum PkError {
  PK_OK = 0,
  PK_BAD_RATE = 1,      // a rate that is none of the four
  PK_BAD_FRAMES = 2,    // a negative n_frames
  PK_NEGATIVE = 3,      // a negative offset or buffer length
  PK_UNALIGNED = 4,     // an offset that is no multiple of 8
  PK_RANGE = 5,         // a span with frames leaves [0, n_ext_samples)
  PK_OVERLAP = 6,       // two spans with frames share samples
  PK_TOO_FAR = 7,       // a base at or past PK_MAX_BASE
};

inline int hop_of_rate(int rate) { return rate == 8000 || rate == 16000 || rate == 32000 || rate == 48000 ? rate / 50 : 0; }

// The back-to-back layout: offsets[s] (optional) = the samples of the spans in front of s, in span order; a span of no frames
// gets the running sum and takes nothing.  n_frames[s] >= 0 and rates[s] one of the four, else -1.  Returns the total.
template <class Span>
long long layout(const Span* spans, int n_spans, const int32_t* rates, long long* offsets) {
  long long at = 0;
  for (int s = 0; s < n_spans; ++s) {
    const int hop = hop_of_rate(rates[s]);
    if (!hop || spans[s].n_frames < 0 || spans[s].n_frames > (INT64_MAX - at) / hop) return -1;
    if (offsets) offsets[s] = at;
    at += (long long)spans[s].n_frames * hop;
  }
  return at;
}

// What a call accepts: every offset non-negative and a multiple of 8; every span with frames inside [0, n_ext) and below
// PK_MAX_BASE; no two spans with frames sharing a sample.  The offset of a span without frames is judged for sign and
// alignment alone.  *bad (optional): the span the verdict names.
template <class Span>
int check(const Span* spans, int n_spans, const int32_t* rates, const long long* offsets, long long n_ext, int* bad = nullptr) {
  auto verdict = [&](int s, int e) {
    if (bad) *bad = s;
    return e;
  };
  if (n_ext < 0) return verdict(-1, PK_NEGATIVE);
  std::vector<std::pair<long long, long long>> ranges;   // [begin, end) of the spans with frames
  std::vector<int> owner;
  for (int s = 0; s < n_spans; ++s) {
    const int hop = hop_of_rate(rates[s]);
    if (!hop) return verdict(s, PK_BAD_RATE);
    if (spans[s].n_frames < 0) return verdict(s, PK_BAD_FRAMES);
    if (offsets[s] < 0) return verdict(s, PK_NEGATIVE);
    if (offsets[s] % PK_ALIGN) return verdict(s, PK_UNALIGNED);
    if (!spans[s].n_frames) continue;
    if (offsets[s] >= n_ext || spans[s].n_frames > (n_ext - offsets[s]) / hop) return verdict(s, PK_RANGE);
    if (offsets[s] >= PK_MAX_BASE) return verdict(s, PK_TOO_FAR);
    ranges.emplace_back(offsets[s], offsets[s] + (long long)spans[s].n_frames * hop);
    owner.push_back(s);
  }
  std::vector<int> order(ranges.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
  std::sort(order.begin(), order.end(), [&](int a, int b) { return ranges[a] < ranges[b]; });
  for (size_t i = 1; i < order.size(); ++i)
    if (ranges[order[i]].first < ranges[order[i - 1]].second) return verdict(owner[order[i]], PK_OVERLAP);
  return PK_OK;
}

inline const char* error_text(int e) {
  switch (e) {
    case PK_BAD_RATE: return "a sample rate that is none of 8000 / 16000 / 32000 / 48000";
    case PK_BAD_FRAMES: return "a negative frame count";
    case PK_NEGATIVE: return "a negative offset or length";
    case PK_UNALIGNED: return "an offset that is no multiple of 8 samples";
    case PK_RANGE: return "a span that leaves the external-rate buffer";
    case PK_OVERLAP: return "two spans that share samples";
    case PK_TOO_FAR: return "an offset of 2^34 samples or more";
    default: return "ok";
  }
}

}  // namespace spk
}  // namespace lyra
