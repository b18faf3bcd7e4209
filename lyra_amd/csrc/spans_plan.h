// spans_plan.h -- time-parallel transcodes of long recordings: the warm-up bound and the planner of
// lyra_hip_encode_spans_dev / lyra_hip_decode_spans_dev (spans_api.inc).  Plain C++, no device: host code, the C ABI's
// lyra_hip_spans_plan and the CPU tests share this file.
//
// The codec state is convolution history only (state_layout.h), so the state after hop t and every output from hop t + 1 on
// are functions of a bounded window of past hops.  A stream that starts from the reset state `warmup` hops before frame f
// therefore holds, at frame f, exactly the state of the stream that ran from frame 0 -- bit for bit, every kernel computes a
// row from the same operands in the same order -- and a long span can be cut into chunks that run side by side.
//
// Warm-up bound.  Walk a graph from its output back to its input and keep `a`, the number of rows in front of
// the first row of hop t, at the current layer's time resolution, that the first output row of hop t can see:
//   causal convolution, kernel K, dilation d, stride 1     a += (K - 1) d          (its history: state_layout.h rows)
//   residual block with such a depthwise convolution       a += (K - 1) d          (the skip path sees less)
//   strided convolution K / s, n_in = s n_out rows          a  = s a + (K - s)      (concat(state, x), VALID: SURVEY.md A.1)
//   transposed convolution K / s, n_out = s n_in rows       a  = floor((a + K - 1) / s)  (output row r sums inputs i with
//                                                                                   i s <= r <= i s + K - 1: A.3)
// At the graph's input, a rows are ceil(a / rows per hop) hops.  Every history entry kept after hop t is an operand of hop
// t + 1's first rows, i.e. lies inside that window shifted by one hop: `warmup` hops restore the state, and the outputs that
// follow are computed from restored state.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "state_layout.h"

namespace lyra {
namespace sp {

constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }
// the three residual blocks of a stage: depthwise k3, dilations 1 / 3 / 9 (histories of 2, 6 and 18 rows)
constexpr int RESBLOCKS = (3 - 1) * 1 + (3 - 1) * 3 + (3 - 1) * 9;
constexpr int conv_back(int a, int K, int s) { return s * a + (K - s); }
constexpr int tconv_back(int a, int K, int s) { return (a + K - 1) / s; }

// soundstream_encoder, output to input: bottleneck k3 | k4/s2 | 3 blocks @ 2 rows per hop | k4/s2 |
// 3 blocks @ 4 | k10/s5 | 3 blocks @ 20 | first layer k64/s16 on samples
constexpr int enc_samples_back() {
  int a = 3 - 1;
  a = conv_back(a, 4, 2) + RESBLOCKS;
  a = conv_back(a, 4, 2) + RESBLOCKS;
  a = conv_back(a, 10, 5) + RESBLOCKS;
  return conv_back(a, 64, 16);
}
// lyragan (A.3), output to input: last layer tconv k64/s16 | 3 blocks @ 20 rows per hop | tconv k10/s5 | 3 blocks @ 4 |
// tconv k4/s2 | 3 blocks @ 2 | tconv k4/s2 | bottleneck k3 on feature rows
constexpr int dec_rows_back() {
  int a = tconv_back(0, 64, 16) + RESBLOCKS;
  a = tconv_back(a, 10, 5) + RESBLOCKS;
  a = tconv_back(a, 4, 2) + RESBLOCKS;
  return tconv_back(a, 4, 2) + (3 - 1);
}
constexpr int W_ENC = ceil_div(enc_samples_back(), 320);   // hops
constexpr int W_DEC = dec_rows_back();                     // one feature row per hop
static_assert(enc_samples_back() == 7904 && W_ENC == 25 && W_DEC == 25, "DESIGN.md 4.5 quotes these");
// the layer table above against the histories the kernels keep
static_assert(st::E_R0_0 - st::E_FIRST == (64 - 16) * 4 && st::E0_BYTES >= st::E_D0 + (10 - 5) * 64 * 4 &&
                  st::E_D1 - st::E_R1_2 == 18 * 128 * 4 && st::E_BOTT - st::E_D2 == (4 - 2) * 256 &&
                  st::D_UP0 - st::D_HEAD == (3 - 1) * 64 * 4 && st::D_UP2 - st::D_R1_2 == 18 * 128 * 4 &&
                  st::D2_BYTES >= st::D_UP3 + (64 - 16) * 4,
              "state_layout.h histories");

constexpr int SIDE_ENC = 0, SIDE_DEC = 1;
constexpr int warmup(int side) { return side == SIDE_ENC ? W_ENC : side == SIDE_DEC ? W_DEC : -1; }

struct Span { int32_t stream_id; int64_t first_frame; int64_t n_frames; };   // = lyra_hip_span
// One chunk = one row of the call's batch (= lyra_hip_span_chunk).  It runs on `stream_id` for n_warmup + n_frames steps:
// step i reads buffer frame first_frame - n_warmup + i and, from step n_warmup on, writes its output there.
struct Chunk {
  int32_t stream_id;     // the span's own stream (chunk 0 of a span, n_warmup 0) or a lane
  int32_t span;          // index of the span it belongs to
  int64_t first_frame;   // buffer frame of its first produced hop
  int32_t n_frames;      // produced hops
  int32_t n_warmup;      // hops replayed in front of them, outputs discarded: 0 or warmup(side)
  int32_t phase_offset;  // lanes: (frames of the span in front of the first replayed hop) mod st::PHASE_MOD -- the lane's ring
                         // phase words start at the span stream's plus this, so both write the same ring rows
  int32_t last;          // lanes: 1 = the span's last chunk; its state is handed over to the span's stream
};

enum { PLAN_EINVAL = -1 };

// frames a span of N needs beyond its own T-step chunk, in lanes of T - W produced frames each
inline int64_t lanes_needed(int64_t N, int64_t T, int W) { return N <= T ? 0 : (N - T + (T - W) - 1) / (T - W); }

// Cuts every span into chunks and orders them as the rows of the batch.  What it minimises: the number of steps T of the
// call (every step is one pass through the stage kernels, whose time barely depends on the batch below a few thousand rows).
// With chunk 0 of a span running T hops on the span's own stream and every lane W + (T - W) hops, a span of N frames needs
// ceil((N - T) / (T - W)) lanes; T is the smallest step count whose lane demand fits n_lanes (bisection: the demand falls as T
// grows; T = the longest span needs none).  Each span then shrinks its own step count to the smallest that its lanes still
// cover, T_s = ceil((N + k W) / (k + 1)), so short spans leave the batch early.  Work inflation: (L + W) / L for lane
// chunks of L = T_s - W frames.  A lane's warm-up frames lie inside its span because chunk 0 is T_s > W frames long.
// Row order: the spans' own chunks by falling step count, then the lane chunks by falling step count, so the lanes active at
// step i are a prefix of the lane rows (own rows that have ended inside the prefix are masked on the device).
// Returns the number of chunks (<= n_spans + n_lanes) or PLAN_EINVAL: bad side, negative counts or frames, an id outside
// 0..max_streams-1 or named twice among spans and lanes, frame ranges of two spans that overlap.  *n_steps: T.
inline int plan(int side, const Span* spans, int n_spans, const int32_t* lane_ids, int n_lanes, int max_streams,
                std::vector<Chunk>* out, int* n_steps) {
  const int W = warmup(side);
  if (W < 0 || n_spans < 0 || n_lanes < 0 || (n_spans && !spans) || (n_lanes && !lane_ids)) return PLAN_EINVAL;
  if ((int64_t)n_spans + n_lanes > max_streams) return PLAN_EINVAL;
  std::vector<uint8_t> seen((size_t)std::max(max_streams, 0), 0);
  auto take = [&](int32_t id) {
    if (id < 0 || id >= max_streams || seen[id]) return false;
    seen[id] = 1;
    return true;
  };
  int64_t longest = 0;
  for (int s = 0; s < n_spans; ++s) {
    if (!take(spans[s].stream_id) || spans[s].first_frame < 0 || spans[s].n_frames < 0 ||
        spans[s].n_frames > INT32_MAX - W)
      return PLAN_EINVAL;
    longest = std::max(longest, spans[s].n_frames);
  }
  for (int l = 0; l < n_lanes; ++l)
    if (!take(lane_ids[l])) return PLAN_EINVAL;
  {
    std::vector<std::pair<int64_t, int64_t>> r;
    for (int s = 0; s < n_spans; ++s)
      if (spans[s].n_frames) r.push_back({spans[s].first_frame, spans[s].n_frames});
    std::sort(r.begin(), r.end());
    for (size_t i = 1; i < r.size(); ++i)
      if (r[i - 1].first + r[i - 1].second > r[i].first) return PLAN_EINVAL;
  }
  auto demand = [&](int64_t T) {
    int64_t k = 0;
    for (int s = 0; s < n_spans; ++s) k += lanes_needed(spans[s].n_frames, T, W);
    return k;
  };
  int64_t T = longest;
  if (n_lanes > 0 && longest > W + 1) {
    int64_t lo = W + 1, hi = longest;   // demand(hi) == 0 fits
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (demand(mid) <= n_lanes) hi = mid; else lo = mid + 1;
    }
    T = lo;
  }
  std::vector<Chunk> own, lanes;
  int next_lane = 0;
  for (int s = 0; s < n_spans; ++s) {
    const int64_t N = spans[s].n_frames;
    if (N == 0) continue;
    const int64_t k = lanes_needed(N, T, W);
    const int64_t Ts = k ? (N + k * W + k) / (k + 1) : N;
    own.push_back({spans[s].stream_id, s, spans[s].first_frame, (int32_t)Ts, 0, 0, 0});
    for (int64_t j = 0, at = Ts; j < k; ++j, at += Ts - W) {
      const int64_t n = std::min<int64_t>(Ts - W, N - at);
      lanes.push_back({lane_ids[next_lane++], s, spans[s].first_frame + at, (int32_t)n, W,
                       (int32_t)((at - W) % st::PHASE_MOD), j == k - 1});
    }
  }
  auto longer = [](const Chunk& a, const Chunk& b) { return a.n_warmup + a.n_frames > b.n_warmup + b.n_frames; };
  std::stable_sort(own.begin(), own.end(), longer);
  std::stable_sort(lanes.begin(), lanes.end(), longer);
  out->assign(own.begin(), own.end());
  out->insert(out->end(), lanes.begin(), lanes.end());
  int steps = 0;
  for (const Chunk& c : *out) steps = std::max(steps, c.n_warmup + c.n_frames);
  if (n_steps) *n_steps = steps;
  return (int)out->size();
}

}  // namespace sp
}  // namespace lyra
