// spans_lossy_plan.h -- the planner of lyra_hip_decode_spans_lossy_dev (spans_lossy_api.inc): what every tick of every span does,
// worked out on the host before any kernel runs.  Plain C++, no device: host code, the C ABI's lyra_hip_spans_lossy_plan and the
// CPU tests share this file.
//
// lossy_tick (lossy_plan.h) is a pure function of the control word and of whether a packet arrived, so the control word at the
// start of a span and the span's packet sizes fix, for every frame, which legs run (lossy_info) and where the cross-fade
// stands.  What the legs then need of each other is little:
//   generative model  advances on run_gen ticks only, on the packet's RVQ decode or on zero features: a stream whose state is
//                     convolution history, so sp::plan cuts the COMPACTED list of run_gen frames into chunks and lanes;
//   NoiseEstimator    (decoder side) a recurrence over the generative hops of the RECEIVED ticks, in order;
//   comfort noise     run_cng tick k of a span uses hop counter C_HOP + k and the estimate as it stood after the received
//                     frames in front of the tick: its VERSION = their number.  Version 0 is the estimate on entry; the scan
//                     over the received list writes the versions that some tick reads to snapshot rows.
#pragma once
#include <stdint.h>

#include <vector>

#include "lossy_plan.h"
#include "spans_plan.h"

namespace lyra {
namespace slp {

struct SpanLists {
  std::vector<int64_t> gen_frame;      // buffer frames of the run_gen ticks, in order ...
  std::vector<uint8_t> gen_received;   // ... 1: from the packet, 0: concealed (zero features); plan_mixed: the packet's size
  std::vector<int64_t> rx_frame;       // buffer frames of the received ticks
  std::vector<int64_t> cng_frame;      // buffer frames of the run_cng ticks ...
  std::vector<int32_t> cng_version;    // ... and the received frames of the span in front of each
  std::vector<int32_t> versions;       // the versions some tick reads, rising, each once
  std::vector<int32_t> info;           // lossy_info per frame of the span
  uint32_t ctl_out = 0;                // the control word after the span
};

// packet_bytes[frame]: 0 = no packet, nbytes = a packet; ctl_in[s]: the control word of span s's stream on entry.
// Returns 0, or sp::PLAN_EINVAL for a size that is neither, negative spans or missing arrays; *out is then unspecified.
// nbytes == SIZE_PER_FRAME (plan_mixed): a packet is any size of the codec (mixed_received: 8 / 15 / 23), chosen per frame as
// SetEncodedPacket does, and gen_received holds that size.  The state machine sees only whether a packet came, so every other
// list is the uniform plan's for the same receive pattern.
constexpr int SIZE_PER_FRAME = -1;
inline int plan_sized(const sp::Span* spans, int n_spans, const int32_t* packet_bytes, int nbytes, const uint32_t* ctl_in,
                      std::vector<SpanLists>* out) {
  const bool mixed = nbytes == SIZE_PER_FRAME;
  if (n_spans < 0 || (!mixed && nbytes <= 0) || (n_spans && (!spans || !ctl_in)) || !out) return sp::PLAN_EINVAL;
  out->assign((size_t)n_spans, SpanLists());
  for (int s = 0; s < n_spans; ++s) {
    const int64_t first = spans[s].first_frame, n = spans[s].n_frames;
    if (first < 0 || n < 0 || n > INT32_MAX || (n && !packet_bytes)) return sp::PLAN_EINVAL;
    SpanLists& L = (*out)[(size_t)s];
    uint32_t ctl = ctl_in[s];
    int32_t received = 0;
    L.info.reserve((size_t)n);
    for (int64_t f = first; f < first + n; ++f) {
      const int32_t pb = packet_bytes[f];
      if (pb != 0 && (mixed ? !mixed_received(pb) : pb != nbytes)) return sp::PLAN_EINVAL;
      const LossyTick t = lossy_tick(ctl, pb != 0);
      ctl = t.ctl;
      if (t.run_cng) {   // in front of the tick's own update: launch_cng precedes launch_noise_masked
        L.cng_frame.push_back(f);
        L.cng_version.push_back(received);
        if (L.versions.empty() || L.versions.back() != received) L.versions.push_back(received);
      }
      if (t.run_gen) {
        L.gen_frame.push_back(f);
        L.gen_received.push_back(!t.feed_est ? 0 : mixed ? (uint8_t)pb : 1);
      }
      if (t.feed_est) {
        L.rx_frame.push_back(f);
        ++received;
      }
      L.info.push_back(lossy_info(t));
    }
    L.ctl_out = ctl;
  }
  return 0;
}

inline int plan(const sp::Span* spans, int n_spans, const int32_t* packet_bytes, int nbytes, const uint32_t* ctl_in,
                std::vector<SpanLists>* out) {
  return nbytes <= 0 ? sp::PLAN_EINVAL : plan_sized(spans, n_spans, packet_bytes, nbytes, ctl_in, out);
}
inline int plan_mixed(const sp::Span* spans, int n_spans, const int32_t* packet_bytes, const uint32_t* ctl_in,
                      std::vector<SpanLists>* out) {
  return plan_sized(spans, n_spans, packet_bytes, SIZE_PER_FRAME, ctl_in, out);
}

// What the generative model sees: span s = the run_gen ticks of span s, laid out span after span in one dense list.
inline std::vector<sp::Span> compact_gen_spans(const sp::Span* spans, const std::vector<SpanLists>& lists) {
  std::vector<sp::Span> c(lists.size());
  int64_t at = 0;
  for (size_t s = 0; s < lists.size(); ++s) {
    c[s] = sp::Span{spans[s].stream_id, at, (int64_t)lists[s].gen_frame.size()};
    at += c[s].n_frames;
  }
  return c;
}

}  // namespace slp
}  // namespace lyra
