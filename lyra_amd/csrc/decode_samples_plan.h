// decode_samples_plan.h -- LyraDecoder's packet-loss state machine for ANY request size up to one hop, on integers only.
//
// SetEncodedPacket's adjustment of concealment_progress (lyra_decoder.cc:186-196) and the loop of DecodeSamplesInternal
// (:228-315) with GetNumSamplesToGenerate (:65-91), for an internal request of 0..320 samples at 16 kHz.  Nothing in it
// depends on a decoded sample, so one kernel plans a whole call of lyra_hip_decode_samples_dev.  Per stream:
//   cp    concealment_progress, signed, -320..1280 (negative: the rest of a concealed / comfort-noise hop after a packet)
//   fade  fade_progress 0..640, to_cng  fade_direction == kFadeToCNG
//   gpos  read position inside the current generative hop (0 = none held), cpos the same for the comfort-noise hop
//   wait  feature vectors queued in front of the generative model whose hop has not started, head their ring position
// (GenerativeModel's FIFO, generative_model_interface.h:50-101, holds `wait` vectors plus the one of a hop in progress.)
// The seven integers live in bytes DS_STATE.. of the stream's comfort-noise slot (state_layout.h R_CNG, beside LOSSY_CTL);
// all zero is the reference's initial state, so context creation and lyra_hip_reset_streams need nothing new.
// For requests of at most one hop the loop runs at most twice, starts at most one generative and one comfort-noise hop and
// completes at most one received hop (tests/test_decode_samples_plan_cpu.py proves it on the reference model's trajectory);
// ds_plan reports `bad` instead of going further.  The queue is bounded (DS_FIFO_DEPTH; the reference's is not): a packet
// that finds it full is not delivered at all -- no adjustment, no queueing -- and reported.
// Host and device code and a plain C++ compiler share this file.
#pragma once
#include <stdint.h>

#include "lossy_plan.h"

namespace lyra {

constexpr int DS_STATE = 16;        // byte offset of DsState in a stream's R_CNG slot (C_HOP 0..7, LOSSY_CTL 8..11, C_OLA 64..)
constexpr int DS_FIFO_DEPTH = 4;    // waiting feature vectors per stream (a 10 ms receiver one tick late holds 2)
constexpr int DS_HOP = 320;

struct DsState { int32_t cp, fade, to_cng, gpos, cpos, wait, head; };
static_assert(DS_STATE + sizeof(DsState) <= 64, "DsState must fit in front of the overlap-add accumulator");

// One pass of the loop: n samples, of which gen_n from the generative hop at gen_off and cng_n from the comfort-noise hop
// at cng_off (each n or 0); where both run the cross-fade starts from fade_progress `fade` in direction `dir`.
struct DsSeg { int n, gen_n, cng_n, gen_off, cng_off, fade, dir; };

constexpr int DS_SRC_NONE = -2, DS_SRC_ZERO = -1;   // gen_src: no hop starts / ZeroFeatureEstimator / ring slot >= 0

struct DsPlan {
  DsState s;          // state after the call
  int dropped;        // the packet found the queue full and was not delivered
  int push_slot;      // ring slot that takes this call's packet, or -1
  int nseg;
  DsSeg seg[2];
  int gen_start;      // pass that starts a generative hop, or -1
  int gen_src;        // where that hop's features come from
  int cng_start;      // pass that starts a comfort-noise hop, or -1
  int est_seg;        // pass at whose end a RECEIVED hop completes (NoiseEstimator::ReceiveSamples), or -1
  int est_new;        // that hop is the one started in this call (else the stream's held hop)
  int comfort_noise;  // is_comfort_noise() after the call
  int bad;            // a bound stated above was exceeded (never, for requests of at most one hop)
};

LYRA_LOSSY_HD inline int ds_model_available(const DsState& s) { return s.wait * DS_HOP + (s.gpos ? DS_HOP - s.gpos : 0); }
LYRA_LOSSY_HD inline int ds_cng_available(const DsState& s) { return s.cpos ? DS_HOP - s.cpos : 0; }

// received: a valid packet came with this call; total: internal samples requested (0..320)
LYRA_LOSSY_HD inline DsPlan ds_plan(DsState s, bool received, int total) {
  DsPlan p;
  p.dropped = 0; p.push_slot = -1; p.nseg = 0;
  p.gen_start = -1; p.gen_src = DS_SRC_NONE; p.cng_start = -1; p.est_seg = -1; p.est_new = 0; p.bad = 0;
  for (int k = 0; k < 2; ++k) { DsSeg z = {0, 0, 0, 0, 0, 0, -1}; p.seg[k] = z; }
  // ---- SetEncodedPacket (:186-196) ----
  if (received && s.wait >= DS_FIFO_DEPTH) { p.dropped = 1; received = false; }
  if (received) {
    if (s.cp == LOSSY_CONCEAL) s.cp = -ds_cng_available(s);
    else if (s.cp > 0) s.cp = -ds_model_available(s);
    p.push_slot = (s.head + s.wait) % DS_FIFO_DEPTH;
    s.wait++;
  }
  // ---- DecodeSamplesInternal (:228-315) ----
  int done = 0;
  while (done < total) {
    if (p.nseg == 2) { p.bad = 1; break; }
    // GetNumSamplesToGenerate (:65-91)
    int rem = s.cp < 0 ? -s.cp : s.cp < LOSSY_CONCEAL ? ds_model_available(s) % DS_HOP : ds_cng_available(s);
    if (rem == 0) rem = DS_HOP;
    const int n = total - done < rem ? total - done : rem;
    const bool rx = ds_model_available(s) > 0 && s.cp == 0;
    if (rx) s.to_cng = 0;
    else if (s.cp == LOSSY_CONCEAL) s.to_cng = 1;
    else s.cp += n;
    const int dir = s.to_cng ? 1 : -1;
    int gen_n = n, cng_n = n, next = s.fade + dir * n;
    if (dir == 1 && s.fade == LOSSY_FADE) { next = LOSSY_FADE; gen_n = 0; }
    else if (dir == -1 && s.fade == 0) { next = 0; cng_n = 0; }
    DsSeg& g = p.seg[p.nseg];
    g.n = n; g.gen_n = gen_n; g.cng_n = cng_n; g.gen_off = s.gpos; g.cng_off = s.cpos; g.fade = s.fade; g.dir = dir;
    bool completed = false;
    if (gen_n > 0) {
      if (s.gpos == 0) {   // RunConditioning of the oldest queued features, or of ZeroFeatureEstimator's
        if (p.gen_start >= 0) p.bad = 1;
        p.gen_start = p.nseg;
        if (s.wait > 0) { p.gen_src = s.head; s.head = (s.head + 1) % DS_FIFO_DEPTH; s.wait--; }
        else p.gen_src = DS_SRC_ZERO;
      }
      if (gen_n > DS_HOP - s.gpos) p.bad = 1;
      s.gpos += gen_n;
      if (s.gpos >= DS_HOP) { s.gpos = 0; completed = true; }
    }
    if (cng_n > 0) {
      if (s.cpos == 0) {
        if (p.cng_start >= 0) p.bad = 1;
        p.cng_start = p.nseg;
      }
      if (cng_n > DS_HOP - s.cpos) p.bad = 1;
      s.cpos += cng_n;
      if (s.cpos >= DS_HOP) s.cpos = 0;
    }
    s.fade = next;
    if (rx && completed) {   // received hops are taken whole: the estimator's input is the stream's entire hop
      if (p.est_seg >= 0) p.bad = 1;
      p.est_seg = p.nseg;
      p.est_new = p.gen_start == p.nseg ? 1 : 0;
    }
    done += n;
    p.nseg++;
  }
  p.s = s;
  p.comfort_noise = s.fade == LOSSY_FADE ? 1 : 0;
  return p;
}

// ---- what the plan kernel hands the noise-stream leg: four int32 per row ------------------------------------------------
//   [0] n of pass 1 | n of pass 2 << 16     [1] DS_* flags     [2] gen_off | cng_off << 16 of pass 1 (pass 2 starts at 0)
//   [3] fade of pass 1 | fade of pass 2 << 16
constexpr int32_t DS_S1_GEN = 1, DS_S1_CNG = 2, DS_S2_GEN = 4, DS_S2_CNG = 8, DS_S1_TO_CNG = 16, DS_S2_TO_CNG = 32,
                  DS_GEN_NEW = 64,      // a generative hop started: the call's hop row is valid and becomes the held hop
                  DS_CNG_NEW = 128,     // the same for comfort noise
                  DS_EST = 256, DS_EST_NEW = 512, DS_CN = 1024,
                  DS_S1_GEN_NEW = 2048, DS_S1_CNG_NEW = 4096;   // pass 1 reads the hop started in this call

LYRA_LOSSY_HD inline void ds_info(const DsPlan& p, int32_t w[4]) {
  const DsSeg &a = p.seg[0], &b = p.seg[1];
  int32_t f = 0;
  if (a.gen_n) f |= DS_S1_GEN;
  if (a.cng_n) f |= DS_S1_CNG;
  if (b.gen_n) f |= DS_S2_GEN;
  if (b.cng_n) f |= DS_S2_CNG;
  if (a.dir > 0) f |= DS_S1_TO_CNG;
  if (b.dir > 0) f |= DS_S2_TO_CNG;
  if (p.gen_start >= 0) f |= DS_GEN_NEW;
  if (p.cng_start >= 0) f |= DS_CNG_NEW;
  if (p.est_seg >= 0) f |= DS_EST;
  if (p.est_new) f |= DS_EST_NEW;
  if (p.comfort_noise) f |= DS_CN;
  if (p.gen_start == 0) f |= DS_S1_GEN_NEW;
  if (p.cng_start == 0) f |= DS_S1_CNG_NEW;
  w[0] = a.n | (b.n << 16);
  w[1] = f;
  w[2] = a.gen_off | (a.cng_off << 16);
  w[3] = a.fade | (b.fade << 16);
}

// The request-size rule of lyra_hip_decode_samples_dev: BufferedResampler's leftover (buffered_resampler.cc:92-147) stays
// empty for ever iff every request maps to a whole number of internal samples.  Returns that number, or -1.
LYRA_LOSSY_HD inline int ds_internal_samples(int num_samples, int sample_rate_hz) {
  if (sample_rate_hz != 8000 && sample_rate_hz != 16000 && sample_rate_hz != 32000 && sample_rate_hz != 48000) return -1;
  if (num_samples < 0 || num_samples > sample_rate_hz / 50) return -1;
  const long v = (long)num_samples * 16000;
  return v % sample_rate_hz ? -1 : (int)(v / sample_rate_hz);
}

}  // namespace lyra
