// stream_blob.h -- one stream's codec state as a relocatable blob (lyra_hip_export_streams / lyra_hip_import_streams).
//
//   [HEADER_BYTES header][the 12 regions of state_layout.h in st::Region order, st::BYTES][decode-samples section]
// The decode-samples section is what lyra_hip_decode_samples_dev keeps by stream id outside the regions: the feature ring
// (DS_FIFO_DEPTH x 64 floats), the held generative hop and the held comfort-noise hop (320 int16 each); all zero when the
// exporting context never allocated them.  BYTES is a multiple of 256 and rows of a batch are BYTES apart, so every row --
// and every piece of it -- is 16-byte aligned.  All integers little-endian (the device's and every supported host's order).
//
// Header (byte offsets; everything from H_END to HEADER_BYTES is zero):
//   0  u32 MAGIC            4  u32 VERSION          8  u32 BYTES            12 u32 FINGERPRINT (layout, compile time)
//   16 u32 requant mode     20 u32 MODEL_VERSION    24 i32 source stream id 28 u32 zero
//   32 u64 effective comfort-noise key = the exporting context's seed ^ source id ^ the slot's key word (st::C_KEY)
// In the payload the key word of the R_CNG slot is ZERO: the key travels in the header, so blobs of equal stream state are
// byte-identical whichever context or id they came from.  Import stores key ^ its own seed ^ the target id there.
//
// A blob is untrusted input to kernels that form addresses and trip counts from some of its integers.  validate() checks
// the header against the importing side's own constants and EVERY such integer against its domain (list from an audit of
// the kernels that read the regions; float / int8 / int16 payload and the counters C_HOP and the key need no check):
//   ring phase words (st::PHASE of R_E1, R_E2, R_D0, R_D1)         < st::PHASE_MOD     ring row = (phase * T + t) mod R
//   R_NOISE_E / R_NOISE_D  N_INIT, N_IS_NOISE                       0 or 1
//                          N_HOPS                                   0 .. NOISE_HOPS_MAX - 1   (hops_per_update at 48 kHz)
//   R_RS_E / R_RS_D        RS_IN_POS                                0 .. 5              first tap of the decimator
//   R_RS_D                 DSA_LEFT_COUNT (decode_samples_any_plan.h) 0 .. DSA_LEFT_MAX   trip count and offset of the splice
//   R_CNG  LOSSY_CTL       concealment / 320  (bits 0-7)            0 .. 4
//                          fade / 320         (bits 8-15)           0 .. 2              index into the cross-fade table
//                          direction          (bit 16), bits 17-31  0 / 1, zero
//   R_CNG  DsState         cp                                       -320 .. 1280
//                          fade                                     0 .. 640            index into the cross-fade table
//                          to_cng                                   0 or 1
//                          gpos, cpos                               0 .. 319            offsets into the held hops
//                          wait                                     0 .. DS_FIFO_DEPTH
//                          head                                     0 .. DS_FIFO_DEPTH - 1   ring slot
//   R_CNG  bytes 44..63 except the key word, and the key word itself: zero in a blob
// With every field inside its domain the kernels' accesses stay inside the stream's own slots and rows, except that a
// DsState whose fields contradict each other can make ds_slice_kernel READ up to one hop past a held hop: the by-id hop
// arrays carry one spare row for that (decode_samples_api.inc), so the read stays inside the arrays -- but it reaches the held
// hop of the NEXT stream id: such a blob can put up to one hop of that stream's decoded audio into its own stream's output.
// Known limit of field-by-field domains; closing it needs cross-field invariants proven over ds_plan's reachable states.
// Host and device code and a plain C++ compiler share this file.
#pragma once
#include <stdint.h>
#include <string.h>

#include "decode_samples_any_plan.h"
#include "decode_samples_plan.h"
#include "state_layout.h"

namespace lyra {
namespace sb {

constexpr uint32_t MAGIC = 0x4253594Cu;   // "LYSB"
constexpr uint32_t VERSION = 1;
constexpr uint32_t MODEL_VERSION = 3;     // lyra_config.h:145-166
constexpr int HEADER_BYTES = 256;
constexpr int H_MAGIC = 0, H_VERSION = 4, H_BYTES = 8, H_FINGERPRINT = 12, H_MODE = 16, H_MODEL = 20, H_SRC_ID = 24,
              H_ZERO = 28, H_KEY = 32, H_END = 40;

constexpr int DS_RING_BYTES = DS_FIFO_DEPTH * 64 * 4;
constexpr int DS_HOP_BYTES = DS_HOP * 2;
constexpr int DS_SECTION_BYTES = DS_RING_BYTES + 2 * DS_HOP_BYTES;
constexpr int STATE_OFF = HEADER_BYTES;
constexpr int DS_OFF = STATE_OFF + st::BYTES;
constexpr int DS_RING_OFF = DS_OFF, DS_GAN_OFF = DS_RING_OFF + DS_RING_BYTES, DS_CNG_OFF = DS_GAN_OFF + DS_HOP_BYTES;
constexpr int BYTES = DS_OFF + DS_SECTION_BYTES;
static_assert(BYTES % 256 == 0 && DS_SECTION_BYTES % 16 == 0 && DS_HOP_BYTES % 16 == 0, "rows and pieces are 16-byte aligned");

constexpr int NOISE_HOPS_MAX = 150;   // NoiseEstimator::Create at 48 kHz: round(1 s / (320 / 48000 s)) hops per update

// ---- the layout table: the payload's pieces in blob order (12 regions, then the three arrays of the section) -----------
constexpr int N_PIECES = st::R_COUNT + 3;
struct Piece { int off, bytes; };
LYRA_LOSSY_HD constexpr int region_bytes(int r) {   // st::REGION_BYTES as a function (no runtime-indexed table on the device)
  return r == st::R_E0 ? st::E0_BYTES : r == st::R_E1 ? st::E1_BYTES : r == st::R_E2 ? st::E2_BYTES :
         r == st::R_D0 ? st::D0_BYTES : r == st::R_D1 ? st::D1_BYTES : r == st::R_D2 ? st::D2_BYTES :
         r == st::R_MEL ? st::MEL_BYTES : r == st::R_NOISE_E || r == st::R_NOISE_D ? st::NOISE_BYTES :
         r == st::R_RS_E || r == st::R_RS_D ? st::RS_BYTES : st::CNG_BYTES;
}
LYRA_LOSSY_HD constexpr int region_off(int r) {
  int o = STATE_OFF;
  for (int i = 0; i < r; ++i) o += region_bytes(i);
  return o;
}
LYRA_LOSSY_HD constexpr Piece piece(int i) {
  return i < st::R_COUNT ? Piece{region_off(i), region_bytes(i)}
       : i == st::R_COUNT ? Piece{DS_RING_OFF, DS_RING_BYTES}
       : i == st::R_COUNT + 1 ? Piece{DS_GAN_OFF, DS_HOP_BYTES} : Piece{DS_CNG_OFF, DS_HOP_BYTES};
}
static_assert(region_off(st::R_COUNT) == DS_OFF, "the regions fill the payload up to the section");

// ---- which regions belong to which side (LYRA_HIP_STATE_ENCODER = 1, LYRA_HIP_STATE_DECODER = 2) -----------------------
constexpr unsigned SIDE_ENCODER = 1u, SIDE_DECODER = 2u;
LYRA_LOSSY_HD constexpr unsigned region_side(int r) {
  return r == st::R_E0 || r == st::R_E1 || r == st::R_E2 || r == st::R_NOISE_E || r == st::R_RS_E ? SIDE_ENCODER : SIDE_DECODER;
}

// ---- compile-time fingerprint of everything the payload's meaning depends on -------------------------------------------
constexpr uint32_t fnv(uint32_t h, uint32_t v) {
  for (int i = 0; i < 4; ++i) h = (h ^ ((v >> (8 * i)) & 255u)) * 16777619u;
  return h;
}
constexpr uint32_t fingerprint() {
  uint32_t h = 2166136261u;
  for (int r = 0; r < st::R_COUNT; ++r) h = fnv(h, (uint32_t)st::REGION_BYTES[r]);
  h = fnv(h, (uint32_t)DS_STATE);
  h = fnv(h, (uint32_t)DS_FIFO_DEPTH);
  h = fnv(h, (uint32_t)LOSSY_CTL);
  h = fnv(h, (uint32_t)st::C_KEY);
  return h;
}
constexpr uint32_t FINGERPRINT = fingerprint();

// ---- validate ------------------------------------------------------------------------------------------------------------
// 0: the blob may be imported; else the first failing check (V_*).  `blob` must be 4-byte aligned.
enum Verdict { V_OK = 0, V_MAGIC, V_VERSION, V_BYTES, V_FINGERPRINT, V_MODE, V_MODEL, V_SRC_ID, V_HEADER_ZERO, V_PHASE,
               V_NOISE, V_RS_IN_POS, V_LOSSY_CTL, V_DS_STATE, V_CNG_HEADER, V_DSA_LEFT };

LYRA_LOSSY_HD inline uint32_t ld32(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *reinterpret_cast<const uint32_t*>(p);
#else
  uint32_t v;
  memcpy(&v, p, 4);
  return v;
#endif
}

// Every load is issued whatever the earlier checks said (no early return): the loads are independent of each other.
LYRA_LOSSY_HD inline int validate(const uint8_t* blob, uint32_t requant_mode) {
  int rc = V_OK;
#define LYRA_SB_CHECK(ok, code) do { if (!(ok) && rc == V_OK) rc = (code); } while (0)
  LYRA_SB_CHECK(ld32(blob + H_MAGIC) == MAGIC, V_MAGIC);
  LYRA_SB_CHECK(ld32(blob + H_VERSION) == VERSION, V_VERSION);
  LYRA_SB_CHECK(ld32(blob + H_BYTES) == (uint32_t)BYTES, V_BYTES);
  LYRA_SB_CHECK(ld32(blob + H_FINGERPRINT) == FINGERPRINT, V_FINGERPRINT);
  LYRA_SB_CHECK(ld32(blob + H_MODE) == requant_mode, V_MODE);
  LYRA_SB_CHECK(ld32(blob + H_MODEL) == MODEL_VERSION, V_MODEL);
  LYRA_SB_CHECK((int32_t)ld32(blob + H_SRC_ID) >= 0, V_SRC_ID);
  uint32_t z = ld32(blob + H_ZERO);
  for (int o = H_END; o < HEADER_BYTES; o += 4) z |= ld32(blob + o);
  LYRA_SB_CHECK(z == 0, V_HEADER_ZERO);
  const int ringed[4] = {st::R_E1, st::R_E2, st::R_D0, st::R_D1};
  for (int i = 0; i < 4; ++i) LYRA_SB_CHECK(ld32(blob + region_off(ringed[i]) + st::PHASE) < (uint32_t)st::PHASE_MOD, V_PHASE);
  const int noise[2] = {st::R_NOISE_E, st::R_NOISE_D};
  for (int i = 0; i < 2; ++i) {
    const uint8_t* n = blob + region_off(noise[i]);
    LYRA_SB_CHECK(ld32(n + st::N_INIT) <= 1u, V_NOISE);
    LYRA_SB_CHECK(ld32(n + st::N_HOPS) < (uint32_t)NOISE_HOPS_MAX, V_NOISE);
    LYRA_SB_CHECK(ld32(n + st::N_IS_NOISE) <= 1u, V_NOISE);
  }
  LYRA_SB_CHECK(ld32(blob + region_off(st::R_RS_E) + st::RS_IN_POS) < 6u, V_RS_IN_POS);
  LYRA_SB_CHECK(ld32(blob + region_off(st::R_RS_D) + st::RS_IN_POS) < 6u, V_RS_IN_POS);
  const uint8_t* g = blob + region_off(st::R_CNG);
  const uint32_t ctl = ld32(g + LOSSY_CTL);
  LYRA_SB_CHECK((ctl & 255u) <= (uint32_t)(LOSSY_CONCEAL / 320) && ((ctl >> 8) & 255u) <= (uint32_t)(LOSSY_FADE / 320) &&
                (ctl >> 17) == 0u, V_LOSSY_CTL);
  const int32_t cp = (int32_t)ld32(g + DS_STATE), fade = (int32_t)ld32(g + DS_STATE + 4);
  const uint32_t to_cng = ld32(g + DS_STATE + 8), gpos = ld32(g + DS_STATE + 12), cpos = ld32(g + DS_STATE + 16),
                 wait = ld32(g + DS_STATE + 20), head = ld32(g + DS_STATE + 24);
  LYRA_SB_CHECK(cp >= -DS_HOP && cp <= LOSSY_CONCEAL && fade >= 0 && fade <= LOSSY_FADE && to_cng <= 1u &&
                gpos < (uint32_t)DS_HOP && cpos < (uint32_t)DS_HOP && wait <= (uint32_t)DS_FIFO_DEPTH &&
                head < (uint32_t)DS_FIFO_DEPTH, V_DS_STATE);
  uint32_t zc = ld32(g + 12);
  for (int o = DS_STATE + (int)sizeof(DsState); o < st::C_OLA; o += 4) zc |= ld32(g + o);   // includes the key word
  LYRA_SB_CHECK(zc == 0, V_CNG_HEADER);
  // BufferedResampler's leftover count of lyra_hip_decode_samples_any_dev (zero in every blob written before that call existed)
  LYRA_SB_CHECK(ld32(blob + region_off(st::R_RS_D) + DSA_LEFT_COUNT) <= (uint32_t)DSA_LEFT_MAX, V_DSA_LEFT);
#undef LYRA_SB_CHECK
  return rc;
}

// ---- building a header (export kernel, tests) ----------------------------------------------------------------------------
LYRA_LOSSY_HD inline void put32(uint8_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  *reinterpret_cast<uint32_t*>(p) = v;
#else
  memcpy(p, &v, 4);
#endif
}
// the 16 words that are not all zero; the caller has zeroed (or zeroes) the rest of the header
LYRA_LOSSY_HD inline void header_words(uint32_t requant_mode, int32_t src_id, uint64_t key, uint32_t w[16]) {
  for (int i = 0; i < 16; ++i) w[i] = 0;
  w[H_MAGIC / 4] = MAGIC; w[H_VERSION / 4] = VERSION; w[H_BYTES / 4] = (uint32_t)BYTES; w[H_FINGERPRINT / 4] = FINGERPRINT;
  w[H_MODE / 4] = requant_mode; w[H_MODEL / 4] = MODEL_VERSION; w[H_SRC_ID / 4] = (uint32_t)src_id;
  w[H_KEY / 4] = (uint32_t)key; w[H_KEY / 4 + 1] = (uint32_t)(key >> 32);
}
LYRA_LOSSY_HD inline uint64_t header_key(const uint8_t* blob) {
  return (uint64_t)ld32(blob + H_KEY) | ((uint64_t)ld32(blob + H_KEY + 4) << 32);
}

}  // namespace sb
}  // namespace lyra
