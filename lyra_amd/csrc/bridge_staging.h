// bridge_staging.h -- host-only: where every array of a conference-bridge tick lies in the two pinned staging slots of
// lyra_hip_bridge_begin / lyra_hip_speakers_begin / lyra_hip_shared_begin and their _end calls (bridge_api.inc), shared by
// api.hip and a plain compiler (tests/bridge/bridge_staging_test.cc).  One upload and one download per tick, so each
// direction is one run of bytes: int32 arrays first (offsets in 4-byte words), then the packets, 23 bytes a row.  The three
// kinds of tick share a prefix in both directions -- one begin() fills it, one end() reads it -- and no kind carries
// another's arrays: a full-mix tick moves 7 arrays up and 3 down, as it always has.
#ifndef LYRA_BRIDGE_STAGING_H_
#define LYRA_BRIDGE_STAGING_H_

#include <algorithm>
#include <cstddef>

namespace bridge_staging {

enum Kind { FULL, SPEAKERS, SHARED };   // lyra_hip_bridge_begin, lyra_hip_speakers_begin, lyra_hip_shared_begin

constexpr size_t PACKET_BYTES = 23;     // LYRA_HIP_MAX_PACKET_BYTES
constexpr size_t NONE = ~(size_t)0;     // an array this kind of tick does not have

struct Layout {
  // going up, int32 [B] each unless noted
  size_t ids = 0, packet_bytes = NONE, order = NONE, muted = NONE;
  size_t room_start = NONE;                      // [B + 1]
  size_t num_bits = NONE, dtx = NONE;            // FULL, SPEAKERS: per listener
  size_t room_keys = NONE;                       // SHARED
  size_t enc_ids = NONE, enc_bits = NONE, enc_dtx = NONE;   // SHARED: [E] each
  size_t in_packets = NONE;                      // bytes [B][23], at this WORD offset
  size_t in_bytes = 0;                           // the upload
  // coming down, int32 [B] each unless noted
  size_t out_packet_bytes = 0, is_noise = NONE, is_comfort_noise = NONE;
  size_t is_speaker = NONE;                      // SPEAKERS, SHARED
  size_t levels = NONE;                          // SPEAKERS, SHARED: int64 [B], at 16 * B bytes: 8-byte aligned
  size_t slot_of = NONE;                         // SHARED
  size_t out_packets = NONE;                     // bytes [B][23], at this WORD offset
  size_t out_bytes = 0;                          // the download
};

// B rows; E encoder rows of a SHARED tick (ignored otherwise)
inline Layout layout(Kind kind, size_t B, size_t E) {
  Layout L;
  L.packet_bytes = B;
  L.order = 2 * B;
  L.muted = 3 * B;
  L.room_start = 4 * B;
  size_t w = 5 * B + 1;
  if (kind == SHARED) {
    L.room_keys = w;
    L.enc_ids = w + B;
    L.enc_bits = L.enc_ids + E;
    L.enc_dtx = L.enc_bits + E;
    w = L.enc_dtx + E;
  } else {
    L.num_bits = w;
    L.dtx = w + B;
    w += 2 * B;
  }
  L.in_packets = w;
  L.in_bytes = w * 4 + B * PACKET_BYTES;
  L.is_noise = B;
  L.is_comfort_noise = 2 * B;
  w = 3 * B;
  if (kind != FULL) {
    L.is_speaker = 3 * B;
    L.levels = 4 * B;
    w = 6 * B;
  }
  if (kind == SHARED) {
    L.slot_of = 6 * B;
    w = 7 * B;
  }
  L.out_packets = w;
  L.out_bytes = w * 4 + B * PACKET_BYTES;
  return L;
}

// What a slot holds: the largest tick of any kind a context of max_streams can begin (B = E = max_streams).
inline size_t slot_in_bytes(size_t max_streams) {
  return std::max(layout(FULL, max_streams, 0).in_bytes, layout(SHARED, max_streams, max_streams).in_bytes);
}
inline size_t slot_out_bytes(size_t max_streams) { return layout(SHARED, max_streams, max_streams).out_bytes; }

}  // namespace bridge_staging
#endif  // LYRA_BRIDGE_STAGING_H_
