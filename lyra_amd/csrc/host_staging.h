// host_staging.h -- host-only: where every array of a request lies in the staging slot (HostSlot, api.hip) of each pipelined
// host-buffer form (pipelines.h), shared by api.hip and a plain compiler (tests/host_staging/host_staging_test.cc).  A slot
// has four runs of bytes: pinned h_in / h_out, device d_in / d_out.  All offsets here are in BYTES from the start of a run;
// `room` is what a slot must hold.  The bridge's ticks are laid out by bridge_staging.h (in 4-byte words); this header adds
// the room of their slot.
// Two shapes:
//   - one copy per direction (decode_streams, decode_samples_streams, the bridge): the device run is the pinned run, byte for
//     byte, so an array has ONE offset and the arrays lie n rows apart, n the rows of the request;
//   - one copy per array (encode, decode, decode_samples, decode_samples_any, encode_streams): every array that is copied or
//     handed to a kernel on its own starts on a 256-byte boundary of the device run (kernels read PCM and packets with 16-byte
//     vector loads), m = max_streams rows apart, and has a separate offset in the pinned run.
#ifndef LYRA_HOST_STAGING_H_
#define LYRA_HOST_STAGING_H_

#include <cstddef>

#include "bridge_staging.h"

namespace host_staging {

constexpr size_t ALIGN = 256;            // of every carved device sub-buffer
constexpr size_t PACKET_BYTES = 23;      // LYRA_HIP_MAX_PACKET_BYTES
constexpr size_t PACKET_ROOM = 24;       // per stream where packets of a uniform size are staged (the packet rows' room)
constexpr size_t HOP16 = 320;            // samples of a hop at 16 kHz
constexpr size_t MAX_EXT_HOP = 960;      // LYRA_HIP_MAX_EXT_HOP: ... at 48 kHz
constexpr size_t MAX_HOPS = 4;           // LYRA_HIP_DECODE_SAMPLES_MAX_HOPS

inline size_t aligned(size_t bytes) { return (bytes + ALIGN - 1) / ALIGN * ALIGN; }

struct Room { size_t h_in = 0, h_out = 0, d_in = 0, d_out = 0; };

// lyra_hip_encode_begin / _end; m = max_streams.  The audio goes up from the caller's memory, not through h_in.
struct Encode {
  size_t h_ids = 0;                                   // h_in:  int32 [m]
  size_t h_packets = 0, h_packet_bytes = 0;           // h_out: [m][24] | int32 [m]
  size_t d_ids = 0, d_pcm = 0, d_pcm16 = 0;           // d_in:  int32 [m] | int16 [m][960] external rate | int16 [m][320] resampled
  size_t d_packets = 0, d_packet_bytes = 0;           // d_out: [m][24] | int32 [m]
  Room room;
};
inline Encode encode(size_t m) {
  Encode L;
  L.h_packet_bytes = m * PACKET_ROOM;
  L.d_pcm = aligned(m * 4);
  L.d_pcm16 = L.d_pcm + aligned(m * MAX_EXT_HOP * 2);
  L.d_packet_bytes = aligned(m * PACKET_ROOM);
  L.room = {m * 4, L.h_packet_bytes + m * 4, L.d_pcm16 + m * HOP16 * 2, L.d_packet_bytes + m * 4};
  return L;
}

// lyra_hip_decode_begin / _end; m = max_streams.  The samples go down into the caller's memory: no h_out.
struct Decode {
  size_t h_ids = 0, h_packets = 0;                    // h_in:  int32 [m] | [m][24]
  size_t d_ids = 0, d_packets = 0;                    // d_in:  the same
  size_t d_pcm = 0;                                   // d_out: int16 [m][320]
  Room room;
};
inline Decode decode(size_t m) {
  Decode L;
  L.h_packets = m * 4;
  L.d_packets = aligned(m * 4);
  L.room = {L.h_packets + m * PACKET_ROOM, 0, L.d_packets + m * PACKET_ROOM, m * HOP16 * 2};
  return L;
}

// lyra_hip_decode_samples_begin / _end (hops = 1) and lyra_hip_decode_samples_any_begin / _end (hops = MAX_HOPS); m = max_streams
struct DecodeSamples {
  size_t h_ids = 0, h_packet_bytes = 0, h_packets = 0;   // h_in:  int32 [m] | int32 [m] | [m][24]
  size_t d_ids = 0, d_packet_bytes = 0, d_packets = 0;   // d_in:  the same
  size_t d_pcm = 0;                                      // d_out: int16 [m][hops * 960]
  Room room;
};
inline DecodeSamples decode_samples(size_t m, size_t hops) {
  DecodeSamples L;
  L.h_packet_bytes = m * 4;
  L.h_packets = m * 8;
  L.d_packet_bytes = aligned(m * 4);
  L.d_packets = 2 * aligned(m * 4);
  L.room = {L.h_packets + m * PACKET_ROOM, 0, L.d_packets + m * PACKET_ROOM, m * hops * MAX_EXT_HOP * 2};
  return L;
}

// lyra_hip_encode_streams_begin / _end; n rows of m = max_streams.  The five int32 arrays go up as one run (`meta`, n rows
// apart, the same on the device); the audio goes up from the caller's memory.
struct EncodeStreams {
  size_t ids = 0, rates = 0, bits = 0, dtx = 0, offsets = 0, meta_bytes = 0;   // inside h_in and inside d_in + d_meta
  size_t d_meta = 0, d_pcm = 0;                       // d_in:  the run | int16 [m * 960] packed
  size_t h_packets = 0, h_packet_bytes = 0;           // h_out: [m][23], 24 per stream in total | int32 [m]
  size_t d_packets = 0, d_packet_bytes = 0;           // d_out: [m][23] | int32 [m]
  Room room;
};
inline EncodeStreams encode_streams(size_t n, size_t m) {
  EncodeStreams L;
  L.rates = n * 4;
  L.bits = n * 8;
  L.dtx = n * 12;
  L.offsets = n * 16;
  L.meta_bytes = n * 20;
  L.d_pcm = aligned(m * 20);
  L.h_packet_bytes = m * PACKET_ROOM;
  L.d_packet_bytes = aligned(m * PACKET_BYTES);
  L.room = {m * 20, L.h_packet_bytes + m * 4, L.d_pcm + m * MAX_EXT_HOP * 2, L.d_packet_bytes + m * 4};
  return L;
}

// lyra_hip_decode_streams_begin / _end; n rows of m = max_streams.  One copy per direction.
struct DecodeStreams {
  size_t ids = 0, packet_bytes = 0, rates = 0, offsets = 0, packets = 0, in_bytes = 0;   // going up: 4 x int32 [n] | [n][23]
  size_t is_noise = 0, is_comfort_noise = 0, pcm = 0;   // coming down: 2 x int32 [n] | the packed samples (the download: pcm + 2 per sample)
  Room room;
};
inline DecodeStreams decode_streams(size_t n, size_t m) {
  DecodeStreams L;
  L.packet_bytes = n * 4;
  L.rates = n * 8;
  L.offsets = n * 12;
  L.packets = n * 16;
  L.in_bytes = L.packets + n * PACKET_BYTES;
  L.is_comfort_noise = n * 4;
  L.pcm = n * 8;
  const size_t in = m * (16 + PACKET_BYTES), out = m * (8 + MAX_EXT_HOP * 2);
  L.room = {in, out, in, out};
  return L;
}

// lyra_hip_decode_samples_streams_begin / _end; n rows, and the room is for n rows: the slot grows with the request.
struct DecodeSamplesStreams {
  size_t ids = 0, packet_bytes = 0, rates = 0, sizes = 0, offsets = 0, packets = 0, in_bytes = 0;   // 5 x int32 [n] | [n][23]
  size_t is_noise = 0, is_comfort_noise = 0, pcm = 0;   // as DecodeStreams
  Room room;
};
inline DecodeSamplesStreams decode_samples_streams(size_t n) {
  DecodeSamplesStreams L;
  L.packet_bytes = n * 4;
  L.rates = n * 8;
  L.sizes = n * 12;
  L.offsets = n * 16;
  L.packets = n * 20;
  L.in_bytes = L.packets + n * PACKET_BYTES;
  L.is_comfort_noise = n * 4;
  L.pcm = n * 8;
  const size_t out = n * (8 + MAX_HOPS * MAX_EXT_HOP * 2);
  L.room = {L.in_bytes, out, L.in_bytes, out};
  return L;
}

// the three kinds of bridge tick (bridge_staging::layout): the largest tick of any kind a context of m streams can begin
inline Room bridge(size_t m) {
  const size_t in = bridge_staging::slot_in_bytes(m), out = bridge_staging::slot_out_bytes(m);
  return {in, out, in, out};
}

}  // namespace host_staging
#endif  // LYRA_HOST_STAGING_H_
