// bridge_spans_kernels.h -- the kernels of bridge_spans_kernels.hip (include/lyra_hip_bridge_spans.h, bridge_spans_api.inc):
// the conference bridge's mix as one pass over all ticks of a recording.  Participant p's tick t is buffer frame
// first[p] + t; order / room_start are the membership index over participant numbers, built and checked by the library
// (bridge_spans_plan.h), so no entry is counted as bad here; ticks t0 .. t0 + n_ticks - 1 are one slab of the pass.
#pragma once
#include "kernels.h"

namespace lyra {

// full mix: one wavefront per (room, tick)
__global__ void bridge_spans_mix_kernel(const int16_t* pcm, const long long* first, const int32_t* order,
                                        const int32_t* room_start, int n_rooms, long long t0, int n_ticks, const int32_t* muted,
                                        const int32_t* is_cn, int16_t* mix);
// one wavefront per (participant in no room, tick): the frame's mix row is zeroed
__global__ void bridge_spans_zero_kernel(const long long* first, const int32_t* lone, int n_lone, long long t0, int n_ticks,
                                         int16_t* mix);
// loudest-N, stage 1: one wavefront per (participant, tick): the frame's level into lv[tick in slab][P] (and levels[frame]
// where given), is_speaker[frame] = 0 where given, and zeros for the mix row of a participant in no room
__global__ void bridge_spans_level_kernel(const int16_t* pcm, const long long* first, const int32_t* part_room, int P,
                                          long long t0, int n_ticks, long long* lv, long long* levels, int16_t* mix,
                                          int32_t* is_speaker);
// stage 2: one wavefront per (room, tick): the room's max_speakers loudest candidates, as participant numbers, into
// spk[tick in slab][room][8] (-1 padded); is_speaker[frame] = 1 where given.  keys: [ticks of the slab][n_members], rooms > 64
__global__ void bridge_spans_select_kernel(const long long* lv, const long long* first, const int32_t* order,
                                           const int32_t* room_start, int n_rooms, int n_members, int P, long long t0,
                                           int n_ticks, const int32_t* muted, const int32_t* is_cn, int max_speakers,
                                           unsigned long long* keys, int32_t* spk, int32_t* is_speaker);
// stage 3: one wavefront per (8 consecutive positions of the index, tick)
__global__ void bridge_spans_speakers_mix_kernel(const int16_t* pcm, const long long* first, const int32_t* order, int n_members,
                                                 const int32_t* pos_room, int n_rooms, long long t0, int n_ticks,
                                                 const int32_t* spk, int16_t* mix);

}  // namespace lyra
