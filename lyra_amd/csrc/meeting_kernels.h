// meeting_kernels.h -- the kernels of meeting_kernels.hip (include/lyra_hip_spans_meeting.h, meeting_api.inc): the conference
// bridge's mix over a meeting with a schedule, table-driven.  The host cuts the meeting into epochs of constant membership
// (meeting_plan.h) and those into pieces that fit a launch; MeetEpoch is one piece.  One launch per stage covers every
// (piece, unit, tick) of a slab of pieces [e_lo, e_hi): a wavefront finds its piece by a binary search over the prefix sums
// wave0[kind], then its unit and tick inside it.  An entry is one participant present in one epoch: on meeting tick t its
// frame is base[entry] + t.  The entries of an epoch's rooms come first, room-contiguous (room_start holds positions inside
// the epoch), then the present participants in no room (room[entry] = -1).  The index is the library's own, built and checked
// on the host: nothing here counts bad entries.
#pragma once
#include "kernels.h"

namespace lyra {

enum { MEET_ROOMS = 0, MEET_LONE = 1, MEET_ENTRIES = 2, MEET_CHUNKS = 3 };   // what a launch's wavefronts are counted in

struct MeetEpoch {
  long long wave0[4];   // the piece's first wavefront in a launch over rooms / participants in no room / entries / chunks of 8
                        // members, each times ticks, counted from the table's first piece
  long long tick0;      // first meeting tick
  long long sel;        // byte offset of the piece's selection scratch in the slab's: levels [ticks][n_entries] int64 |
                        // speaker lists [ticks][n_rooms][8] int32 | keys [ticks][n_members] uint64 (big only)
  int n_ticks;
  int entry0;           // offset into base / room
  int n_entries, n_members;
  int room0;            // offset into room_start (n_rooms + 1 values)
  int n_rooms;
  int big;              // a room above 64 members: the selection parks its keys
  int pad;
};

// full mix: one wavefront per (room, tick)
__global__ void meeting_mix_kernel(const MeetEpoch* tab, int e_lo, int e_hi, long long n_waves, const int16_t* pcm,
                                   const long long* base, const int32_t* room_start, const int32_t* muted, const int32_t* is_cn,
                                   int16_t* mix);
// one wavefront per (present participant in no room, tick): the frame's mix row is zeroed
__global__ void meeting_zero_kernel(const MeetEpoch* tab, int e_lo, int e_hi, long long n_waves, const long long* base,
                                    int16_t* mix);
// loudest-N, stage 1: one wavefront per (entry, tick): the frame's level into the piece's levels (and levels[frame] where
// given), is_speaker[frame] = 0 where given, and zeros for the mix row of a participant in no room
__global__ void meeting_level_kernel(const MeetEpoch* tab, int e_lo, int e_hi, long long n_waves, const int16_t* pcm,
                                     const long long* base, const int32_t* room, unsigned char* sel, long long* levels,
                                     int16_t* mix, int32_t* is_speaker);
// stage 2: one wavefront per (room, tick): the room's max_speakers loudest candidates, as positions inside the epoch, into
// the piece's speaker lists (-1 padded); is_speaker[frame] = 1 where given
__global__ void meeting_select_kernel(const MeetEpoch* tab, int e_lo, int e_hi, long long n_waves, const long long* base,
                                      const int32_t* room_start, const int32_t* muted, const int32_t* is_cn, int max_speakers,
                                      unsigned char* sel, int32_t* is_speaker);
// stage 3: one wavefront per (8 consecutive member positions of the epoch, tick)
__global__ void meeting_speakers_mix_kernel(const MeetEpoch* tab, int e_lo, int e_hi, long long n_waves, const int16_t* pcm,
                                            const long long* base, const int32_t* room, const unsigned char* sel, int16_t* mix);

}  // namespace lyra
