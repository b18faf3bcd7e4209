// pipelines.h -- the pipelined host-buffer forms of the C ABI (a `_begin` that enqueues, an `_end` that hands the oldest
// result over) and which of them may be in flight together.  Plain C++: tests/test_pipeline_exclusion_cpu.py compiles this
// header with the host compiler and prints the table.  The counters are lyra_hip_ctx::pl_begun / pl_ended, the checks
// pl_admit and pl_any_in_flight, the staging of the requests in flight lyra_hip_ctx::pl_slot (api.hip; host_staging.h).
#pragma once

namespace lyra {

enum Pipeline {
  PL_ENCODE,                   // lyra_hip_encode_begin
  PL_DECODE,                   // lyra_hip_decode_begin
  PL_TWIN_FETCH,               // lyra_hip_twin_fetch_begin
  PL_ENCODE_STREAMS,           // lyra_hip_encode_streams_begin
  PL_DECODE_STREAMS,           // lyra_hip_decode_streams_begin
  PL_DECODE_SAMPLES,           // lyra_hip_decode_samples_begin
  PL_DECODE_SAMPLES_ANY,       // lyra_hip_decode_samples_any_begin
  PL_DECODE_SAMPLES_STREAMS,   // lyra_hip_decode_samples_streams_begin
  PL_BRIDGE,                   // lyra_hip_bridge_begin / speakers_begin / shared_begin: one pipeline, three kinds of tick
  PL_COUNT
};

constexpr int PL_DEPTH = 2;    // requests of one pipeline in flight at most

constexpr const char* PL_NAME[PL_COUNT] = {"encode", "decode", "twin_fetch", "encode_streams", "decode_streams",
                                           "decode_samples", "decode_samples_any", "decode_samples_streams", "bridge"};
// what each pipeline's end() calls a request in its refusal "..._end: no <noun> in flight": the wordings the families grew
// up with, which callers and the host classes' fakes know
constexpr const char* PL_IN_FLIGHT_NOUN[PL_COUNT] = {"call", "call", "request", "call", "call", "request", "request", "request", "tick"};

// PL_EXCLUDES[p][o]: p's begin() is refused while a request of o is in flight.  The two encode pipelines share the encode-side
// streams' order, the decode pipelines the decode-side streams', a bridge tick runs on both sides' streams.
// decode <-> decode_samples is NOT excluded: allowed today, not known to be intended.
// lyra_hip_twin_fetch_begin checks its own depth only (it does not consult its row: a fetch begun under a bridge tick is accepted).
constexpr bool PL_EXCLUDES[PL_COUNT][PL_COUNT] = {
    //              enc dec twf es  dst ds  dsa dss brg
    /* encode  */ {0, 0, 0, 1, 0, 0, 0, 0, 1},
    /* decode  */ {0, 0, 0, 0, 1, 0, 1, 1, 1},
    /* twin_f  */ {0, 0, 0, 0, 0, 0, 0, 0, 1},
    /* enc_str */ {1, 0, 0, 0, 0, 0, 0, 0, 1},
    /* dec_str */ {0, 1, 0, 0, 0, 1, 1, 1, 1},
    /* ds      */ {0, 0, 0, 0, 1, 0, 1, 1, 1},
    /* ds_any  */ {0, 1, 0, 0, 1, 1, 0, 1, 1},
    /* ds_strm */ {0, 1, 0, 0, 1, 1, 1, 0, 1},
    /* bridge  */ {1, 1, 1, 1, 1, 1, 1, 1, 0},
};

}  // namespace lyra
