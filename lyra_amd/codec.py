"""Python mirror of the reference plugin surface over the C ABI (include/lyra_hip.h).

Batched, array-in/array-out versions of
  FeatureExtractorInterface::Extract            lyra/feature_extractor_interface.h:32-39
  VectorQuantizerInterface::Quantize / DecodeToLossyFeatures
                                                lyra/vector_quantizer_interface.h:28-41
  GenerativeModelInterface::AddFeatures / GenerateSamples
                                                lyra/generative_model_interface.h:32-42
with the same names, argument meaning and error behaviour (None on failure, like std::nullopt), plus the
fused LyraEncoder::Encode / LyraDecoder::DecodeSamples steady-state path.  numpy arrays go through the
host-pointer entry points; torch CUDA tensors through the `_dev` ones (no copies, no sync).
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HOP = 320
NUM_FEATURES = 64
NUM_MEL = 160
MAX_BITS = 184

_BITRATES = {3200: 64, 6000: 120, 9200: 184}  # lyra_config.cc:44-48


def bitrate_to_num_bits(bitrate):
    return _BITRATES[bitrate]


def packet_size(num_bits):
    return (num_bits + 7) // 8  # lyra_config.h: 8 / 15 / 23 bytes


MAX_PACKET_BYTES = 23  # LYRA_HIP_MAX_PACKET_BYTES: packet row stride of the mixed-bitrate calls
MAX_EXT_HOP = 960      # LYRA_HIP_MAX_EXT_HOP: row stride (samples) of external-rate audio in the per-stream-rate calls


def library_path():
    # LYRA_HIP_LIB: developer override used to A/B kernel variants on the GPU box
    return os.environ.get("LYRA_HIP_LIB") or os.path.join(HERE, "liblyra_hip.so")


def default_model_dir():
    return os.path.join(HERE, "assets")


def build_library(force=False):
    """Compile lyra_amd/csrc for gfx950 (hipcc cross-compiles without a GPU)."""
    src = os.path.join(HERE, "csrc")
    args = ["make", "-C", src, "-j8"] + (["-B"] if force else [])
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return library_path()


class LyraHipError(RuntimeError):
    pass


class StepsDesc(C.Structure):
    """lyra_hip_steps (include/lyra_hip.h): many hops of B streams from one call."""
    _fields_ = [("d_stream_ids", C.c_void_p), ("B", C.c_int), ("num_bits", C.c_int), ("flags", C.c_uint),
                ("first_step", C.c_long), ("n_steps", C.c_int), ("ring", C.c_int), ("d_pcm_ring", C.c_void_p),
                ("d_packets", C.c_void_p * 2), ("d_packet_bytes", C.c_void_p * 2), ("d_pcm_out", C.c_void_p * 2),
                ("d_features", C.c_void_p), ("n_features", C.c_int), ("d_packet_ring", C.c_void_p), ("n_packet_ring", C.c_int), ("d_is_noise", C.c_void_p), ("external_rate", C.c_int),
                ("d_ext_out", C.c_void_p * 2),
                # read by the library only with STEP_PACKET_LOSS
                ("d_received_ring", C.c_void_p), ("n_received_ring", C.c_int), ("d_is_comfort_noise", C.c_void_p),
                # read by the library only with STEP_MIXED_BITRATE
                ("d_bits_ring", C.c_void_p), ("n_bits_ring", C.c_int)]


class StepsDescRates(C.Structure):
    """lyra_hip_steps_rates: lyra_hip_steps with d_rates behind it, read by the library only with STEP_MIXED_RATE."""
    _fields_ = [("steps", StepsDesc), ("d_rates", C.c_void_p)]


STEP_ENCODE, STEP_DECODE, STEP_DTX, STEP_DECODER_NOISE = 1, 2, 4, 8
STEP_PACKET_LOSS = 16
STEP_MIXED_BITRATE = 32
STEP_MIXED_RATE = 64


_libs = {}


# lyra_hip_span / lyra_hip_span_chunk (include/lyra_hip.h) as numpy record types
SPAN_DTYPE = np.dtype([("stream_id", "<i4"), ("first_frame", "<i8"), ("n_frames", "<i8")], align=True)
SPAN_CHUNK_DTYPE = np.dtype([("stream_id", "<i4"), ("span", "<i4"), ("first_frame", "<i8"), ("n_frames", "<i4"),
                             ("n_warmup", "<i4"), ("phase_offset", "<i4"), ("last", "<i4")], align=True)
SIDES = {"encoder": 0, "decoder": 1}


def _spans(spans):
    """[(stream_id, first_frame, n_frames), ...] or a SPAN_DTYPE array -> contiguous SPAN_DTYPE array"""
    if isinstance(spans, np.ndarray) and spans.dtype == SPAN_DTYPE:
        return np.ascontiguousarray(spans)
    return np.array([tuple(int(v) for v in s) for s in spans], SPAN_DTYPE).reshape(-1)


def span_warmup_frames(side, lib=None):
    """Hops a fresh stream replays before its state equals the sequential stream's (lyra_hip_span_warmup_frames)."""
    return (lib or _load()).lyra_hip_span_warmup_frames(SIDES[side])


def spans_plan(side, spans, lane_ids, max_streams, lib=None):
    """The planner of encode_spans / decode_spans (lyra_hip_spans_plan; no GPU): (chunks as a SPAN_CHUNK_DTYPE array in
    batch-row order, number of steps).  LyraHipError for what the calls refuse."""
    L = lib or _load()
    sp = _spans(spans)
    lanes = np.ascontiguousarray(np.asarray(lane_ids, np.int32).reshape(-1))
    chunks = np.zeros(sp.size + lanes.size + 1, SPAN_CHUNK_DTYPE)
    steps = C.c_int(0)
    n = L.lyra_hip_spans_plan(SIDES[side], sp.ctypes.data, sp.size, lanes.ctypes.data, lanes.size, int(max_streams),
                              chunks.ctypes.data, chunks.size, C.addressof(steps))
    if n < 0:
        raise LyraHipError("lyra_hip_spans_plan: invalid spans or lanes")
    return chunks[:n], steps.value


def spans_packed_layout(spans, sample_rates, lib=None):
    """The back-to-back layout of the packed span calls (lyra_hip_spans_packed_layout; no GPU): (ext_offsets int64 [n_spans],
    total samples).  Span s takes n_frames * sample_rates[s] / 50 samples from ext_offsets[s]; a span of no frames takes nothing.
    LyraHipError for a rate that is none of 8000 / 16000 / 32000 / 48000 or a negative frame count."""
    L = lib or _load()
    sp = _spans(spans)
    rates = np.ascontiguousarray(np.asarray(sample_rates, np.int32).reshape(-1))
    if rates.size != sp.size:
        raise LyraHipError(f"spans: sample_rates has {rates.size} entries for {sp.size} spans")
    offsets = np.zeros(sp.size, np.int64)
    total = L.lyra_hip_spans_packed_layout(sp.ctypes.data, sp.size, rates.ctypes.data, offsets.ctypes.data)
    if total < 0:
        raise LyraHipError("lyra_hip_spans_packed_layout: invalid spans or sample rates")
    return offsets, int(total)


SPAN_LOSSY_COUNTS_DTYPE = np.dtype([("n_gen", "<i8"), ("n_received", "<i8"), ("n_cng", "<i8"), ("n_versions", "<i8"),
                                    ("ctl_out", "<u4"), ("reserved", "<i4")], align=True)


def spans_lossy_plan(spans, packet_bytes, packet_size_bytes, ctl_in, lane_ids, max_streams, lib=None):
    """The planner of decode_spans_lossy (lyra_hip_spans_lossy_plan; no GPU).  packet_bytes int32 [frames] (0 = no packet),
    ctl_in: the span streams' control words on entry.  Returns a dict: counts (SPAN_LOSSY_COUNTS_DTYPE per span), the dense lists
    gen_frames, gen_received, rx_frames, cng_frames, cng_versions, versions, info (span after span), chunks (SPAN_CHUNK_DTYPE,
    first_frame counting in gen_frames) and n_steps.  LyraHipError for what the call refuses."""
    return _spans_lossy_plan(spans, packet_bytes, int(packet_size_bytes), ctl_in, lane_ids, max_streams, lib)


def spans_lossy_plan_mixed(spans, packet_bytes, ctl_in, lane_ids, max_streams, lib=None):
    """The planner of decode_spans_lossy_mixed (lyra_hip_spans_lossy_plan_mixed; no GPU): spans_lossy_plan with a size per frame,
    0 / 8 / 15 / 23.  The same dict, except that gen_bytes takes the place of gen_received: 0 for a concealed tick, else the size
    of the packet the tick is fed from."""
    return _spans_lossy_plan(spans, packet_bytes, None, ctl_in, lane_ids, max_streams, lib)


def _spans_lossy_plan(spans, packet_bytes, packet_size_bytes, ctl_in, lane_ids, max_streams, lib):
    """packet_size_bytes None: the mixed form"""
    mixed = packet_size_bytes is None
    rx_key, what = ("gen_bytes", "spans_lossy_plan_mixed") if mixed else ("gen_received", "spans_lossy_plan")
    L = lib or _load()
    sp = _spans(spans)
    lanes = np.ascontiguousarray(np.asarray(lane_ids, np.int32).reshape(-1))
    pb = np.ascontiguousarray(np.asarray(packet_bytes, np.int32).reshape(-1))
    ctl = np.ascontiguousarray(np.asarray(ctl_in, np.uint32).reshape(-1))
    if ctl.size != sp.size:
        raise LyraHipError(f"{what}: one control word per span")
    if sp.size and (np.any(sp["first_frame"] < 0) or np.any(sp["n_frames"] < 0) or
                    int(np.max(sp["first_frame"] + sp["n_frames"])) > pb.size):
        raise LyraHipError(f"{what}: a span lies outside the {pb.size} frames of packet_bytes")
    T = int(sp["n_frames"].sum()) if sp.size else 0
    counts = np.zeros(max(sp.size, 1), SPAN_LOSSY_COUNTS_DTYPE)
    out = {k: np.zeros(max(T, 1), d) for k, d in (("gen_frames", np.int64), (rx_key, np.uint8), ("rx_frames", np.int64),
                                                    ("cng_frames", np.int64), ("cng_versions", np.int32), ("versions", np.int32),
                                                    ("info", np.int32))}
    chunks = np.zeros(sp.size + lanes.size + 1, SPAN_CHUNK_DTYPE)
    steps = C.c_int(0)
    fn = L.lyra_hip_spans_lossy_plan_mixed if mixed else L.lyra_hip_spans_lossy_plan
    n = fn(sp.ctypes.data, sp.size, lanes.ctypes.data, lanes.size, int(max_streams), pb.ctypes.data,
           *(() if mixed else (packet_size_bytes,)), ctl.ctypes.data, counts.ctypes.data,
           *(out[k].ctypes.data for k in ("gen_frames", rx_key, "rx_frames", "cng_frames", "cng_versions", "versions", "info")),
           chunks.ctypes.data, chunks.size, C.addressof(steps))
    if n < 0:
        raise LyraHipError(f"lyra_hip_{what}: invalid spans, lanes or packet sizes")
    counts = counts[:sp.size]
    size = {"gen_frames": "n_gen", rx_key: "n_gen", "rx_frames": "n_received", "cng_frames": "n_cng",
            "cng_versions": "n_cng", "versions": "n_versions"}
    res = {k: v[:int(counts[size[k]].sum())] for k, v in out.items() if k in size}
    res.update(info=out["info"][:T], counts=counts, chunks=chunks[:n], n_steps=steps.value)
    return res


def _signatures():
    """name -> (restype, argtypes) of every function of include/lyra_hip.h this module binds; tests/test_abi_cpu.py holds
    each entry to its prototype."""
    vp, ci, cp, cl, cu, sz = C.c_void_p, C.c_int, C.c_char_p, C.c_long, C.c_uint, C.c_size_t
    hop = [vp, vp, ci]             # ctx, stream ids, B
    spans = [vp, vp, ci, vp, ci]   # ctx, spans, n_spans, lane ids, n_lanes
    ints = {   # return int
        "create": [cp, ci, ci, ci, C.POINTER(vp)], "create_from_image": [cp, sz, ci, ci, ci, C.POINTER(vp)],
        "reset_streams": hop, "noise_estimate": [vp, ci, vp, ci, vp],
        "set_cng_seed": [vp, C.c_uint64], "set_encoder_sample_rate": [vp, ci],
        "encode_begin": hop + [vp, ci, ci, ci], "encode_end": [vp, vp, vp],
        "decode_begin": hop + [vp, ci], "decode_end": [vp, vp],
        "twin_fetch_begin": [vp, ci, ci, ci], "twin_fetch_end": [vp, vp],
        "encode_ext_dev": hop + [vp, ci, ci, ci, vp, vp], "decode_ext_dev": hop + [vp, ci, ci, ci, vp, vp, vp],
        "decode_lossy_dev": hop + [vp, vp, ci, ci, vp, vp, vp, vp],
        "encode_mixed_dev": hop + [vp, ci, vp, ci, vp, vp], "decode_lossy_mixed_dev": hop + [vp, vp, ci, vp, vp, vp, vp],
        "encode_rates_dev": hop + [vp, vp, vp, ci, vp, vp], "decode_lossy_rates_dev": hop + [vp] * 7,
        "decode_samples_dev": hop + [vp, vp, ci, ci, vp, vp, vp],
        "span_warmup_frames": [ci], "spans_plan": [ci, vp, ci, vp, ci, ci, vp, ci, vp],
        "spans_lossy_plan": [vp, ci, vp, ci, ci, vp, ci, vp] + [vp] * 8 + [vp, ci, vp],
        "encode_spans_ext": spans + [vp, ci, ci, vp], "decode_spans_ext": spans + [vp, ci, ci, vp],
        "encode_spans_ext_dev": spans + [vp, ci, vp, ci, vp], "decode_spans_ext_dev": spans + [vp, ci, ci, vp, vp],
        "encode_spans_dtx": spans + [vp, ci, ci, vp, vp], "encode_spans_dtx_dev": spans + [vp, ci, vp, ci, vp, vp],
        "run_steps_dev": [vp, C.POINTER(StepsDesc)], "synchronize": [vp], "wait_for_stream": [vp, vp], "stream_wait": [vp, vp],
        "set_serial": [vp, ci], "set_stream_priorities": [vp, ci, ci, ci], "max_streams": [vp],
        "profile_enable": [vp, cu], "profile_sample": [vp, ci], "profile_kernel_count": [], "profile_read": [vp, vp, vp],
    }
    twins = {   # return int; NAME on host buffers and NAME_dev on device buffers share the signature
        "extract": hop + [vp, vp], "generate": hop + [vp, vp], "logmel": hop + [vp, vp], "comfort_noise": hop + [vp, vp],
        "rvq_encode": [vp, ci, vp, ci, vp], "rvq_decode": [vp, ci, vp, vp],
        "encode": hop + [vp, ci, vp], "decode": hop + [vp, ci, vp], "encode_dtx": hop + [vp, ci, vp, vp],
        "noise_receive": [vp, ci, vp, ci, vp, vp], "resample": [vp, ci, vp, ci, vp, ci, ci, ci, vp],
        "export_streams": hop + [vp], "import_streams": hop + [vp, cu],
        "encode_spans": spans + [vp, ci, vp], "decode_spans": spans + [vp, ci, vp],
        "noise_spans": [vp, ci, vp, ci, vp, vp], "decode_spans_lossy": spans + [vp, vp, ci, ci, vp, vp, vp, vp],
    }
    table = {
        "destroy": (None, [vp]), "last_error": (cp, [vp]), "profile_kernel_name": (cp, [ci]),
        "stream_blob_bytes": (sz, []), "state_bytes_per_stream": (sz, []), "debug_read": (cl, [vp, ci, vp, cl]),
    }
    table.update({name: (vp, [vp]) for name in ("stream", "stream_decode", "stream_quantizer")})
    table.update({name + "_errors": (cl, [vp, ci])
                  for name in ("decode_lossy", "encode_mixed", "rates", "decode_samples", "import")})
    table.update({name: (ci, args) for name, args in ints.items()})
    table.update({name + suf: (ci, args) for name, args in twins.items() for suf in ("", "_dev")})
    return {"lyra_hip_" + name: sig for name, sig in table.items()}


_SIGNATURES = _signatures()


def _signatures_spans_mixed():
    """The same for include/lyra_hip_spans_mixed.h (tests/test_spans_mixed_cpu.py holds each entry to its prototype)."""
    vp, ci = C.c_void_p, C.c_int
    spans = [vp, vp, ci, vp, ci]   # ctx, spans, n_spans, lane ids, n_lanes
    table = {
        "encode_spans_mixed_dev": spans + [vp, ci, vp, vp, ci, vp, vp], "encode_spans_mixed": spans + [vp, ci, vp, ci, vp, vp],
        "decode_spans_lossy_mixed_dev": spans + [vp, vp, ci, vp, vp, vp, vp],
        "decode_spans_lossy_mixed": spans + [vp, vp, ci, vp, vp, vp, vp],
        "spans_lossy_plan_mixed": [vp, ci, vp, ci, ci, vp, vp] + [vp] * 8 + [vp, ci, vp],
    }
    return {"lyra_hip_" + name: (ci, args) for name, args in table.items()}


_SIGNATURES_SPANS_MIXED = _signatures_spans_mixed()


def _signatures_spans_rates():
    """The same for include/lyra_hip_spans_rates.h (tests/test_spans_rates_cpu.py holds each entry to its prototype)."""
    vp, ci = C.c_void_p, C.c_int
    spans = [vp, vp, ci, vp, ci]   # ctx, spans, n_spans, lane ids, n_lanes
    table = {
        "encode_spans_rates_dev": spans + [vp, vp, vp, vp, ci, vp, vp], "decode_spans_lossy_rates_dev": spans + [vp] * 7,
        "decode_spans_rates_dev": spans + [vp, ci, vp, vp, vp],
    }
    return {"lyra_hip_" + name: (ci, args) for name, args in table.items()}


_SIGNATURES_SPANS_RATES = _signatures_spans_rates()


def _signatures_spans_packed():
    """The same for include/lyra_hip_spans_packed.h (tests/test_spans_packed_cpu.py holds each entry to its prototype)."""
    vp, ci, ll = C.c_void_p, C.c_int, C.c_longlong
    spans = [vp, vp, ci, vp, ci]   # ctx, spans, n_spans, lane ids, n_lanes
    table = {
        "encode_spans_packed_dev": spans + [vp, ll, vp, vp, vp, vp, ci, vp, vp],
        "decode_spans_lossy_packed_dev": spans + [vp, vp, vp, vp, vp, ll, vp, vp, vp],
        "decode_spans_packed_dev": spans + [vp, ci, vp, vp, vp, ll, vp],
        "encode_spans_packed": spans + [vp, ll, vp, vp, vp, ci, vp, vp],
        "decode_spans_lossy_packed": spans + [vp, vp, vp, vp, vp, ll, vp, vp, vp],
        "decode_spans_packed": spans + [vp, ci, vp, vp, vp, ll, vp],
    }
    table = {"lyra_hip_" + name: (ci, args) for name, args in table.items()}
    table["lyra_hip_spans_packed_layout"] = (ll, [vp, ci, vp, vp])
    return table


_SIGNATURES_SPANS_PACKED = _signatures_spans_packed()


def _signatures_encode_streams():
    """The same for include/lyra_hip_encode_streams.h (tests/test_encode_streams_cpu.py holds each entry to its prototype)."""
    vp, ci, cl = C.c_void_p, C.c_int, C.c_long
    table = {
        "encode_streams_dev": [vp, vp, ci, vp, cl] + [vp] * 6, "encode_streams_begin": [vp, vp, ci] + [vp] * 4,
        "encode_streams_end": [vp, vp, vp],
    }
    return {"lyra_hip_" + name: (ci, args) for name, args in table.items()}


_SIGNATURES_ENCODE_STREAMS = _signatures_encode_streams()


def _signatures_decode_streams():
    """The same for include/lyra_hip_decode_streams.h (tests/test_decode_streams_cpu.py holds each entry to its prototype)."""
    vp, ci, cl = C.c_void_p, C.c_int, C.c_long
    table = {
        "decode_streams_dev": [vp, vp, ci, vp, vp, vp, vp, cl] + [vp] * 4, "decode_streams_begin": [vp, vp, ci] + [vp] * 3,
        "decode_streams_end": [vp] * 4,
    }
    return {"lyra_hip_" + name: (ci, args) for name, args in table.items()}


_SIGNATURES_DECODE_STREAMS = _signatures_decode_streams()


def _signatures_decode_samples_any():
    """The same for include/lyra_hip_decode_samples_any.h (tests/test_decode_samples_any_cpu.py holds each entry to its
    prototype)."""
    vp, ci = C.c_void_p, C.c_int
    table = {
        "decode_samples_any_dev": [vp, vp, ci, vp, vp, ci, ci, vp, vp, vp],
        "decode_samples_any_begin": [vp, vp, ci, vp, vp, ci, ci], "decode_samples_any_end": [vp, vp],
    }
    return {"lyra_hip_" + name: (ci, args) for name, args in table.items()}


_SIGNATURES_DECODE_SAMPLES_ANY = _signatures_decode_samples_any()


def _signatures_decode_samples_streams():
    """The same for include/lyra_hip_decode_samples_streams.h (tests/test_decode_samples_streams_plan_cpu.py holds each entry to
    its prototype)."""
    vp, ci, cl = C.c_void_p, C.c_int, C.c_long
    table = {
        "decode_samples_streams_dev": [vp, vp, ci, vp, vp, vp, vp, ci, vp, cl, vp, vp, vp],
        "decode_samples_streams_begin": [vp, vp, ci] + [vp] * 4, "decode_samples_streams_end": [vp] * 4,
    }
    return {"lyra_hip_" + name: (ci, args) for name, args in table.items()}


_SIGNATURES_DECODE_SAMPLES_STREAMS = _signatures_decode_samples_streams()


class BridgeTick(C.Structure):
    """lyra_hip_bridge_tick (include/lyra_hip_bridge.h)"""
    _fields_ = [("d_stream_ids", C.c_void_p), ("B", C.c_int), ("d_packets", C.c_void_p), ("d_packet_bytes", C.c_void_p),
                ("d_order", C.c_void_p), ("d_room_start", C.c_void_p), ("n_rooms", C.c_int), ("n_members", C.c_int),
                ("d_muted", C.c_void_p), ("flags", C.c_uint), ("d_num_bits", C.c_void_p), ("d_dtx", C.c_void_p),
                ("d_out_packets", C.c_void_p), ("d_out_packet_bytes", C.c_void_p), ("d_pcm16", C.c_void_p),
                ("d_mix", C.c_void_p), ("d_is_noise", C.c_void_p), ("d_is_comfort_noise", C.c_void_p)]


BRIDGE_SKIP_COMFORT_NOISE = 1   # LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE
BRIDGE_MAX_ROOM = 32767         # LYRA_HIP_BRIDGE_MAX_ROOM


def _signatures_bridge():
    """The same for include/lyra_hip_bridge.h (tests/test_bridge_cpu.py holds each entry to its prototype)."""
    vp, ci, cu, cl = C.c_void_p, C.c_int, C.c_uint, C.c_long
    table = {
        "bridge_plan": (ci, [vp, ci, vp, vp, vp, vp]), "bridge_mix_dev": (ci, [vp, vp, ci, vp, vp, ci, ci, vp, vp, vp]),
        "bridge_tick_dev": (ci, [vp, vp]), "bridge_begin": (ci, [vp, vp, ci, vp, vp, vp, vp, cu, vp, vp]),
        "bridge_end": (ci, [vp] * 5), "bridge_errors": (cl, [vp, ci]),
    }
    return {"lyra_hip_" + name: sig for name, sig in table.items()}


_SIGNATURES_BRIDGE = _signatures_bridge()


def _load_bridge(L, path):
    """_SIGNATURES_BRIDGE applied to a loaded library; one that lacks a function of it is refused."""
    for name, (restype, argtypes) in _SIGNATURES_BRIDGE.items():
        fn = getattr(L, name, None)
        if fn is None:
            raise LyraHipError(f"{path} does not export {name}")
        fn.restype, fn.argtypes = restype, argtypes
    return L


def bridge_plan(rooms, lib=None):
    """The membership index of the conference bridge (lyra_hip_bridge_plan; no GPU): rooms int32 [B], a room label >= 0 per
    row or < 0 for a row in no room -> (order int32 [n_members], room_start int32 [n_rooms + 1]).  Rooms in ascending label
    order, rows ascending inside a room.  LyraHipError for a room of more than BRIDGE_MAX_ROOM members."""
    L = lib or _load()
    rooms = np.ascontiguousarray(np.asarray(rooms, np.int32).reshape(-1))
    order = np.zeros(max(rooms.size, 1), np.int32)
    start = np.zeros(rooms.size + 1, np.int32)
    n_rooms, n_members = C.c_int(0), C.c_int(0)
    if L.lyra_hip_bridge_plan(rooms.ctypes.data, rooms.size, order.ctypes.data, start.ctypes.data, C.addressof(n_rooms),
                              C.addressof(n_members)) != 0:
        raise LyraHipError(f"lyra_hip_bridge_plan: a room of more than {BRIDGE_MAX_ROOM} members")
    return order[:n_members.value].copy(), start[:n_rooms.value + 1].copy()


class SpeakersTick(C.Structure):
    """lyra_hip_speakers_tick (include/lyra_hip_speakers.h): the fields of BridgeTick, then the selection's"""
    _fields_ = BridgeTick._fields_ + [("max_speakers", C.c_int), ("d_levels", C.c_void_p), ("d_is_speaker", C.c_void_p)]


SPEAKERS_SKIP_COMFORT_NOISE = 1   # LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE
SPEAKERS_MAX = 8                  # LYRA_HIP_SPEAKERS_MAX


def _signatures_speakers():
    """The same for include/lyra_hip_speakers.h (tests/test_speakers_cpu.py holds each entry to its prototype)."""
    vp, ci, cu = C.c_void_p, C.c_int, C.c_uint
    table = {
        "speakers_mix_dev": [vp, vp, ci, vp, vp, ci, ci, vp, vp, ci, vp, vp, vp], "speakers_tick_dev": [vp, vp],
        "speakers_begin": [vp, vp, ci, vp, vp, vp, vp, cu, vp, vp, ci], "speakers_end": [vp] * 7,
    }
    return {"lyra_hip_" + name: (ci, args) for name, args in table.items()}


_SIGNATURES_SPEAKERS = _signatures_speakers()


def _load_speakers(L, path):
    """_SIGNATURES_SPEAKERS applied to a loaded library; one that lacks a function of it is refused."""
    for name, (restype, argtypes) in _SIGNATURES_SPEAKERS.items():
        fn = getattr(L, name, None)
        if fn is None:
            raise LyraHipError(f"{path} does not export {name}")
        fn.restype, fn.argtypes = restype, argtypes
    return L


class SharedTick(C.Structure):
    """lyra_hip_shared_tick (include/lyra_hip_shared_bridge.h)"""
    _fields_ = [("d_stream_ids", C.c_void_p), ("B", C.c_int), ("d_packets", C.c_void_p), ("d_packet_bytes", C.c_void_p),
                ("d_order", C.c_void_p), ("d_room_start", C.c_void_p), ("n_rooms", C.c_int), ("n_members", C.c_int),
                ("d_muted", C.c_void_p), ("flags", C.c_uint), ("d_out_packets", C.c_void_p), ("d_out_packet_bytes", C.c_void_p),
                ("d_pcm16", C.c_void_p), ("d_is_noise", C.c_void_p), ("d_is_comfort_noise", C.c_void_p),
                ("max_speakers", C.c_int), ("d_levels", C.c_void_p), ("d_is_speaker", C.c_void_p),
                ("d_room_keys", C.c_void_p), ("d_slots", C.c_void_p), ("n_table_rooms", C.c_int),
                ("d_enc_stream_ids", C.c_void_p), ("d_enc_num_bits", C.c_void_p), ("d_enc_dtx", C.c_void_p),
                ("d_enc_mix", C.c_void_p), ("d_enc_packets", C.c_void_p), ("d_enc_packet_bytes", C.c_void_p),
                ("d_slot_of", C.c_void_p)]


SHARED_SLOTS = 8                  # LYRA_HIP_SHARED_SLOTS


def _signatures_shared():
    """The same for include/lyra_hip_shared_bridge.h (tests/test_shared_bridge_cpu.py holds each entry to its prototype)."""
    vp, ci, cu = C.c_void_p, C.c_int, C.c_uint
    table = {
        "shared_mix_dev": [vp, vp, vp, ci, vp, vp, ci, ci, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp],
        "shared_tick_dev": [vp, vp],
        "shared_begin": [vp, vp, ci, vp, vp, vp, vp, cu, ci, vp, ci, vp, vp, vp], "shared_end": [vp] * 8,
        "shared_reset_rooms": [vp, vp, ci],
    }
    return {"lyra_hip_" + name: (ci, args) for name, args in table.items()}


_SIGNATURES_SHARED = _signatures_shared()


def _load_shared(L, path):
    """_SIGNATURES_SHARED applied to a loaded library; one that lacks a function of it is refused."""
    for name, (restype, argtypes) in _SIGNATURES_SHARED.items():
        fn = getattr(L, name, None)
        if fn is None:
            raise LyraHipError(f"{path} does not export {name}")
        fn.restype, fn.argtypes = restype, argtypes
    return L


class BridgeSpansCall(C.Structure):
    """lyra_hip_spans_bridge_call (include/lyra_hip_bridge_spans.h)"""
    _fields_ = [("spans", C.c_void_p), ("P", C.c_int), ("lane_ids", C.c_void_p), ("n_lanes", C.c_int), ("rooms", C.c_void_p),
                ("d_packets", C.c_void_p), ("packet_bytes", C.c_void_p), ("d_muted", C.c_void_p), ("flags", C.c_uint),
                ("num_bits", C.c_void_p), ("dtx", C.c_void_p), ("d_out_packets", C.c_void_p),
                ("d_out_packet_bytes", C.c_void_p), ("d_pcm16", C.c_void_p), ("d_mix", C.c_void_p),
                ("d_is_noise", C.c_void_p), ("d_is_comfort_noise", C.c_void_p), ("max_speakers", C.c_int),
                ("d_levels", C.c_void_p), ("d_is_speaker", C.c_void_p)]


def _signatures_bridge_spans():
    """The same for include/lyra_hip_bridge_spans.h (tests/test_bridge_spans_cpu.py holds each entry to its prototype)."""
    vp, ci, cu = C.c_void_p, C.c_int, C.c_uint
    table = {
        "spans_bridge_plan": [vp, ci, vp, vp, vp, vp, vp, vp],
        "spans_bridge_mix_dev": [vp, vp, ci, vp, vp, vp, vp, ci, vp, vp, vp],
        "spans_bridge_dev": [vp, vp],
        "spans_bridge": [vp, vp, ci, vp, ci, vp, vp, vp, vp, cu, vp, vp, ci] + [vp] * 8,
    }
    return {"lyra_hip_" + name: (ci, args) for name, args in table.items()}


_SIGNATURES_BRIDGE_SPANS = _signatures_bridge_spans()


def _load_bridge_spans(L, path):
    """_SIGNATURES_BRIDGE_SPANS applied to a loaded library; one that lacks a function of it is refused."""
    for name, (restype, argtypes) in _SIGNATURES_BRIDGE_SPANS.items():
        fn = getattr(L, name, None)
        if fn is None:
            raise LyraHipError(f"{path} does not export {name}")
        fn.restype, fn.argtypes = restype, argtypes
    return L


def _bridge_spans_args(spans, rooms):
    """participants of a recording and their room labels -> (SPAN_DTYPE array [P], int32 [P]); LyraHipError where the shapes
    do not fit, before the library is called"""
    sp = _spans(spans)
    labels = np.ascontiguousarray(np.asarray(rooms, np.int32).reshape(-1))
    if sp.size < 1:
        raise LyraHipError("bridge_spans: no participants")
    if labels.size != sp.size:
        raise LyraHipError(f"bridge_spans: rooms has {labels.size} entries for {sp.size} participants")
    if np.any(sp["n_frames"] != sp["n_frames"][0]):
        raise LyraHipError("bridge_spans: every participant's span needs the same n_frames")
    return sp, labels


def bridge_spans_plan(spans, rooms, lib=None):
    """The data model of a recording through the bridge, checked (lyra_hip_spans_bridge_plan; no GPU): spans are (stream_id,
    first_frame, n_frames) per participant with one n_frames = T for all, rooms int32 [P] labels (< 0: in no room) ->
    (order int32 [n_members] participant numbers, room_start int32 [n_rooms + 1], T).  LyraHipError for unequal n_frames,
    overlapping or negative ranges, an id named twice, or a room of more than BRIDGE_MAX_ROOM members."""
    L = lib or _load()
    sp, labels = _bridge_spans_args(spans, rooms)
    order = np.zeros(sp.size, np.int32)
    start = np.zeros(sp.size + 1, np.int32)
    n_rooms, n_members, n_ticks = C.c_int(0), C.c_int(0), C.c_int64(0)
    if L.lyra_hip_spans_bridge_plan(sp.ctypes.data, sp.size, labels.ctypes.data, order.ctypes.data, start.ctypes.data,
                                    C.addressof(n_rooms), C.addressof(n_members), C.addressof(n_ticks)) != 0:
        raise LyraHipError("lyra_hip_spans_bridge_plan: invalid spans or rooms")
    return order[:n_members.value].copy(), start[:n_rooms.value + 1].copy(), n_ticks.value


MEETING_STAY_DTYPE = np.dtype([("participant", "<i4"), ("room", "<i4"), ("first_tick", "<i8"), ("n_ticks", "<i8")], align=True)
MEETING_MAX_ENTRIES = 1 << 22   # LYRA_HIP_MEETING_MAX_ENTRIES


class MeetingSpansCall(C.Structure):
    """lyra_hip_spans_meeting_call (include/lyra_hip_spans_meeting.h)"""
    _fields_ = [("spans", C.c_void_p), ("P", C.c_int), ("lane_ids", C.c_void_p), ("n_lanes", C.c_int), ("stays", C.c_void_p),
                ("n_stays", C.c_int), ("d_packets", C.c_void_p), ("packet_bytes", C.c_void_p), ("d_muted", C.c_void_p),
                ("flags", C.c_uint), ("num_bits", C.c_void_p), ("dtx", C.c_void_p), ("d_out_packets", C.c_void_p),
                ("d_out_packet_bytes", C.c_void_p), ("d_pcm16", C.c_void_p), ("d_mix", C.c_void_p),
                ("d_is_noise", C.c_void_p), ("d_is_comfort_noise", C.c_void_p), ("max_speakers", C.c_int),
                ("d_levels", C.c_void_p), ("d_is_speaker", C.c_void_p)]


def _signatures_spans_meeting():
    """The same for include/lyra_hip_spans_meeting.h (tests/test_spans_meeting_cpu.py holds each entry to its prototype)."""
    vp, ci, cu = C.c_void_p, C.c_int, C.c_uint
    table = {
        "spans_meeting_plan": [vp, ci, vp, ci] + [vp] * 7,
        "spans_meeting_mix_dev": [vp, vp, ci, vp, ci, vp, vp, vp, ci, vp, vp, vp],
        "spans_meeting_dev": [vp, vp],
        "spans_meeting": [vp, vp, ci, vp, ci, vp, ci, vp, vp, vp, cu, vp, vp, ci] + [vp] * 8,
    }
    return {"lyra_hip_" + name: (ci, args) for name, args in table.items()}


_SIGNATURES_SPANS_MEETING = _signatures_spans_meeting()


def _load_spans_meeting(L, path):
    """_SIGNATURES_SPANS_MEETING applied to a loaded library; one that lacks a function of it is refused."""
    for name, (restype, argtypes) in _SIGNATURES_SPANS_MEETING.items():
        fn = getattr(L, name, None)
        if fn is None:
            raise LyraHipError(f"{path} does not export {name}")
        fn.restype, fn.argtypes = restype, argtypes
    return L


def _stays(stays):
    """[(participant, room, first_tick, n_ticks), ...] or a MEETING_STAY_DTYPE array -> contiguous MEETING_STAY_DTYPE array"""
    if isinstance(stays, np.ndarray) and stays.dtype == MEETING_STAY_DTYPE:
        return np.ascontiguousarray(stays)
    return np.array([tuple(int(v) for v in s) for s in stays], MEETING_STAY_DTYPE).reshape(-1)


def _meeting_args(spans, stays):
    """participants of a meeting and its schedule -> (SPAN_DTYPE array [P], MEETING_STAY_DTYPE array); LyraHipError where the
    shapes do not fit, before the library is called"""
    sp, st = _spans(spans), _stays(stays)
    if sp.size < 1:
        raise LyraHipError("meeting: no participants")
    if st.size and (st["participant"].min() < 0 or st["participant"].max() >= sp.size):
        raise LyraHipError(f"meeting: a stay names a participant outside 0..{sp.size - 1}")
    present = np.bincount(st["participant"], weights=st["n_ticks"], minlength=sp.size) if st.size else np.zeros(sp.size)
    if np.any(present != sp["n_frames"]):
        raise LyraHipError("meeting: the stays of a participant do not sum to its span's n_frames")
    return sp, st


def meeting_plan(spans, stays, lib=None):
    """The data model of a meeting with a schedule, checked (lyra_hip_spans_meeting_plan; no GPU): spans are (stream_id,
    first_frame, n_frames = present ticks) per participant, stays (participant, room, first_tick, n_ticks) sorted by
    (participant, first_tick) -> dict(n_ticks, epoch_tick int64 [n_epochs + 1], epoch_entry int64 [n_epochs + 1],
    entry_participant int32 [n_entries], entry_room int32 [n_entries]: the dense room number inside the epoch, -1 in no room).
    LyraHipError for what the header calls LYRA_HIP_EINVAL."""
    L = lib or _load()
    sp, st = _meeting_args(spans, stays)
    n_epochs, n_entries, n_ticks = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    head = (sp.ctypes.data, sp.size, st.ctypes.data if st.size else None, st.size, C.addressof(n_epochs), C.addressof(n_entries),
            C.addressof(n_ticks))
    if L.lyra_hip_spans_meeting_plan(*head, None, None, None, None) != 0:
        raise LyraHipError("lyra_hip_spans_meeting_plan: invalid spans or stays")
    tick, entry = np.zeros(n_epochs.value + 1, np.int64), np.zeros(n_epochs.value + 1, np.int64)
    part, room = np.zeros(max(n_entries.value, 1), np.int32), np.zeros(max(n_entries.value, 1), np.int32)
    if L.lyra_hip_spans_meeting_plan(*head, tick.ctypes.data, entry.ctypes.data, part.ctypes.data, room.ctypes.data) != 0:
        raise LyraHipError("lyra_hip_spans_meeting_plan: invalid spans or stays")
    return dict(n_ticks=n_ticks.value, epoch_tick=tick, epoch_entry=entry, entry_participant=part[:n_entries.value].copy(),
                entry_room=room[:n_entries.value].copy())


def _load(path=None):
    """The C-ABI library (default: library_path()); a second path loads a build variant beside it (lyra_amd/variants/).
    A library that lacks a function of _SIGNATURES, _SIGNATURES_SPANS_MIXED, _SIGNATURES_SPANS_RATES, _SIGNATURES_SPANS_PACKED,
    _SIGNATURES_ENCODE_STREAMS, _SIGNATURES_DECODE_STREAMS, _SIGNATURES_DECODE_SAMPLES_ANY or
    _SIGNATURES_DECODE_SAMPLES_STREAMS is refused, and so is one that lacks a function of _SIGNATURES_BRIDGE (_load_bridge) or _SIGNATURES_SPEAKERS
    (_load_speakers) or _SIGNATURES_SHARED (_load_shared) or _SIGNATURES_BRIDGE_SPANS (_load_bridge_spans) or
    _SIGNATURES_SPANS_MEETING (_load_spans_meeting)."""
    path = os.path.abspath(path or library_path())
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise LyraHipError(f"{path} not built (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                           "there is no CPU fallback")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64; if the system copy gets loaded first
    # (through liblyra_hip.so's dependency) and torch is imported later, torch finds "No HIP GPUs".  Callers that
    # mix this library with torch tensors (the *_dev entry points) are safe regardless of import order if torch's
    # runtime is the one already resident when liblyra_hip.so is opened.
    import importlib.util
    import sys
    if "torch" not in sys.modules and importlib.util.find_spec("torch") is not None and \
            os.environ.get("LYRA_HIP_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(path)
    for name, (restype, argtypes) in (*_SIGNATURES.items(), *_SIGNATURES_SPANS_MIXED.items(), *_SIGNATURES_SPANS_RATES.items(),
                                       *_SIGNATURES_SPANS_PACKED.items(),
                                       *_SIGNATURES_ENCODE_STREAMS.items(), *_SIGNATURES_DECODE_STREAMS.items(),
                                       *_SIGNATURES_DECODE_SAMPLES_ANY.items(), *_SIGNATURES_DECODE_SAMPLES_STREAMS.items()):
        fn = getattr(L, name, None)
        if fn is None:
            raise LyraHipError(f"{path} does not export {name}")
        fn.restype, fn.argtypes = restype, argtypes
    _libs[path] = _load_spans_meeting(_load_bridge_spans(_load_shared(_load_speakers(_load_bridge(L, path), path), path), path), path)
    return L


STATE_ENCODER, STATE_DECODER, STATE_BOTH = 1, 2, 3   # LYRA_HIP_STATE_*: the `sides` of import_streams


_TORCH = {}   # dtype name of a `_dev` buffer -> (torch.Tensor, torch's dtype), resolved once: torch stays an optional import


def _torch_names(dtype_name):
    import torch
    _TORCH[dtype_name] = (torch.Tensor, getattr(torch, dtype_name))
    return _TORCH[dtype_name]


def _np(a, dtype, shape):
    a = np.ascontiguousarray(a, dtype)
    return a.reshape(shape)


def _np01(a, shape):
    """an optional array of switches as int32 zeros and ones (None stays None)"""
    return None if a is None else _np(np.asarray(a) != 0, np.int32, shape)


class LyraHip:
    """One GPU context: weights + per-stream state for `max_streams` streams."""

    def __init__(self, model_dir=None, device=0, max_streams=4096, requant="xnnpack", weights_image=None,
                 sub_batches=None, library=None):
        """sub_batches: split every `_dev` call into that many independent sub-batches on stream pairs of their own
        (the library's LYRA_HIP_SUBBATCHES switch, read when the context is created).  Pays when only ONE side is
        driven (decode-only at B = 8192: +6 %), not for interleaved encode + decode, where the two sides already
        overlap."""
        self.L = _load(library)   # library: path of a build variant (experiments); default liblyra_hip.so
        h = C.c_void_p()
        mode = {"exact": 0, "gemmlowp_double": 1, "xnnpack": 2, "builtin_mixed": 3}[requant]
        saved = os.environ.get("LYRA_HIP_SUBBATCHES")
        if sub_batches is not None:
            os.environ["LYRA_HIP_SUBBATCHES"] = str(int(sub_batches))
        try:
            self._create(h, mode, model_dir, device, max_streams, weights_image)
        finally:
            if sub_batches is not None:
                if saved is None:
                    del os.environ["LYRA_HIP_SUBBATCHES"]
                else:
                    os.environ["LYRA_HIP_SUBBATCHES"] = saved
        self.h = h
        self.device = device
        self.max_streams = max_streams
        self.requant = requant
        self.sub_batches = sub_batches
        self._pending_encodes = []   # (B, num_bits) of the hops begun by encode_begin, oldest first
        self._pending_decodes = []   # B of the calls begun by decode_begin, oldest first
        self._pending_stream_encodes = []   # B of the hops begun by encode_streams_begin, oldest first
        self._pending_any_decodes = []      # (B, num_samples) of the requests begun by decode_samples_any_begin, oldest first
        self._pending_stream_decodes = []   # (B, packed samples) of the hops begun by decode_streams_begin, oldest first
        self._pending_sample_stream_decodes = []   # the same for decode_samples_streams_begin
        self._pending_ticks = []   # (kind, B) of the ticks begun by bridge_begin / speakers_begin / shared_begin, oldest first

    def _create(self, h, mode, model_dir, device, max_streams, weights_image):
        if weights_image is not None:   # bytes of a lyra_v1.lyrapack (lyra_hip_create_from_image)
            weights_image = bytes(weights_image)
            rc = self.L.lyra_hip_create_from_image(weights_image, len(weights_image), device, max_streams, mode,
                                                   C.byref(h))
        else:
            rc = self.L.lyra_hip_create((model_dir or default_model_dir()).encode(), device, max_streams, mode,
                                        C.byref(h))
        if rc != 0:
            raise LyraHipError(f"lyra_hip_create failed ({rc}): {self.L.lyra_hip_last_error(None).decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.L.lyra_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ----------------------------------------------------------------------------------
    def last_error(self):
        return self.L.lyra_hip_last_error(self.h).decode()

    def _chk(self, rc):
        if rc != 0:
            raise LyraHipError(f"lyra_hip error {rc}: {self.last_error()}")

    def stream_handle(self):
        """hipStream_t (int) of the encode side."""
        return self.L.lyra_hip_stream(self.h)

    def stream_handle_decode(self):
        """hipStream_t (int) of the decode side."""
        return self.L.lyra_hip_stream_decode(self.h)

    def stream_handle_quantizer(self):
        """hipStream_t (int) of the quantizer of encode_dev / encode_dtx_dev (their packets are written there)."""
        return self.L.lyra_hip_stream_quantizer(self.h)

    def synchronize(self):
        self._chk(self.L.lyra_hip_synchronize(self.h))

    def state_bytes_per_stream(self):
        return self.L.lyra_hip_state_bytes_per_stream()

    def reset(self, stream_ids=None):
        if stream_ids is None:
            self._chk(self.L.lyra_hip_reset_streams(self.h, None, 0))
            self.synchronize()
        else:
            ids = _np(stream_ids, np.int32, (-1,))
            self._chk(self.L.lyra_hip_reset_streams(self.h, ids.ctypes.data, ids.size))

    @staticmethod
    def _ids(stream_ids, B):
        if stream_ids is None:
            return np.arange(B, dtype=np.int32)
        return _np(stream_ids, np.int32, (B,))

    def _rows(self, a, dtype, width, stream_ids):
        """a -> (contiguous [B][width] array, B, int32 [B] stream ids, 0 .. B - 1 by default), held by the caller for the call"""
        a = _np(a, dtype, (-1, width))
        return a, a.shape[0], self._ids(stream_ids, a.shape[0])

    # -- numpy (host pointer) API --------------------------------------------------------------------
    def extract(self, pcm, stream_ids=None):
        """pcm int16 [B][320] -> features float32 [B][64] (SoundStreamEncoder::Extract)."""
        pcm, B, ids = self._rows(pcm, np.int16, HOP, stream_ids)
        out = np.empty((B, NUM_FEATURES), np.float32)
        self._chk(self.L.lyra_hip_extract(self.h, ids.ctypes.data, B, pcm.ctypes.data, out.ctypes.data))
        return out

    def rvq_encode(self, features, num_bits):
        features = _np(features, np.float32, (-1, NUM_FEATURES))
        B = features.shape[0]
        idx = np.empty((B, 46), np.int32)
        self._chk(self.L.lyra_hip_rvq_encode(self.h, B, features.ctypes.data, num_bits, idx.ctypes.data))
        return idx

    def rvq_decode(self, indices):
        indices = _np(indices, np.int32, (-1, 46))
        B = indices.shape[0]
        out = np.empty((B, NUM_FEATURES), np.float32)
        self._chk(self.L.lyra_hip_rvq_decode(self.h, B, indices.ctypes.data, out.ctypes.data))
        return out

    def generate(self, features, stream_ids=None):
        """features [B][64] -> pcm int16 [B][320] (AddFeatures + GenerateSamples(320))."""
        features, B, ids = self._rows(features, np.float32, NUM_FEATURES, stream_ids)
        out = np.empty((B, HOP), np.int16)
        self._chk(self.L.lyra_hip_generate(self.h, ids.ctypes.data, B, features.ctypes.data, out.ctypes.data))
        return out

    def logmel(self, pcm, stream_ids=None):
        pcm, B, ids = self._rows(pcm, np.int16, HOP, stream_ids)
        out = np.empty((B, NUM_MEL), np.float32)
        self._chk(self.L.lyra_hip_logmel(self.h, ids.ctypes.data, B, pcm.ctypes.data, out.ctypes.data))
        return out

    def encode(self, pcm, num_bits, stream_ids=None):
        """pcm int16 [B][320] -> packets uint8 [B][num_bits/8] (LyraEncoder::Encode, 16 kHz, no DTX)."""
        pcm, B, ids = self._rows(pcm, np.int16, HOP, stream_ids)
        out = np.empty((B, packet_size(num_bits)), np.uint8)
        self._chk(self.L.lyra_hip_encode(self.h, ids.ctypes.data, B, pcm.ctypes.data, num_bits, out.ctypes.data))
        return out

    def encode_begin(self, pcm, num_bits, stream_ids=None, sample_rate_hz=16000, dtx=False):
        """Pipelined form of encode() (include/lyra_hip.h "Pipelined host-buffer calls"): starts a hop and returns; up to
        two hops may be in flight; pcm int16 [B][sample_rate_hz / 50] at 8 / 16 / 32 / 48 kHz.  `pcm` may be reused at once."""
        pcm, B, ids = self._rows(pcm, np.int16, sample_rate_hz // 50, stream_ids)
        if dtx:
            self._chk(self.L.lyra_hip_set_encoder_sample_rate(self.h, sample_rate_hz))
        self._chk(self.L.lyra_hip_encode_begin(self.h, ids.ctypes.data, B, pcm.ctypes.data, sample_rate_hz, num_bits, int(dtx)))
        self._pending_encodes.append((B, num_bits))

    def encode_end(self):
        """-> (packets uint8 [B][num_bits/8], packet_bytes int32 [B]) of the OLDEST hop begun."""
        B, num_bits = self._pending_encodes.pop(0)
        out = np.empty((B, packet_size(num_bits)), np.uint8)
        lens = np.empty(B, np.int32)
        self._chk(self.L.lyra_hip_encode_end(self.h, out.ctypes.data, lens.ctypes.data))
        return out, lens

    def encode_streams_begin(self, pcm, sample_rates, num_bits, dtx=None, stream_ids=None):
        """Pipelined encode of streams that differ in sample rate, bitrate and DTX (lyra_hip_encode_streams_begin): pcm int16,
        PACKED -- row b holds sample_rates[b] / 50 samples, rows back to back (a numpy array, or a CPU torch tensor, e.g. a
        pinned one); sample_rates / num_bits int32 [B]; dtx [B] 0 / non-zero or None (no stream uses DTX).  Up to two hops in
        flight; `pcm` may be reused at once."""
        rates = _np(sample_rates, np.int32, (-1,))
        B = rates.shape[0]
        bits = _np(num_bits, np.int32, (B,))
        flags = None if dtx is None else _np(np.asarray(dtx) != 0, np.int32, (B,))
        ids = self._ids(stream_ids, B)
        # (the library reads sum(rates / 50) samples once it has accepted every rate; a list it refuses is not sized here)
        n = int(rates.sum()) // 50 if np.isin(rates, (8000, 16000, 32000, 48000)).all() else None
        if hasattr(pcm, "data_ptr"):   # a CPU torch tensor is read in place
            if pcm.is_cuda or str(pcm.dtype) != "torch.int16" or not pcm.is_contiguous() or n not in (None, pcm.numel()):
                raise LyraHipError(f"pcm: expected a contiguous CPU int16 tensor of {n} samples")
            p_pcm = pcm.data_ptr()
        else:
            pcm = _np(pcm, np.int16, (-1,))
            if n not in (None, pcm.size):
                raise LyraHipError(f"pcm: {pcm.size} samples, expected {n} (the sum of sample_rates / 50)")
            p_pcm = pcm.ctypes.data
        self._chk(self.L.lyra_hip_encode_streams_begin(self.h, ids.ctypes.data, B, p_pcm, rates.ctypes.data, bits.ctypes.data,
                                                       None if flags is None else flags.ctypes.data))
        self._pending_stream_encodes.append(B)

    def encode_streams_end(self):
        """-> (packets uint8 [B][MAX_PACKET_BYTES], zero behind each packet's bytes, packet_bytes int32 [B]) of the OLDEST
        hop begun by encode_streams_begin."""
        if not self._pending_stream_encodes:
            self._chk(self.L.lyra_hip_encode_streams_end(self.h, None, None))
        B = self._pending_stream_encodes.pop(0)
        out = np.empty((B, MAX_PACKET_BYTES), np.uint8)
        lens = np.empty(B, np.int32)
        self._chk(self.L.lyra_hip_encode_streams_end(self.h, out.ctypes.data, lens.ctypes.data))
        return out, lens

    def decode_streams_begin(self, packets, packet_bytes, sample_rates, stream_ids=None):
        """Pipelined hop of decoders that differ in sample rate and packet size (lyra_hip_decode_streams_begin): packets uint8
        [B][MAX_PACKET_BYTES], packet_bytes int32 [B] (0 = no packet on this hop, else 8 / 15 / 23), sample_rates int32 [B];
        numpy arrays or CPU torch tensors (e.g. pinned ones).  Up to two hops in flight; the arrays may be reused at once."""
        def host(a, dtype, shape):   # a CPU torch tensor is read in place
            if hasattr(a, "data_ptr"):
                if a.is_cuda or not a.is_contiguous() or str(a.dtype) != "torch." + np.dtype(dtype).name:
                    raise LyraHipError(f"expected a contiguous CPU {np.dtype(dtype).name} tensor")
                if shape[0] >= 0 and tuple(a.shape) != tuple(shape):
                    raise LyraHipError(f"shape {tuple(a.shape)}, expected {tuple(shape)}")
                return a, a.data_ptr(), a.shape[0]
            a = _np(a, dtype, shape)
            return a, a.ctypes.data, a.shape[0]
        rates, p_rates, B = host(sample_rates, np.int32, (-1,))
        packets, p_packets, _ = host(packets, np.uint8, (B, MAX_PACKET_BYTES))
        sizes, p_sizes, _ = host(packet_bytes, np.int32, (B,))
        ids = self._ids(stream_ids, B)
        total = int(np.asarray(rates).astype(np.int64).sum()) // 50   # (what end() sizes its array by: before the call)
        self._chk(self.L.lyra_hip_decode_streams_begin(self.h, ids.ctypes.data, B, p_packets, p_sizes, p_rates))
        self._pending_stream_decodes.append((B, total))

    def decode_streams_end(self):
        """-> (pcm int16, PACKED: row b holds sample_rates[b] / 50 samples, rows back to back in batch order; is_noise int32
        [B]; is_comfort_noise int32 [B]) of the OLDEST hop begun by decode_streams_begin."""
        if not self._pending_stream_decodes:
            self._chk(self.L.lyra_hip_decode_streams_end(self.h, None, None, None))
        B, total = self._pending_stream_decodes[0]
        pcm = np.empty(total, np.int16)
        noise = np.empty(B, np.int32)
        cn = np.empty(B, np.int32)
        rc = self.L.lyra_hip_decode_streams_end(self.h, pcm.ctypes.data, noise.ctypes.data, cn.ctypes.data)
        self._pending_stream_decodes.pop(0)   # (the library gives the slot back whatever the wait returns)
        self._chk(rc)
        return pcm, noise, cn

    def decode_begin(self, packets, num_bits, stream_ids=None):
        """Pipelined form of decode(): starts a call and returns (up to two in flight); decode_end() -> pcm of the oldest."""
        packets, B, ids = self._rows(packets, np.uint8, packet_size(num_bits), stream_ids)
        self._chk(self.L.lyra_hip_decode_begin(self.h, ids.ctypes.data, B, packets.ctypes.data, num_bits))
        self._pending_decodes.append(B)

    def decode_end(self):
        out = np.empty((self._pending_decodes.pop(0), HOP), np.int16)
        self._chk(self.L.lyra_hip_decode_end(self.h, out.ctypes.data))
        return out

    def decode(self, packets, num_bits, stream_ids=None):
        """packets uint8 [B][num_bits/8] -> pcm int16 [B][320] (SetEncodedPacket + DecodeSamples(320))."""
        packets, B, ids = self._rows(packets, np.uint8, packet_size(num_bits), stream_ids)
        out = np.empty((B, HOP), np.int16)
        self._chk(self.L.lyra_hip_decode(self.h, ids.ctypes.data, B, packets.ctypes.data, num_bits, out.ctypes.data))
        return out

    _SIDES = SIDES

    def noise_receive(self, pcm, stream_ids=None, side="decoder"):
        """NoiseEstimator::ReceiveSamples, one full hop per stream -> is_noise int32 [B]."""
        pcm, B, ids = self._rows(pcm, np.int16, HOP, stream_ids)
        out = np.empty(B, np.int32)
        self._chk(self.L.lyra_hip_noise_receive(self.h, self._SIDES[side], ids.ctypes.data, B, pcm.ctypes.data,
                                                out.ctypes.data))
        return out

    def noise_estimate(self, stream_ids, side="decoder"):
        """NoiseEstimator::noise_estimate() -> float32 [B][160]."""
        ids = _np(stream_ids, np.int32, (-1,))
        out = np.empty((ids.size, NUM_MEL), np.float32)
        self._chk(self.L.lyra_hip_noise_estimate(self.h, self._SIDES[side], ids.ctypes.data, ids.size, out.ctypes.data))
        return out

    def encode_dtx(self, pcm, num_bits, stream_ids=None):
        """LyraEncoder::Encode with enable_dtx -> (packets uint8 [B][nbytes], packet_bytes int32 [B]; 0 = empty packet)."""
        pcm, B, ids = self._rows(pcm, np.int16, HOP, stream_ids)
        out = np.zeros((B, packet_size(num_bits)), np.uint8)
        nbytes = np.empty(B, np.int32)
        self._chk(self.L.lyra_hip_encode_dtx(self.h, ids.ctypes.data, B, pcm.ctypes.data, num_bits, out.ctypes.data,
                                             nbytes.ctypes.data))
        return out, nbytes

    def resample(self, audio, in_rate, out_rate, stream_ids=None, side="encoder"):
        """Resampler::Resample per stream: int16 [B][n_in] -> int16 [B][n_in * out_rate / in_rate]."""
        audio = np.ascontiguousarray(audio, np.int16)
        B, n_in = audio.shape
        ids = self._ids(stream_ids, B)
        out = np.empty((B, n_in * out_rate // in_rate), np.int16)
        self._chk(self.L.lyra_hip_resample(self.h, self._SIDES[side], ids.ctypes.data, B, audio.ctypes.data, n_in,
                                           in_rate, out_rate, out.ctypes.data))
        return out

    def comfort_noise(self, features=None, stream_ids=None, B=None):
        """ComfortNoiseGenerator: one hop per stream; features float32 [B][160] or None (= the decoder-side noise estimate)."""
        if features is not None:
            features = _np(features, np.float32, (-1, NUM_MEL))
            B = features.shape[0]
        elif B is None and stream_ids is not None:
            B = len(stream_ids)
        ids = self._ids(stream_ids, B)
        out = np.empty((B, HOP), np.int16)
        self._chk(self.L.lyra_hip_comfort_noise(self.h, ids.ctypes.data, B,
                                                features.ctypes.data if features is not None else None, out.ctypes.data))
        return out

    def set_encoder_sample_rate(self, sample_rate_hz):
        """The rate a DTX LyraEncoder was created with: time constants of the encoder-side noise estimator
        (lyra_encoder.cc:82-85, noise_estimator.cc:96-124)."""
        self._chk(self.L.lyra_hip_set_encoder_sample_rate(self.h, sample_rate_hz))

    def set_cng_seed(self, seed):
        self._chk(self.L.lyra_hip_set_cng_seed(self.h, seed))

    def profile_kernel_names(self):
        n = self.L.lyra_hip_profile_kernel_count()
        return [self.L.lyra_hip_profile_kernel_name(i).decode() for i in range(n)]

    def set_stream_priorities(self, encode_side=0, decode_side=0, quantizer=2):
        """Priorities (0 lowest .. 2 highest) of the context's three main streams; drains the context (include/lyra_hip.h)."""
        self._chk(self.L.lyra_hip_set_stream_priorities(self.h, int(encode_side), int(decode_side), int(quantizer)))

    def profile_enable(self, on=True, only=None, every=1):
        """Bracket kernel launches with HIP events: all kernels, or only the named one(s); every `every`-th launch."""
        self._chk(self.L.lyra_hip_profile_sample(self.h, int(every)))
        mask = 0
        if on:
            names = self.profile_kernel_names()
            if only:
                for k in ([only] if isinstance(only, str) else only):
                    mask |= 1 << names.index(k)
            else:
                mask = (1 << len(names)) - 1
        self._chk(self.L.lyra_hip_profile_enable(self.h, mask))

    def profile_read(self):
        """{kernel name: (total_ms, launches)} since the last read (HIP events on the context's stream)."""
        n = self.L.lyra_hip_profile_kernel_count()
        ms = (C.c_double * n)()
        cnt = (C.c_long * n)()
        self._chk(self.L.lyra_hip_profile_read(self.h, ms, cnt))
        return {self.L.lyra_hip_profile_kernel_name(i).decode(): (ms[i], cnt[i]) for i in range(n)}

    def debug_read(self, which, n):
        out = np.empty(n, np.float32)
        got = self.L.lyra_hip_debug_read(self.h, which, out.ctypes.data, n)
        if got < 0:
            raise LyraHipError(self.last_error())
        return out[:got]

    # -- torch (device pointer) API ---------------------------------------------------------------------------
    # The library's streams are non-blocking: they do not order against torch's streams by themselves.  With
    # `torch_order=True` (default) every `_dev` call is bracketed by lyra_hip_wait_for_stream /
    # lyra_hip_stream_wait on torch's CURRENT stream, so tensors produced or consumed by torch kernels on that
    # stream are safe without a synchronize.  bench.py turns it off (it synchronises explicitly around the timed
    # region and wants no extra event traffic inside it).
    torch_order = True

    def set_serial(self, on=True):
        """Run the library streams strictly in call order (lyra_hip_set_serial)."""
        self._chk(self.L.lyra_hip_set_serial(self.h, 1 if on else 0))

    def _dev_ptr(self, t, dtype_name, shape, what):
        tensor, want = _TORCH.get(dtype_name) or _torch_names(dtype_name)
        if not isinstance(t, tensor) or not t.is_cuda or t.device.index != self.device:
            raise LyraHipError(f"{what}: expected a CUDA tensor on device {self.device}")
        if t.dtype != want:
            raise LyraHipError(f"{what}: dtype {t.dtype}, expected {want}")
        if not t.is_contiguous():
            raise LyraHipError(f"{what}: tensor is not contiguous")
        if tuple(t.shape) != tuple(shape):
            raise LyraHipError(f"{what}: shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t.data_ptr()

    def _opt_dev_ptr(self, t, dtype_name, shape, what):
        """_dev_ptr of a buffer the call can do without: None -> a null pointer"""
        return None if t is None else self._dev_ptr(t, dtype_name, shape, what)

    # the buffers most `_dev` calls share, B rows each
    def _p_ids(self, t, B):
        return self._dev_ptr(t, "int32", (B,), "stream ids")

    def _p_pcm(self, t, B):
        return self._dev_ptr(t, "int16", (B, HOP), "pcm")

    def _p_packets(self, t, B, nbytes):
        return self._dev_ptr(t, "uint8", (B, nbytes), "packets")

    def _p_packet_bytes(self, t, B):
        return self._dev_ptr(t, "int32", (B,), "packet bytes")

    def _p_noise_flags(self, d_is_noise, d_is_comfort_noise, B):
        return (self._opt_dev_ptr(d_is_noise, "int32", (B,), "is_noise"),
                self._opt_dev_ptr(d_is_comfort_noise, "int32", (B,), "is_comfort_noise"))

    def _error_count(self, fn, clear):
        """A device error counter (long; negative = the read itself failed), optionally cleared by the read"""
        n = fn(self.h, 1 if clear else 0)
        self._chk(n if n < 0 else 0)
        return n

    def _torch_stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _dev_call(self, fn, *args):
        if self.torch_order:
            st = self._torch_stream()
            self._chk(self.L.lyra_hip_wait_for_stream(self.h, st))
            self._chk(fn(self.h, *args))
            self._chk(self.L.lyra_hip_stream_wait(self.h, st))
        else:
            self._chk(fn(self.h, *args))

    def encode_dev(self, d_ids, d_pcm, num_bits, d_packets):
        B = d_pcm.shape[0]
        self._dev_call(self.L.lyra_hip_encode_dev, self._p_ids(d_ids, B), B, self._p_pcm(d_pcm, B), num_bits,
                       self._p_packets(d_packets, B, packet_size(num_bits)))

    def encode_dtx_dev(self, d_ids, d_pcm, num_bits, d_packets, d_packet_bytes):
        """LyraEncoder::Encode with enable_dtx on device buffers: packets uint8 [B][nbytes] (rows of noise hops are
        left untouched) and packet_bytes int32 [B] (0 = empty packet)."""
        B = d_pcm.shape[0]
        self._dev_call(self.L.lyra_hip_encode_dtx_dev, self._p_ids(d_ids, B), B, self._p_pcm(d_pcm, B), num_bits,
                       self._p_packets(d_packets, B, packet_size(num_bits)), self._p_packet_bytes(d_packet_bytes, B))

    def encode_ext_dev(self, d_ids, d_pcm_ext, sample_rate_hz, num_bits, d_packets, d_packet_bytes=None, dtx=False):
        """LyraEncoder::Encode at an external sample rate as ONE encode-side call (lyra_hip_encode_ext_dev): resampler, with
        dtx the NoiseEstimator decision (d_packet_bytes int32 [B] required), extractor, quantizer.  d_pcm_ext int16
        [B][320 * rate / 16000]."""
        B = d_pcm_ext.shape[0]
        n_ext = HOP * sample_rate_hz // 16000
        self._dev_call(self.L.lyra_hip_encode_ext_dev, self._p_ids(d_ids, B), B,
                       self._dev_ptr(d_pcm_ext, "int16", (B, n_ext), "pcm"), sample_rate_hz, num_bits, 1 if dtx else 0,
                       self._p_packets(d_packets, B, packet_size(num_bits)),
                       self._opt_dev_ptr(d_packet_bytes, "int32", (B,), "packet bytes"))

    def decode_ext_dev(self, d_ids, d_packets, num_bits, sample_rate_hz, d_pcm16, d_pcm_ext=None, d_is_noise=None):
        """LyraDecoder::DecodeSamples for a received hop at an external rate as ONE decode-side call
        (lyra_hip_decode_ext_dev): decode -> d_pcm16 [B][320]; d_is_noise given: the decoder-side NoiseEstimator; rate !=
        16000: the resampler -> d_pcm_ext [B][320 * rate / 16000].  Estimator and resampler complete on the noise stream."""
        B = d_packets.shape[0]
        n_ext = HOP * sample_rate_hz // 16000
        self._dev_call(self.L.lyra_hip_decode_ext_dev, self._p_ids(d_ids, B), B,
                       self._p_packets(d_packets, B, packet_size(num_bits)), num_bits, sample_rate_hz,
                       1 if d_is_noise is not None else 0, self._p_pcm(d_pcm16, B),
                       self._opt_dev_ptr(d_pcm_ext, "int16", (B, n_ext), "external-rate pcm"),
                       self._opt_dev_ptr(d_is_noise, "int32", (B,), "is_noise"))

    def decode_lossy_dev(self, d_ids, d_packets, d_packet_bytes, num_bits, sample_rate_hz, d_pcm16, d_pcm_ext=None,
                         d_is_noise=None, d_is_comfort_noise=None):
        """LyraDecoder::SetEncodedPacket (if received) + DecodeSamples(one hop) for a hop-synchronous receiver
        (lyra_hip_decode_lossy_dev): d_packet_bytes int32 [B], 0 = no packet this hop (concealment / comfort noise), else
        the packet size; d_pcm16 [B][320], d_pcm_ext [B][rate / 50] (rate != 16000), d_is_noise / d_is_comfort_noise int32
        [B] optional.  The outputs complete on the noise stream."""
        B = d_packets.shape[0]
        n_ext = HOP * sample_rate_hz // 16000
        self._dev_call(self.L.lyra_hip_decode_lossy_dev, self._p_ids(d_ids, B), B,
                       self._p_packets(d_packets, B, packet_size(num_bits)), self._p_packet_bytes(d_packet_bytes, B),
                       num_bits, sample_rate_hz, self._p_pcm(d_pcm16, B),
                       self._opt_dev_ptr(d_pcm_ext, "int16", (B, n_ext), "external-rate pcm"),
                       *self._p_noise_flags(d_is_noise, d_is_comfort_noise, B))

    def decode_lossy_errors(self, clear=False):
        """packet_bytes values seen by decode_lossy_dev / run_steps that were neither 0 nor the packet size (synchronises)."""
        return self._error_count(self.L.lyra_hip_decode_lossy_errors, clear)

    def encode_mixed_dev(self, d_ids, d_pcm_ext, sample_rate_hz, d_num_bits, d_packets, d_packet_bytes, dtx=False):
        """encode_ext_dev with a bit count per stream (lyra_hip_encode_mixed_dev): d_num_bits int32 [B] (multiples of 4 in
        4..184), d_packets uint8 [B][MAX_PACKET_BYTES] (row b gets packet_bytes[b] bytes, the rest is left alone),
        d_packet_bytes int32 [B] (0: DTX noise hop or invalid bit count, see encode_mixed_errors)."""
        B = d_pcm_ext.shape[0]
        n_ext = HOP * sample_rate_hz // 16000
        self._dev_call(self.L.lyra_hip_encode_mixed_dev, self._p_ids(d_ids, B), B,
                       self._dev_ptr(d_pcm_ext, "int16", (B, n_ext), "pcm"), sample_rate_hz,
                       self._dev_ptr(d_num_bits, "int32", (B,), "num_bits"), 1 if dtx else 0,
                       self._p_packets(d_packets, B, MAX_PACKET_BYTES), self._p_packet_bytes(d_packet_bytes, B))

    def encode_mixed_errors(self, clear=False):
        """Invalid bit counts seen by encode_mixed_dev / run_steps with a bits ring (synchronises)."""
        return self._error_count(self.L.lyra_hip_encode_mixed_errors, clear)

    def decode_lossy_mixed_dev(self, d_ids, d_packets, d_packet_bytes, sample_rate_hz, d_pcm16, d_pcm_ext=None,
                               d_is_noise=None, d_is_comfort_noise=None):
        """decode_lossy_dev with the packet size per row (lyra_hip_decode_lossy_mixed_dev): d_packets uint8
        [B][MAX_PACKET_BYTES], d_packet_bytes int32 [B]: 0 = no packet, 8 / 15 / 23 = received at 64 / 120 / 184 bits,
        anything else = no packet, counted in decode_lossy_errors."""
        B = d_packets.shape[0]
        n_ext = HOP * sample_rate_hz // 16000
        self._dev_call(self.L.lyra_hip_decode_lossy_mixed_dev, self._p_ids(d_ids, B), B,
                       self._p_packets(d_packets, B, MAX_PACKET_BYTES), self._p_packet_bytes(d_packet_bytes, B),
                       sample_rate_hz, self._p_pcm(d_pcm16, B),
                       self._opt_dev_ptr(d_pcm_ext, "int16", (B, n_ext), "external-rate pcm"),
                       *self._p_noise_flags(d_is_noise, d_is_comfort_noise, B))

    def encode_rates_dev(self, d_ids, d_pcm_ext, d_sample_rates, d_num_bits, d_packets, d_packet_bytes, dtx=False):
        """encode_mixed_dev with a sample rate per stream (lyra_hip_encode_rates_dev): d_pcm_ext int16 [B][MAX_EXT_HOP], row
        b holds d_sample_rates[b] / 50 samples; d_sample_rates int32 [B] (8000 / 16000 / 32000 / 48000; anything else:
        packet_bytes 0, no state advances, counted in rates_errors); the rest as encode_mixed_dev.  Does not read
        set_encoder_sample_rate's setting."""
        B = d_pcm_ext.shape[0]
        self._dev_call(self.L.lyra_hip_encode_rates_dev, self._p_ids(d_ids, B), B,
                       self._dev_ptr(d_pcm_ext, "int16", (B, MAX_EXT_HOP), "pcm"),
                       self._dev_ptr(d_sample_rates, "int32", (B,), "sample rates"),
                       self._dev_ptr(d_num_bits, "int32", (B,), "num_bits"), 1 if dtx else 0,
                       self._p_packets(d_packets, B, MAX_PACKET_BYTES), self._p_packet_bytes(d_packet_bytes, B))

    def encode_streams_dev(self, d_ids, d_pcm_ext, d_sample_rates, d_num_bits, d_packets, d_packet_bytes, d_dtx=None,
                           d_pcm_offsets=None, n_pcm_samples=None):
        """encode_rates_dev with DTX per stream and, optionally, packed audio rows (lyra_hip_encode_streams_dev): d_dtx int32
        [B] (0: the stream's encoder has no noise estimator) or None (no stream uses DTX); d_pcm_ext int16, any shape: row b
        holds d_sample_rates[b] / 50 samples at d_pcm_offsets[b] (int32 [B], multiples of 8 samples inside the buffer; None:
        b * MAX_EXT_HOP); n_pcm_samples: how much of d_pcm_ext the rows may lie in (None: all of it).  A row with a bad offset
        is treated as one with an invalid rate (rates_errors)."""
        B = d_sample_rates.shape[0]
        if n_pcm_samples is None:
            n_pcm_samples = d_pcm_ext.numel()
        elif n_pcm_samples > d_pcm_ext.numel():
            raise LyraHipError(f"pcm: n_pcm_samples {n_pcm_samples} exceeds the tensor's {d_pcm_ext.numel()} samples")
        self._dev_call(self.L.lyra_hip_encode_streams_dev, self._p_ids(d_ids, B), B,
                       self._dev_ptr(d_pcm_ext, "int16", tuple(d_pcm_ext.shape), "pcm"), int(n_pcm_samples),
                       self._opt_dev_ptr(d_pcm_offsets, "int32", (B,), "pcm offsets"),
                       self._dev_ptr(d_sample_rates, "int32", (B,), "sample rates"),
                       self._dev_ptr(d_num_bits, "int32", (B,), "num_bits"),
                       self._opt_dev_ptr(d_dtx, "int32", (B,), "dtx flags"),
                       self._p_packets(d_packets, B, MAX_PACKET_BYTES), self._p_packet_bytes(d_packet_bytes, B))

    def decode_lossy_rates_dev(self, d_ids, d_packets, d_packet_bytes, d_sample_rates, d_pcm16, d_pcm_ext,
                               d_is_noise=None, d_is_comfort_noise=None):
        """decode_lossy_mixed_dev with a sample rate per stream (lyra_hip_decode_lossy_rates_dev): d_pcm_ext int16
        [B][MAX_EXT_HOP], row b receives d_sample_rates[b] / 50 samples (320 copies of d_pcm16 at 16000; nothing, counted
        in rates_errors, at a value that is no codec rate)."""
        B = d_packets.shape[0]
        self._dev_call(self.L.lyra_hip_decode_lossy_rates_dev, self._p_ids(d_ids, B), B,
                       self._p_packets(d_packets, B, MAX_PACKET_BYTES), self._p_packet_bytes(d_packet_bytes, B),
                       self._dev_ptr(d_sample_rates, "int32", (B,), "sample rates"), self._p_pcm(d_pcm16, B),
                       self._dev_ptr(d_pcm_ext, "int16", (B, MAX_EXT_HOP), "external-rate pcm"),
                       *self._p_noise_flags(d_is_noise, d_is_comfort_noise, B))

    def decode_streams_dev(self, d_ids, d_packets, d_packet_bytes, d_sample_rates, d_pcm, d_pcm_offsets=None, d_pcm16=None,
                           d_is_noise=None, d_is_comfort_noise=None, n_pcm_samples=None):
        """decode_lossy_rates_dev with, optionally, packed output rows and without the 16 kHz hop
        (lyra_hip_decode_streams_dev): d_pcm int16, any shape: row b's d_sample_rates[b] / 50 samples go to d_pcm_offsets[b]
        (int32 [B], multiples of 8 samples inside the buffer; None: b * MAX_EXT_HOP); n_pcm_samples: how much of d_pcm the
        rows may lie in (None: all of it); d_pcm16 int16 [B][HOP] or None (library scratch).  A row with a bad offset is
        treated as one with an invalid rate: nothing of d_pcm is written for it (rates_errors)."""
        B = d_sample_rates.shape[0]
        if n_pcm_samples is None:
            n_pcm_samples = d_pcm.numel()
        elif n_pcm_samples > d_pcm.numel():
            raise LyraHipError(f"pcm: n_pcm_samples {n_pcm_samples} exceeds the tensor's {d_pcm.numel()} samples")
        self._dev_call(self.L.lyra_hip_decode_streams_dev, self._p_ids(d_ids, B), B,
                       self._p_packets(d_packets, B, MAX_PACKET_BYTES), self._p_packet_bytes(d_packet_bytes, B),
                       self._dev_ptr(d_sample_rates, "int32", (B,), "sample rates"),
                       self._dev_ptr(d_pcm, "int16", tuple(d_pcm.shape), "pcm"), int(n_pcm_samples),
                       self._opt_dev_ptr(d_pcm_offsets, "int32", (B,), "pcm offsets"),
                       self._opt_dev_ptr(d_pcm16, "int16", (B, HOP), "16 kHz pcm"),
                       *self._p_noise_flags(d_is_noise, d_is_comfort_noise, B))

    # -- the conference bridge (include/lyra_hip_bridge.h) ---------------------------------------------
    # What the calls of its three kinds of tick share -- the full mix here, the loudest-N selection and the shared encoders
    # below -- is built once:
    def _p_bridge_index(self, d_order, d_room_start):
        """-> (d_order, d_room_start, n_rooms, n_members) as the mix and tick calls take the index of bridge_plan"""
        n_members, n_rooms = d_order.shape[0], d_room_start.shape[0] - 1
        return (self._dev_ptr(d_order, "int32", (n_members,), "order") if n_members else None,
                self._dev_ptr(d_room_start, "int32", (n_rooms + 1,), "room_start"), n_rooms, n_members)

    def _p_mix_sources(self, d_order, d_room_start, d_muted, d_is_comfort_noise, B):
        """-> the index, then the two optional lists of rows that are no source: the middle arguments of the mix calls"""
        return (*self._p_bridge_index(d_order, d_room_start), self._opt_dev_ptr(d_muted, "int32", (B,), "muted"),
                self._opt_dev_ptr(d_is_comfort_noise, "int32", (B,), "is_comfort_noise"))

    def _p_selection(self, max_speakers, d_levels, d_is_speaker, B):
        """-> (max_speakers, d_levels, d_is_speaker): what a selection adds to a mix call and to a tick struct"""
        return (int(max_speakers), self._opt_dev_ptr(d_levels, "int64", (B,), "levels"),
                self._opt_dev_ptr(d_is_speaker, "int32", (B,), "is_speaker"))

    def _p_tick_head(self, d_ids, d_packets, d_packet_bytes, d_order, d_room_start, d_muted, flags):
        """-> B and the leading fields of the three tick structs, d_stream_ids .. flags"""
        B = d_packets.shape[0]
        return B, (self._p_ids(d_ids, B), B, self._p_packets(d_packets, B, MAX_PACKET_BYTES),
                   self._p_packet_bytes(d_packet_bytes, B), *self._p_bridge_index(d_order, d_room_start),
                   self._opt_dev_ptr(d_muted, "int32", (B,), "muted"), int(flags))

    def _p_tick_outputs(self, d_out_packets, d_out_packet_bytes, d_pcm16, B):
        """-> the fields d_out_packets, d_out_packet_bytes, d_pcm16 of the three tick structs"""
        return (self._p_packets(d_out_packets, B, MAX_PACKET_BYTES), self._p_packet_bytes(d_out_packet_bytes, B),
                self._opt_dev_ptr(d_pcm16, "int16", (B, HOP), "16 kHz pcm"))

    def _p_listener_bits(self, d_num_bits, d_dtx, B):
        """-> the fields d_num_bits, d_dtx of the ticks that encode a row per listener"""
        return (self._dev_ptr(d_num_bits, "int32", (B,), "num_bits"), self._opt_dev_ptr(d_dtx, "int32", (B,), "dtx flags"))

    def _tick_begin_args(self, packets, packet_bytes, rooms, muted, flags, stream_ids):
        """-> B, the host arrays (to be kept alive over the call) and the leading arguments of the three begin() calls"""
        packets = _np(packets, np.uint8, (-1, MAX_PACKET_BYTES))
        B = packets.shape[0]
        sizes, labels = (_np(a, np.int32, (B,)) for a in (packet_bytes, rooms))
        m = _np01(muted, (B,))
        ids = self._ids(stream_ids, B)
        return B, (packets, sizes, labels, m, ids), (self.h, ids.ctypes.data, B, packets.ctypes.data, sizes.ctypes.data,
                                                     labels.ctypes.data, None if m is None else m.ctypes.data, int(flags))

    def _tick_begin(self, kind, fn, B, *args):
        self._chk(fn(*args))
        self._pending_ticks.append((kind, B))

    def _tick_end(self, kind, fn, n_flags, with_levels):
        """end() of the three kinds of tick -> (out_packets uint8 [B][23], n_flags int32 [B] arrays -- with_levels: levels int64
        [B] behind the third) in the order of the library's arguments.  The arrays are sized by the oldest tick in flight,
        whatever its kind: an end() of another kind the library refuses, keeping the tick, and its message is what the caller
        sees."""
        if not self._pending_ticks:
            self._chk(fn(self.h, *[None] * (1 + n_flags + with_levels)))
        begun, B = self._pending_ticks[0]
        out = np.empty((B, MAX_PACKET_BYTES), np.uint8)
        flags = [np.empty(B, np.int32) for _ in range(n_flags)]
        arrays = flags[:3] + ([np.empty(B, np.int64)] if with_levels else []) + flags[3:]
        rc = fn(self.h, out.ctypes.data, *(a.ctypes.data for a in arrays))
        if begun == kind:
            self._pending_ticks.pop(0)   # (the library gives the slot back whatever the wait returns)
        self._chk(rc)
        return (out, *arrays)

    def bridge_mix_dev(self, d_pcm16, d_order, d_room_start, d_mix, d_muted=None, d_is_comfort_noise=None):
        """The mix-minus alone (lyra_hip_bridge_mix_dev): d_pcm16 / d_mix int16 [B][320]; d_order int32 [n_members] row
        numbers with a room's rows contiguous, d_room_start int32 [n_rooms + 1] (bridge_plan); d_muted / d_is_comfort_noise
        int32 [B] or None: rows that are no source.  Row b of d_mix receives the clamped sum of the other sources of its room,
        zeros if no room names it.  Bad d_order entries are skipped and counted in bridge_errors.  Completes on the
        encode-side stream."""
        B = d_pcm16.shape[0]
        self._dev_call(self.L.lyra_hip_bridge_mix_dev, self._p_pcm(d_pcm16, B), B,
                       *self._p_mix_sources(d_order, d_room_start, d_muted, d_is_comfort_noise, B), self._p_pcm(d_mix, B))

    def bridge_tick_dev(self, d_ids, d_packets, d_packet_bytes, d_order, d_room_start, d_num_bits, d_out_packets,
                        d_out_packet_bytes, d_muted=None, d_dtx=None, flags=0, d_pcm16=None, d_mix=None, d_is_noise=None,
                        d_is_comfort_noise=None):
        """One tick of the bridge (lyra_hip_bridge_tick_dev): decode_lossy_mixed_dev(16000) on d_packets uint8 [B][23] /
        d_packet_bytes int32 [B], the mix of bridge_mix_dev (flags: BRIDGE_SKIP_COMFORT_NOISE), encode_streams_dev at 16 kHz
        on the mix with d_num_bits int32 [B] / d_dtx int32 [B] or None into d_out_packets uint8 [B][23] /
        d_out_packet_bytes int32 [B].  d_pcm16 / d_mix int16 [B][320], d_is_noise / d_is_comfort_noise int32 [B]: optional
        outputs.  Bit for bit the three calls in a row, outputs and stream state."""
        B, head = self._p_tick_head(d_ids, d_packets, d_packet_bytes, d_order, d_room_start, d_muted, flags)
        t = BridgeTick(*head, *self._p_listener_bits(d_num_bits, d_dtx, B),
                       *self._p_tick_outputs(d_out_packets, d_out_packet_bytes, d_pcm16, B),
                       self._opt_dev_ptr(d_mix, "int16", (B, HOP), "mix"),
                       *self._p_noise_flags(d_is_noise, d_is_comfort_noise, B))
        self._dev_call(self.L.lyra_hip_bridge_tick_dev, C.addressof(t))

    def bridge_begin(self, packets, packet_bytes, rooms, num_bits, muted=None, dtx=None, flags=0, stream_ids=None):
        """Pipelined tick of the bridge from host arrays (lyra_hip_bridge_begin): packets uint8 [B][23], packet_bytes int32 [B]
        (0 / 8 / 15 / 23), rooms int32 [B] (a label >= 0, or < 0: in no room), num_bits int32 [B], muted / dtx [B] or None.
        Up to two ticks in flight; the arrays may be reused at once."""
        B, _alive, head = self._tick_begin_args(packets, packet_bytes, rooms, muted, flags, stream_ids)
        bits, d = _np(num_bits, np.int32, (B,)), _np01(dtx, (B,))
        self._tick_begin("bridge", self.L.lyra_hip_bridge_begin, B, *head, bits.ctypes.data, None if d is None else d.ctypes.data)

    def bridge_end(self):
        """-> (out_packets uint8 [B][23], zero behind each packet's bytes; out_packet_bytes, is_noise, is_comfort_noise int32
        [B]) of the OLDEST tick begun by bridge_begin."""
        return self._tick_end("bridge", self.L.lyra_hip_bridge_end, 3, False)

    def bridge_errors(self, clear=False):
        """d_order entries outside [0, B) that the bridge's mix skipped (synchronises)."""
        return self._error_count(self.L.lyra_hip_bridge_errors, clear)

    # -- the bridge with loudest-N selection (include/lyra_hip_speakers.h) -----------------------------
    def speakers_mix_dev(self, d_pcm16, d_order, d_room_start, d_mix, max_speakers, d_muted=None, d_is_comfort_noise=None,
                         d_levels=None, d_is_speaker=None):
        """The selection mix alone (lyra_hip_speakers_mix_dev): the buffers of bridge_mix_dev; max_speakers in
        1 .. SPEAKERS_MAX; d_levels int64 [B] and d_is_speaker int32 [B]: optional outputs, written for every row.  Row b of
        d_mix receives the clamped sum of the max_speakers loudest sources of its room, itself left out.  Bad d_order entries
        are skipped and counted in bridge_errors.  Completes on the encode-side stream."""
        B = d_pcm16.shape[0]
        sel = self._p_selection(max_speakers, d_levels, d_is_speaker, B)
        self._dev_call(self.L.lyra_hip_speakers_mix_dev, self._p_pcm(d_pcm16, B), B,
                       *self._p_mix_sources(d_order, d_room_start, d_muted, d_is_comfort_noise, B), sel[0],
                       self._p_pcm(d_mix, B), *sel[1:])

    def speakers_tick_dev(self, d_ids, d_packets, d_packet_bytes, d_order, d_room_start, d_num_bits, d_out_packets,
                          d_out_packet_bytes, max_speakers, d_muted=None, d_dtx=None, flags=0, d_pcm16=None, d_mix=None,
                          d_is_noise=None, d_is_comfort_noise=None, d_levels=None, d_is_speaker=None):
        """One tick of the bridge with selection (lyra_hip_speakers_tick_dev): bridge_tick_dev with the mix of
        speakers_mix_dev (flags: SPEAKERS_SKIP_COMFORT_NOISE) and its two further optional outputs, d_levels int64 [B] and
        d_is_speaker int32 [B].  Bit for bit the three calls in a row, outputs and stream state."""
        B, head = self._p_tick_head(d_ids, d_packets, d_packet_bytes, d_order, d_room_start, d_muted, flags)
        t = SpeakersTick(*head, *self._p_listener_bits(d_num_bits, d_dtx, B),
                         *self._p_tick_outputs(d_out_packets, d_out_packet_bytes, d_pcm16, B),
                         self._opt_dev_ptr(d_mix, "int16", (B, HOP), "mix"),
                         *self._p_noise_flags(d_is_noise, d_is_comfort_noise, B),
                         *self._p_selection(max_speakers, d_levels, d_is_speaker, B))
        self._dev_call(self.L.lyra_hip_speakers_tick_dev, C.addressof(t))

    def speakers_begin(self, packets, packet_bytes, rooms, num_bits, max_speakers, muted=None, dtx=None, flags=0,
                       stream_ids=None):
        """Pipelined tick of the bridge with selection from host arrays (lyra_hip_speakers_begin): the arrays of bridge_begin
        and max_speakers in 1 .. SPEAKERS_MAX.  Up to two ticks in flight, bridge_begin's included."""
        B, _alive, head = self._tick_begin_args(packets, packet_bytes, rooms, muted, flags, stream_ids)
        bits, d = _np(num_bits, np.int32, (B,)), _np01(dtx, (B,))
        self._tick_begin("speakers", self.L.lyra_hip_speakers_begin, B, *head, bits.ctypes.data,
                         None if d is None else d.ctypes.data, int(max_speakers))

    def speakers_end(self):
        """-> (out_packets uint8 [B][23], out_packet_bytes, is_noise, is_comfort_noise int32 [B], levels int64 [B], is_speaker
        int32 [B]) of the OLDEST tick in flight, which must be one begun by speakers_begin."""
        return self._tick_end("speakers", self.L.lyra_hip_speakers_end, 4, True)

    # -- the bridge with shared encoders (include/lyra_hip_shared_bridge.h) ------------------------------
    def _p_slot_table(self, d_room_keys, d_slots, n_rooms):
        """-> (d_room_keys, d_slots, n_table_rooms) of shared_mix_dev and the shared tick struct"""
        n_table = d_slots.shape[0]
        return (self._opt_dev_ptr(d_room_keys, "int32", (n_rooms,), "room keys"),
                self._dev_ptr(d_slots, "int32", (n_table, SHARED_SLOTS), "slot table"), n_table)

    def shared_mix_dev(self, d_pcm16, d_ids, d_order, d_room_start, d_slots, d_enc_mix, max_speakers, d_room_keys=None,
                       d_muted=None, d_is_comfort_noise=None, d_levels=None, d_is_speaker=None, d_slot_of=None):
        """Levels, selection, slot update and the encoder mixes alone (lyra_hip_shared_mix_dev): d_pcm16 int16 [B][320], d_ids
        int32 [B] the participants' stream ids, the index of bridge_mix_dev, d_slots int32 [n_table_rooms][SHARED_SLOTS] (in and
        out; -1: a free slot), d_room_keys int32 [n_rooms] or None (room r uses table row r), d_enc_mix int16
        [n_rooms * (1 + max_speakers)][320]; d_levels int64 [B], d_is_speaker and d_slot_of int32 [B]: optional outputs.
        Completes on the encode-side stream."""
        B = d_pcm16.shape[0]
        n_rooms = d_room_start.shape[0] - 1
        E = n_rooms * (1 + int(max_speakers))
        sel = self._p_selection(max_speakers, d_levels, d_is_speaker, B)
        self._dev_call(self.L.lyra_hip_shared_mix_dev, self._p_pcm(d_pcm16, B), self._p_ids(d_ids, B), B,
                       *self._p_mix_sources(d_order, d_room_start, d_muted, d_is_comfort_noise, B), sel[0],
                       *self._p_slot_table(d_room_keys, d_slots, n_rooms),
                       self._dev_ptr(d_enc_mix, "int16", (E, HOP), "encoder mixes"), *sel[1:],
                       self._opt_dev_ptr(d_slot_of, "int32", (B,), "slot_of"))

    def shared_tick_dev(self, d_ids, d_packets, d_packet_bytes, d_order, d_room_start, d_out_packets, d_out_packet_bytes,
                        max_speakers, d_slots, d_enc_ids, d_enc_num_bits, d_room_keys=None, d_enc_dtx=None, d_muted=None,
                        flags=0, d_pcm16=None, d_is_noise=None, d_is_comfort_noise=None, d_levels=None, d_is_speaker=None,
                        d_enc_mix=None, d_enc_packets=None, d_enc_packet_bytes=None, d_slot_of=None):
        """One tick of the bridge with shared encoders (lyra_hip_shared_tick_dev): the decode leg and the selection of
        speakers_tick_dev, then ONE encode_streams_dev call on E = n_rooms * (1 + max_speakers) encoder rows (d_enc_ids,
        d_enc_num_bits, d_enc_dtx int32 [E]: bitrate and DTX belong to a room and a slot, not to a listener) and the fan-out of
        the E packets into d_out_packets uint8 [B][23] / d_out_packet_bytes int32 [B].  d_slots / d_room_keys as in
        shared_mix_dev.  Optional outputs: d_pcm16, d_is_noise, d_is_comfort_noise, d_levels, d_is_speaker, d_slot_of [B];
        d_enc_mix int16 [E][320], d_enc_packets uint8 [E][23], d_enc_packet_bytes int32 [E]."""
        B, head = self._p_tick_head(d_ids, d_packets, d_packet_bytes, d_order, d_room_start, d_muted, flags)
        n_rooms = d_room_start.shape[0] - 1
        E = n_rooms * (1 + int(max_speakers))
        t = SharedTick(*head, *self._p_tick_outputs(d_out_packets, d_out_packet_bytes, d_pcm16, B),
                       *self._p_noise_flags(d_is_noise, d_is_comfort_noise, B),
                       *self._p_selection(max_speakers, d_levels, d_is_speaker, B),
                       *self._p_slot_table(d_room_keys, d_slots, n_rooms),
                       self._dev_ptr(d_enc_ids, "int32", (E,), "encoder stream ids") if E else None,
                       self._dev_ptr(d_enc_num_bits, "int32", (E,), "encoder num_bits") if E else None,
                       self._opt_dev_ptr(d_enc_dtx, "int32", (E,), "encoder dtx flags"),
                       self._opt_dev_ptr(d_enc_mix, "int16", (E, HOP), "encoder mixes"),
                       self._opt_dev_ptr(d_enc_packets, "uint8", (E, MAX_PACKET_BYTES), "encoder packets"),
                       self._opt_dev_ptr(d_enc_packet_bytes, "int32", (E,), "encoder packet sizes"),
                       self._opt_dev_ptr(d_slot_of, "int32", (B,), "slot_of"))
        self._dev_call(self.L.lyra_hip_shared_tick_dev, C.addressof(t))

    def shared_begin(self, packets, packet_bytes, rooms, max_speakers, room_labels, enc_ids, enc_bits, enc_dtx=None,
                     muted=None, flags=0, stream_ids=None):
        """Pipelined tick of the bridge with shared encoders from host arrays (lyra_hip_shared_begin): packets, packet_bytes,
        rooms, muted as bridge_begin; room_labels int32 [n_rooms], strictly ascending and exactly the labels >= 0 present in
        rooms; enc_ids / enc_bits / enc_dtx int32 [n_rooms][1 + max_speakers]: the encoder stream, bit count and DTX switch of
        every room's common row and slots.  The slot table is the context's, one row per label.  Up to two ticks in flight,
        bridge_begin's and speakers_begin's included."""
        B, _alive, head = self._tick_begin_args(packets, packet_bytes, rooms, muted, flags, stream_ids)
        keys, eids, ebits = (_np(a, np.int32, (-1,)) for a in (room_labels, enc_ids, enc_bits))
        d = _np01(enc_dtx, (-1,))
        if 1 <= int(max_speakers) <= SPEAKERS_MAX:    # (anything else the library refuses before it reads an array)
            E = keys.size * (1 + int(max_speakers))
            if eids.size != E or ebits.size != E or (d is not None and d.size != E):
                raise LyraHipError(f"shared_begin: enc_ids, enc_bits and enc_dtx take {keys.size} x (1 + {int(max_speakers)}) entries")
        self._tick_begin("shared", self.L.lyra_hip_shared_begin, B, *head, int(max_speakers), keys.ctypes.data, keys.size,
                         eids.ctypes.data, ebits.ctypes.data, None if d is None else d.ctypes.data)

    def shared_end(self):
        """-> (out_packets uint8 [B][23], out_packet_bytes, is_noise, is_comfort_noise int32 [B], levels int64 [B], is_speaker,
        slot_of int32 [B]) of the OLDEST tick in flight, which must be one begun by shared_begin."""
        return self._tick_end("shared", self.L.lyra_hip_shared_end, 5, True)

    def shared_reset_rooms(self, room_labels):
        """Drain the context and free the slot-table rows of these room labels (lyra_hip_shared_reset_rooms)."""
        keys = _np(room_labels, np.int32, (-1,))
        self._chk(self.L.lyra_hip_shared_reset_rooms(self.h, keys.ctypes.data, keys.size))

    def rates_errors(self, clear=False):
        """Sample rates seen by encode_rates_dev / decode_lossy_rates_dev / run_steps with d_rates that are no codec rate
        (synchronises)."""
        return self._error_count(self.L.lyra_hip_rates_errors, clear)

    def decode_samples_dev(self, d_ids, d_packets, d_packet_bytes, num_samples, sample_rate_hz, d_pcm_ext=None,
                           d_is_noise=None, d_is_comfort_noise=None):
        """LyraDecoder::SetEncodedPacket (rows with a packet) + DecodeSamples(num_samples) for request sizes that are not
        tied to the hop (lyra_hip_decode_samples_dev): d_packets uint8 [B][MAX_PACKET_BYTES], d_packet_bytes int32 [B] (0 = no
        packet, 8 / 15 / 23 = a packet, anything else counted in decode_samples_errors); 0 <= num_samples <= rate / 50 with
        num_samples * 16000 divisible by the rate; d_pcm_ext int16 [B][num_samples] (may be None when num_samples == 0);
        d_is_noise / d_is_comfort_noise int32 [B] optional.  The outputs complete on the noise stream."""
        B = d_packets.shape[0]
        self._dev_call(self.L.lyra_hip_decode_samples_dev, self._p_ids(d_ids, B), B,
                       self._p_packets(d_packets, B, MAX_PACKET_BYTES), self._p_packet_bytes(d_packet_bytes, B),
                       num_samples, sample_rate_hz, self._opt_dev_ptr(d_pcm_ext, "int16", (B, num_samples), "pcm"),
                       *self._p_noise_flags(d_is_noise, d_is_comfort_noise, B))

    def decode_samples_any_dev(self, d_ids, d_packets, d_packet_bytes, num_samples, sample_rate_hz, d_pcm_ext=None,
                               d_is_noise=None, d_is_comfort_noise=None):
        """decode_samples_dev for ANY request size of 0 .. 4 hops (lyra_hip_decode_samples_any_dev): BufferedResampler's
        leftover is part of the stream, and a request above one hop runs the reference loop in up to four rounds inside the
        call.  Arguments as decode_samples_dev; 0 <= num_samples <= 4 * rate / 50."""
        B = d_packets.shape[0]
        self._dev_call(self.L.lyra_hip_decode_samples_any_dev, self._p_ids(d_ids, B), B,
                       self._p_packets(d_packets, B, MAX_PACKET_BYTES), self._p_packet_bytes(d_packet_bytes, B),
                       num_samples, sample_rate_hz, self._opt_dev_ptr(d_pcm_ext, "int16", (B, num_samples), "pcm"),
                       *self._p_noise_flags(d_is_noise, d_is_comfort_noise, B))

    def decode_samples_any_begin(self, packets, packet_bytes, num_samples, sample_rate_hz, stream_ids=None):
        """Pipelined host-buffer form (lyra_hip_decode_samples_any_begin): packets uint8 [B][MAX_PACKET_BYTES], packet_bytes
        int32 [B].  Up to two requests in flight; the arrays may be reused at once."""
        packets, B, ids = self._rows(packets, np.uint8, MAX_PACKET_BYTES, stream_ids)
        sizes = _np(packet_bytes, np.int32, (B,))
        self._chk(self.L.lyra_hip_decode_samples_any_begin(self.h, ids.ctypes.data, B, packets.ctypes.data, sizes.ctypes.data,
                                                           num_samples, sample_rate_hz))
        self._pending_any_decodes.append((B, num_samples))

    def decode_samples_any_end(self):
        """-> pcm int16 [B][num_samples] of the OLDEST request begun by decode_samples_any_begin."""
        if not self._pending_any_decodes:
            self._chk(self.L.lyra_hip_decode_samples_any_end(self.h, None))
        B, n = self._pending_any_decodes[0]
        out = np.empty((B, n), np.int16)
        rc = self.L.lyra_hip_decode_samples_any_end(self.h, out.ctypes.data)
        self._pending_any_decodes.pop(0)   # (the library gives the slot back whatever the wait returns)
        self._chk(rc)
        return out

    def decode_samples_streams_dev(self, d_ids, d_packets, d_packet_bytes, d_sample_rates, d_num_samples, max_hops, d_pcm,
                                   d_pcm_offsets=None, d_is_noise=None, d_is_comfort_noise=None, n_pcm_samples=None):
        """decode_samples_any_dev with a sample rate, a request size and an output offset PER ROW
        (lyra_hip_decode_samples_streams_dev): d_sample_rates / d_num_samples int32 [B]; max_hops 1..4: the rounds the call
        enqueues (a row needs ceil(n * 16000 / rate) <= 320 * max_hops); d_pcm int16, any shape: row b's d_num_samples[b]
        samples go to d_pcm_offsets[b] (int32 [B], any alignment; None: b * 4 * MAX_EXT_HOP); n_pcm_samples: how much of d_pcm
        the rows may lie in (None: all of it).  A row with a bad rate, size or offset, or one that needs more rounds, runs as a
        row without a packet and with a request of 0 samples and is counted in rates_errors."""
        B = d_sample_rates.shape[0]
        if n_pcm_samples is None:
            n_pcm_samples = d_pcm.numel()
        elif n_pcm_samples > d_pcm.numel():
            raise LyraHipError(f"pcm: n_pcm_samples {n_pcm_samples} exceeds the tensor's {d_pcm.numel()} samples")
        self._dev_call(self.L.lyra_hip_decode_samples_streams_dev, self._p_ids(d_ids, B), B,
                       self._p_packets(d_packets, B, MAX_PACKET_BYTES), self._p_packet_bytes(d_packet_bytes, B),
                       self._dev_ptr(d_sample_rates, "int32", (B,), "sample rates"),
                       self._dev_ptr(d_num_samples, "int32", (B,), "request sizes"), int(max_hops),
                       self._dev_ptr(d_pcm, "int16", tuple(d_pcm.shape), "pcm"), int(n_pcm_samples),
                       self._opt_dev_ptr(d_pcm_offsets, "int32", (B,), "pcm offsets"),
                       *self._p_noise_flags(d_is_noise, d_is_comfort_noise, B))

    def decode_samples_streams_begin(self, packets, packet_bytes, sample_rates, num_samples, stream_ids=None):
        """Pipelined host-buffer form (lyra_hip_decode_samples_streams_begin): packets uint8 [B][MAX_PACKET_BYTES],
        packet_bytes, sample_rates and num_samples int32 [B].  Up to two requests in flight; the arrays may be reused at once."""
        packets, B, ids = self._rows(packets, np.uint8, MAX_PACKET_BYTES, stream_ids)
        sizes = _np(packet_bytes, np.int32, (B,))
        rates = _np(sample_rates, np.int32, (B,))
        ns = _np(num_samples, np.int32, (B,))
        total = int(np.maximum(ns, 0).astype(np.int64).sum())   # (what end() sizes its array by: before the call)
        self._chk(self.L.lyra_hip_decode_samples_streams_begin(self.h, ids.ctypes.data, B, packets.ctypes.data, sizes.ctypes.data,
                                                               rates.ctypes.data, ns.ctypes.data))
        self._pending_sample_stream_decodes.append((B, total))

    def decode_samples_streams_end(self):
        """-> (pcm int16, PACKED: row b holds num_samples[b] samples, rows back to back in batch order; is_noise int32 [B];
        is_comfort_noise int32 [B]) of the OLDEST request begun by decode_samples_streams_begin."""
        if not self._pending_sample_stream_decodes:
            self._chk(self.L.lyra_hip_decode_samples_streams_end(self.h, None, None, None))
        B, total = self._pending_sample_stream_decodes[0]
        pcm = np.empty(total, np.int16)
        noise = np.empty(B, np.int32)
        cn = np.empty(B, np.int32)
        rc = self.L.lyra_hip_decode_samples_streams_end(self.h, pcm.ctypes.data if total else None, noise.ctypes.data,
                                                        cn.ctypes.data)
        self._pending_sample_stream_decodes.pop(0)   # (the library gives the slot back whatever the wait returns)
        self._chk(rc)
        return pcm, noise, cn

    def decode_samples_errors(self, clear=False):
        """Invalid packet sizes plus packets that found the feature FIFO full, seen by decode_samples_dev (synchronises)."""
        return self._error_count(self.L.lyra_hip_decode_samples_errors, clear)

    # -- stream state as blobs (lyra_hip_export_streams / lyra_hip_import_streams) -------------------------------------
    def stream_blob_bytes(self):
        """Bytes of one stream's state blob (a multiple of 256)."""
        return self.L.lyra_hip_stream_blob_bytes()

    def export_streams(self, stream_ids):
        """The whole codec state of the listed streams -> uint8 [B][stream_blob_bytes()].  Drains the context."""
        ids = _np(stream_ids, np.int32, (-1,))
        out = np.empty((ids.size, self.stream_blob_bytes()), np.uint8)
        self._chk(self.L.lyra_hip_export_streams(self.h, ids.ctypes.data, ids.size, out.ctypes.data))
        return out

    def import_streams(self, stream_ids, blobs, sides=STATE_BOTH):
        """Replace the state of stream_ids[b] by blobs[b] (uint8 [B][stream_blob_bytes()]); sides: STATE_ENCODER,
        STATE_DECODER or both.  Every blob is validated first: one bad blob and nothing changes (LyraHipError)."""
        ids = _np(stream_ids, np.int32, (-1,))
        blobs = _np(blobs, np.uint8, (ids.size, self.stream_blob_bytes()))
        self._chk(self.L.lyra_hip_import_streams(self.h, ids.ctypes.data, ids.size, blobs.ctypes.data, sides))

    def export_streams_dev(self, d_ids, d_blobs):
        """export_streams on device buffers: d_ids int32 [B] (-1 skips the row), d_blobs uint8 [B][stream_blob_bytes()]."""
        B = d_ids.shape[0]
        self._dev_call(self.L.lyra_hip_export_streams_dev, self._p_ids(d_ids, B), B,
                       self._dev_ptr(d_blobs, "uint8", (B, self.stream_blob_bytes()), "blobs"))

    def import_streams_dev(self, d_ids, d_blobs, sides=STATE_BOTH):
        """import_streams on device buffers.  A blob that fails validation is skipped on the device, its target stream
        left untouched and counted in import_errors(); the other rows are imported."""
        B = d_ids.shape[0]
        self._dev_call(self.L.lyra_hip_import_streams_dev, self._p_ids(d_ids, B), B,
                       self._dev_ptr(d_blobs, "uint8", (B, self.stream_blob_bytes()), "blobs"), sides)

    def import_errors(self, clear=False):
        """Blob rows import_streams_dev refused (synchronises)."""
        return self._error_count(self.L.lyra_hip_import_errors, clear)

    # -- time-parallel spans (lyra_hip_encode_spans / lyra_hip_decode_spans) ----------------------------------------------
    @staticmethod
    def _span_hop(sample_rate_hz):
        if sample_rate_hz not in (8000, 16000, 32000, 48000):
            raise LyraHipError(f"spans: sample rate {sample_rate_hz} Hz (8000 / 16000 / 32000 / 48000)")
        return sample_rate_hz // 50

    @staticmethod
    def _span_args(spans, lane_ids, frames):
        """spans and lanes of a call on buffers of `frames` frames -> the C arguments (spans, n_spans, lane_ids, n_lanes) and
        the arrays they point into, which the caller holds until the call has returned"""
        sp = _spans(spans)
        lanes = np.ascontiguousarray(np.asarray(lane_ids, np.int32).reshape(-1))
        if sp.size and (np.any(sp["first_frame"] < 0) or np.any(sp["n_frames"] < 0) or
                        int(np.max(sp["first_frame"] + sp["n_frames"])) > frames):
            raise LyraHipError(f"spans: a span lies outside the {frames} frames of the buffer")
        return (sp.ctypes.data, sp.size, lanes.ctypes.data, lanes.size), (sp, lanes)

    def encode_spans(self, spans, pcm, num_bits, lane_ids=(), sample_rate_hz=16000):
        """Long spans of a few streams, time-parallel and bit for bit the hop-by-hop result.  spans: (stream_id,
        first_frame, n_frames) triples into the frame-major pcm int16 [frames][320]; lane_ids: streams lent as scratch
        (their encoder state is reset afterwards).  Returns packets uint8 [frames][bytes]; rows outside every span are 0.
        sample_rate_hz other than 16000 (lyra_hip_encode_spans_ext): pcm is [frames][sample_rate_hz / 50] and the result that
        of resample(side="encoder") + encode per hop."""
        pcm = _np(pcm, np.int16, (-1, self._span_hop(sample_rate_hz)))
        out = np.zeros((pcm.shape[0], packet_size(num_bits)), np.uint8)
        a, _held = self._span_args(spans, lane_ids, pcm.shape[0])
        if sample_rate_hz == 16000:
            self._chk(self.L.lyra_hip_encode_spans(self.h, *a, pcm.ctypes.data, num_bits, out.ctypes.data))
        else:
            self._chk(self.L.lyra_hip_encode_spans_ext(self.h, *a, pcm.ctypes.data, sample_rate_hz, num_bits, out.ctypes.data))
        return out

    def decode_spans(self, spans, packets, num_bits, lane_ids=(), sample_rate_hz=16000):
        """The decoder twin of encode_spans: packets uint8 [frames][bytes] -> pcm int16 [frames][320] (rows outside every
        span are 0); the lanes' decoder state is reset afterwards.  sample_rate_hz other than 16000
        (lyra_hip_decode_spans_ext): pcm int16 [frames][sample_rate_hz / 50], that of decode + resample(side="decoder")."""
        packets = _np(packets, np.uint8, (-1, packet_size(num_bits)))
        out = np.zeros((packets.shape[0], self._span_hop(sample_rate_hz)), np.int16)
        a, _held = self._span_args(spans, lane_ids, packets.shape[0])
        if sample_rate_hz == 16000:
            self._chk(self.L.lyra_hip_decode_spans(self.h, *a, packets.ctypes.data, num_bits, out.ctypes.data))
        else:
            self._chk(self.L.lyra_hip_decode_spans_ext(self.h, *a, packets.ctypes.data, num_bits, sample_rate_hz, out.ctypes.data))
        return out

    def encode_spans_dev(self, spans, d_pcm, num_bits, d_packets, lane_ids=(), sample_rate_hz=16000, d_pcm16=None):
        """encode_spans on device buffers (spans and lane_ids stay host lists): d_pcm int16 [frames][320], d_packets uint8
        [frames][bytes].  Enqueues and does not synchronise.  sample_rate_hz other than 16000
        (lyra_hip_encode_spans_ext_dev): d_pcm is [frames][sample_rate_hz / 50] and d_pcm16 int16 [frames][320] the caller's
        workspace, which holds the resampled audio of the spans' frames afterwards."""
        F = d_pcm.shape[0]
        a, _held = self._span_args(spans, lane_ids, F)
        if sample_rate_hz == 16000 and d_pcm16 is None:
            self._dev_call(self.L.lyra_hip_encode_spans_dev, *a, self._p_pcm(d_pcm, F), num_bits,
                           self._p_packets(d_packets, F, packet_size(num_bits)))
            return
        self._dev_call(self.L.lyra_hip_encode_spans_ext_dev, *a, self._dev_ptr(d_pcm, "int16", (F, sample_rate_hz // 50), "pcm"),
                       sample_rate_hz, self._opt_dev_ptr(d_pcm16, "int16", (F, HOP), "16 kHz pcm"), num_bits,
                       self._p_packets(d_packets, F, packet_size(num_bits)))

    def decode_spans_dev(self, spans, d_packets, num_bits, d_pcm, lane_ids=(), sample_rate_hz=16000, d_pcm16=None):
        """decode_spans on device buffers.  Enqueues and does not synchronise.  sample_rate_hz other than 16000
        (lyra_hip_decode_spans_ext_dev): d_pcm is [frames][sample_rate_hz / 50] and d_pcm16 int16 [frames][320] receives the
        16 kHz output; all of it completes on the decode stream."""
        F = d_pcm.shape[0]
        a, _held = self._span_args(spans, lane_ids, F)
        if sample_rate_hz == 16000 and d_pcm16 is None:
            self._dev_call(self.L.lyra_hip_decode_spans_dev, *a, self._p_packets(d_packets, F, packet_size(num_bits)), num_bits,
                           self._p_pcm(d_pcm, F))
            return
        self._dev_call(self.L.lyra_hip_decode_spans_ext_dev, *a, self._p_packets(d_packets, F, packet_size(num_bits)),
                       num_bits, sample_rate_hz, self._opt_dev_ptr(d_pcm16, "int16", (F, HOP), "16 kHz pcm"),
                       self._dev_ptr(d_pcm, "int16", (F, sample_rate_hz // 50), "pcm"))

    # -- DTX on spans (lyra_hip_encode_spans_dtx / lyra_hip_noise_spans) -------------------------------------------------------
    def encode_spans_dtx(self, spans, pcm, num_bits, lane_ids=(), sample_rate_hz=16000):
        """encode_spans with enable_dtx: bit for bit resample(side="encoder") + encode_dtx per hop.  pcm int16
        [frames][sample_rate_hz / 50]; sample_rate_hz must be the rate given to set_encoder_sample_rate.  Returns (packets uint8
        [frames][bytes], packet_bytes int32 [frames]); rows of noise frames and rows outside every span are 0."""
        pcm = _np(pcm, np.int16, (-1, self._span_hop(sample_rate_hz)))
        out = np.zeros((pcm.shape[0], packet_size(num_bits)), np.uint8)
        nbytes = np.zeros(pcm.shape[0], np.int32)
        a, _held = self._span_args(spans, lane_ids, pcm.shape[0])
        self._chk(self.L.lyra_hip_encode_spans_dtx(self.h, *a, pcm.ctypes.data, sample_rate_hz, num_bits, out.ctypes.data,
                                                   nbytes.ctypes.data))
        return out, nbytes

    def encode_spans_dtx_dev(self, spans, d_pcm, num_bits, d_packets, d_packet_bytes, lane_ids=(), sample_rate_hz=16000,
                             d_pcm16=None):
        """encode_spans_dtx on device buffers: d_pcm int16 [frames][sample_rate_hz / 50], d_packets uint8 [frames][bytes] (rows
        of noise frames are not written), d_packet_bytes int32 [frames], d_pcm16 int16 [frames][320] the 16 kHz workspace (not
        needed at 16000).  Blocks the host once, until the noise decisions are known; the steps behind are only enqueued."""
        F = d_pcm.shape[0]
        a, _held = self._span_args(spans, lane_ids, F)
        self._dev_call(self.L.lyra_hip_encode_spans_dtx_dev, *a,
                       self._dev_ptr(d_pcm, "int16", (F, self._span_hop(sample_rate_hz)), "pcm"), sample_rate_hz,
                       self._opt_dev_ptr(d_pcm16, "int16", (F, HOP), "16 kHz pcm"), num_bits,
                       self._p_packets(d_packets, F, packet_size(num_bits)),
                       self._opt_dev_ptr(d_packet_bytes, "int32", (F,), "packet_bytes"))

    def noise_spans(self, spans, pcm, side="encoder"):
        """NoiseEstimator::ReceiveSamples over every frame of every span of pcm int16 [frames][320] -> is_noise int32 [frames]
        (what noise_receive returns per hop; rows outside every span are 0)."""
        pcm = _np(pcm, np.int16, (-1, HOP))
        out = np.zeros(pcm.shape[0], np.int32)
        a, _held = self._span_args(spans, (), pcm.shape[0])
        self._chk(self.L.lyra_hip_noise_spans(self.h, self._SIDES[side], *a[:2], pcm.ctypes.data, out.ctypes.data))
        return out

    def noise_spans_dev(self, spans, d_pcm, d_is_noise, side="encoder"):
        """noise_spans on device buffers; enqueues and does not synchronise."""
        F = d_pcm.shape[0]
        a, _held = self._span_args(spans, (), F)
        self._dev_call(self.L.lyra_hip_noise_spans_dev, self._SIDES[side], *a[:2],
                       self._p_pcm(d_pcm, F), self._dev_ptr(d_is_noise, "int32", (F,), "is_noise"))

    # -- packet loss on spans (lyra_hip_decode_spans_lossy) -------------------------------------------------------------------
    @staticmethod
    def _span_packet_bytes(packet_bytes, frames, name="packet_bytes"):
        pb = np.ascontiguousarray(np.asarray(packet_bytes, np.int32).reshape(-1))
        if pb.size != frames:
            raise LyraHipError(f"spans: {name} has {pb.size} entries for {frames} frames")
        return pb

    def decode_spans_lossy(self, spans, packets, packet_bytes, num_bits, lane_ids=(), sample_rate_hz=16000):
        """decode_lossy_dev per hop over long spans, time-parallel and bit for bit: packets uint8 [frames][bytes], packet_bytes
        int32 [frames] (0 = no packet: lost, or DTX's empty packet).  Returns (pcm16 int16 [frames][320], pcm_ext int16
        [frames][sample_rate_hz / 50] or None at 16000, is_noise int32 [frames], is_comfort_noise int32 [frames]); rows outside
        every span are 0.  The lanes' decoder stage state is reset afterwards."""
        packets = _np(packets, np.uint8, (-1, packet_size(num_bits)))
        F = packets.shape[0]
        pb = self._span_packet_bytes(packet_bytes, F)
        pcm16 = np.zeros((F, HOP), np.int16)
        ext = np.zeros((F, self._span_hop(sample_rate_hz)), np.int16) if sample_rate_hz != 16000 else None
        is_noise, is_cn = np.zeros(F, np.int32), np.zeros(F, np.int32)
        a, _held = self._span_args(spans, lane_ids, F)
        self._chk(self.L.lyra_hip_decode_spans_lossy(self.h, *a, packets.ctypes.data, pb.ctypes.data, num_bits, sample_rate_hz,
                                                     pcm16.ctypes.data, ext.ctypes.data if ext is not None else None,
                                                     is_noise.ctypes.data, is_cn.ctypes.data))
        return pcm16, ext, is_noise, is_cn

    def decode_spans_lossy_dev(self, spans, d_packets, packet_bytes, num_bits, d_pcm16, lane_ids=(), sample_rate_hz=16000,
                               d_pcm_ext=None, d_is_noise=None, d_is_comfort_noise=None):
        """decode_spans_lossy on device buffers; packet_bytes stays a host array like spans and lane_ids.  d_pcm16 int16
        [frames][320] is required, d_pcm_ext int16 [frames][sample_rate_hz / 50] at a rate other than 16000, d_is_noise /
        d_is_comfort_noise int32 [frames] are optional.  Blocks the host once, at its start, for the span streams' control words;
        everything else is enqueued on the decode stream."""
        F = d_packets.shape[0]
        pb = self._span_packet_bytes(packet_bytes, F)
        a, _held = self._span_args(spans, lane_ids, F)
        self._dev_call(self.L.lyra_hip_decode_spans_lossy_dev, *a,
                       self._p_packets(d_packets, F, packet_size(num_bits)), pb.ctypes.data, num_bits,
                       sample_rate_hz, self._dev_ptr(d_pcm16, "int16", (F, HOP), "16 kHz pcm"),
                       self._opt_dev_ptr(d_pcm_ext, "int16", (F, self._span_hop(sample_rate_hz)), "external-rate pcm"),
                       *self._p_noise_flags(d_is_noise, d_is_comfort_noise, F))

    # -- per-frame bitrates on spans (include/lyra_hip_spans_mixed.h) -----------------------------------------------------------
    def encode_spans_mixed(self, spans, pcm, num_bits, lane_ids=(), sample_rate_hz=16000, dtx=False):
        """encode_spans with a bit count per frame: bit for bit encode_mixed_dev per hop with that hop's count.  pcm int16
        [frames][sample_rate_hz / 50], num_bits int32 [frames] (a multiple of 4 in 4..184 on every span frame); dtx as
        encode_spans_dtx.  Returns (packets uint8 [frames][23], packet_bytes int32 [frames]); bytes past a row's packet_bytes,
        rows of noise frames and rows outside every span are 0."""
        pcm = _np(pcm, np.int16, (-1, self._span_hop(sample_rate_hz)))
        F = pcm.shape[0]
        bits = self._span_packet_bytes(num_bits, F, "num_bits")
        out = np.zeros((F, MAX_PACKET_BYTES), np.uint8)
        nbytes = np.zeros(F, np.int32)
        a, _held = self._span_args(spans, lane_ids, F)
        self._chk(self.L.lyra_hip_encode_spans_mixed(self.h, *a, pcm.ctypes.data, sample_rate_hz, bits.ctypes.data, int(bool(dtx)),
                                                     out.ctypes.data, nbytes.ctypes.data))
        return out, nbytes

    def encode_spans_mixed_dev(self, spans, d_pcm, num_bits, d_packets, d_packet_bytes, lane_ids=(), sample_rate_hz=16000,
                               d_pcm16=None, dtx=False):
        """encode_spans_mixed on device buffers; num_bits stays a host array like spans and lane_ids.  d_pcm int16
        [frames][sample_rate_hz / 50], d_packets uint8 [frames][23] (bytes past a row's size are not written), d_packet_bytes int32
        [frames], d_pcm16 int16 [frames][320] the 16 kHz workspace (not needed at 16000).  Enqueues and does not synchronise,
        except with dtx, which blocks the host once as encode_spans_dtx_dev does."""
        F = d_pcm.shape[0]
        bits = self._span_packet_bytes(num_bits, F, "num_bits")
        a, _held = self._span_args(spans, lane_ids, F)
        self._dev_call(self.L.lyra_hip_encode_spans_mixed_dev, *a,
                       self._dev_ptr(d_pcm, "int16", (F, self._span_hop(sample_rate_hz)), "pcm"), sample_rate_hz,
                       self._opt_dev_ptr(d_pcm16, "int16", (F, HOP), "16 kHz pcm"), bits.ctypes.data, int(bool(dtx)),
                       self._p_packets(d_packets, F, MAX_PACKET_BYTES),
                       self._opt_dev_ptr(d_packet_bytes, "int32", (F,), "packet_bytes"))

    def decode_spans_lossy_mixed(self, spans, packets, packet_bytes, lane_ids=(), sample_rate_hz=16000):
        """decode_spans_lossy with the size chosen per frame: packets uint8 [frames][23], packet_bytes int32 [frames] in
        {0, 8, 15, 23}; bit for bit decode_lossy_mixed_dev per hop.  Returns what decode_spans_lossy returns."""
        packets = _np(packets, np.uint8, (-1, MAX_PACKET_BYTES))
        F = packets.shape[0]
        pb = self._span_packet_bytes(packet_bytes, F)
        pcm16 = np.zeros((F, HOP), np.int16)
        ext = np.zeros((F, self._span_hop(sample_rate_hz)), np.int16) if sample_rate_hz != 16000 else None
        is_noise, is_cn = np.zeros(F, np.int32), np.zeros(F, np.int32)
        a, _held = self._span_args(spans, lane_ids, F)
        self._chk(self.L.lyra_hip_decode_spans_lossy_mixed(self.h, *a, packets.ctypes.data, pb.ctypes.data, sample_rate_hz,
                                                           pcm16.ctypes.data, ext.ctypes.data if ext is not None else None,
                                                           is_noise.ctypes.data, is_cn.ctypes.data))
        return pcm16, ext, is_noise, is_cn

    def decode_spans_lossy_mixed_dev(self, spans, d_packets, packet_bytes, d_pcm16, lane_ids=(), sample_rate_hz=16000,
                                     d_pcm_ext=None, d_is_noise=None, d_is_comfort_noise=None):
        """decode_spans_lossy_mixed on device buffers, the arguments of decode_spans_lossy_dev without num_bits: d_packets uint8
        [frames][23], packet_bytes a host array.  Blocks the host once, at its start."""
        F = d_packets.shape[0]
        pb = self._span_packet_bytes(packet_bytes, F)
        a, _held = self._span_args(spans, lane_ids, F)
        self._dev_call(self.L.lyra_hip_decode_spans_lossy_mixed_dev, *a, self._p_packets(d_packets, F, MAX_PACKET_BYTES),
                       pb.ctypes.data, sample_rate_hz, self._dev_ptr(d_pcm16, "int16", (F, HOP), "16 kHz pcm"),
                       self._opt_dev_ptr(d_pcm_ext, "int16", (F, self._span_hop(sample_rate_hz)), "external-rate pcm"),
                       *self._p_noise_flags(d_is_noise, d_is_comfort_noise, F))

    spans_lossy_plan_mixed = staticmethod(spans_lossy_plan_mixed)

    # -- per-span sample rates on spans (include/lyra_hip_spans_rates.h) ---------------------------------------------------------
    @staticmethod
    def _span_rates(sample_rates, n_spans):
        rates = np.ascontiguousarray(np.asarray(sample_rates, np.int32).reshape(-1))
        if rates.size != n_spans:
            raise LyraHipError(f"spans: sample_rates has {rates.size} entries for {n_spans} spans")
        return rates

    def encode_spans_rates_dev(self, spans, d_pcm_ext, sample_rates, d_pcm16, num_bits, d_packets, d_packet_bytes, lane_ids=(),
                               dtx=False):
        """encode_spans_mixed_dev with a sample rate per span: bit for bit encode_rates_dev per hop.  sample_rates int32 [n_spans]
        from 8000 / 16000 / 32000 / 48000 and num_bits int32 [frames] stay host arrays like spans and lane_ids.  d_pcm_ext int16
        [frames][MAX_EXT_HOP], a frame of span s holds sample_rates[s] / 50 samples at the front of its row; d_pcm16 int16 [frames][320] (required: it receives the 16 kHz audio of every span frame),
        d_packets uint8 [frames][23], d_packet_bytes int32 [frames].  Enqueues and does not synchronise, except with dtx, which
        blocks the host once as encode_spans_dtx_dev does."""
        F = d_pcm_ext.shape[0]
        bits = self._span_packet_bytes(num_bits, F, "num_bits")
        a, _held = self._span_args(spans, lane_ids, F)
        rates = self._span_rates(sample_rates, a[1])
        self._dev_call(self.L.lyra_hip_encode_spans_rates_dev, *a,
                       self._dev_ptr(d_pcm_ext, "int16", (F, MAX_EXT_HOP), "external-rate pcm"), rates.ctypes.data,
                       self._opt_dev_ptr(d_pcm16, "int16", (F, HOP), "16 kHz pcm"), bits.ctypes.data, int(bool(dtx)),
                       self._p_packets(d_packets, F, MAX_PACKET_BYTES),
                       self._opt_dev_ptr(d_packet_bytes, "int32", (F,), "packet_bytes"))

    def decode_spans_lossy_rates_dev(self, spans, d_packets, packet_bytes, sample_rates, d_pcm16, d_pcm_ext, lane_ids=(),
                                     d_is_noise=None, d_is_comfort_noise=None):
        """decode_spans_lossy_mixed_dev with a sample rate per span: bit for bit decode_lossy_rates_dev per hop.  packet_bytes int32
        [frames] in {0, 8, 15, 23} and sample_rates stay host arrays; d_packets uint8 [frames][23], d_pcm16 int16 [frames][320] and d_pcm_ext
        int16 [frames][MAX_EXT_HOP] both required, d_is_noise / d_is_comfort_noise int32 [frames] optional.  Blocks the host
        once, at its start."""
        F = d_packets.shape[0]
        pb = self._span_packet_bytes(packet_bytes, F)
        a, _held = self._span_args(spans, lane_ids, F)
        rates = self._span_rates(sample_rates, a[1])
        self._dev_call(self.L.lyra_hip_decode_spans_lossy_rates_dev, *a, self._p_packets(d_packets, F, MAX_PACKET_BYTES),
                       pb.ctypes.data, rates.ctypes.data, self._opt_dev_ptr(d_pcm16, "int16", (F, HOP), "16 kHz pcm"),
                       self._opt_dev_ptr(d_pcm_ext, "int16", (F, MAX_EXT_HOP), "external-rate pcm"),
                       *self._p_noise_flags(d_is_noise, d_is_comfort_noise, F))

    def decode_spans_rates_dev(self, spans, d_packets, num_bits, sample_rates, d_pcm16, d_pcm_ext, lane_ids=()):
        """decode_spans_dev with a sample rate per span (no loss, one num_bits): bit for bit decode_dev + resample_dev(side="decoder")
        per hop.  d_packets uint8 [frames][bytes], d_pcm16 int16 [frames][320] and d_pcm_ext int16 [frames][MAX_EXT_HOP] both
        required; a frame of span s gets sample_rates[s] / 50 samples at the front of its d_pcm_ext row.  Enqueues and does not
        synchronise."""
        F = d_packets.shape[0]
        a, _held = self._span_args(spans, lane_ids, F)
        rates = self._span_rates(sample_rates, a[1])
        self._dev_call(self.L.lyra_hip_decode_spans_rates_dev, *a, self._p_packets(d_packets, F, packet_size(num_bits)), num_bits,
                       rates.ctypes.data, self._opt_dev_ptr(d_pcm16, "int16", (F, HOP), "16 kHz pcm"),
                       self._opt_dev_ptr(d_pcm_ext, "int16", (F, MAX_EXT_HOP), "external-rate pcm"))

    # -- per-span sample rates on a packed external-rate buffer (include/lyra_hip_spans_packed.h) --------------------------------
    spans_packed_layout = staticmethod(spans_packed_layout)

    @staticmethod
    def _span_offsets(ext_offsets, n_spans):
        """ext_offsets (None: the back-to-back layout) -> (C argument, the array it points into)"""
        if ext_offsets is None:
            return None, None
        off = np.ascontiguousarray(np.asarray(ext_offsets, np.int64).reshape(-1))
        if off.size != n_spans:
            raise LyraHipError(f"spans: ext_offsets has {off.size} entries for {n_spans} spans")
        return off.ctypes.data, off

    def encode_spans_packed_dev(self, spans, d_pcm_ext, sample_rates, d_pcm16, num_bits, d_packets, d_packet_bytes, lane_ids=(),
                                dtx=False, ext_offsets=None):
        """encode_spans_rates_dev on the packed layout: d_pcm_ext int16 [n_ext_samples] is flat, span s's frames lie back to back
        from ext_offsets[s] (int64 [n_spans], multiples of 8; None: the layout of spans_packed_layout), sample_rates[s] / 50
        samples each.  Every frame-major buffer -- d_pcm16 int16 [frames][320] (required), num_bits, d_packets uint8 [frames][23],
        d_packet_bytes int32 [frames] -- is indexed by first_frame as ever.  Bit for bit encode_spans_rates_dev."""
        F = d_pcm16.shape[0]
        bits = self._span_packet_bytes(num_bits, F, "num_bits")
        a, _held = self._span_args(spans, lane_ids, F)
        rates = self._span_rates(sample_rates, a[1])
        p_off, _off = self._span_offsets(ext_offsets, a[1])
        n_ext = int(d_pcm_ext.numel())
        self._dev_call(self.L.lyra_hip_encode_spans_packed_dev, *a,
                       self._dev_ptr(d_pcm_ext, "int16", (n_ext,), "external-rate pcm"), n_ext, p_off, rates.ctypes.data,
                       self._dev_ptr(d_pcm16, "int16", (F, HOP), "16 kHz pcm"), bits.ctypes.data, int(bool(dtx)),
                       self._p_packets(d_packets, F, MAX_PACKET_BYTES),
                       self._opt_dev_ptr(d_packet_bytes, "int32", (F,), "packet_bytes"))

    def decode_spans_lossy_packed_dev(self, spans, d_packets, packet_bytes, sample_rates, d_pcm16, d_pcm_ext, lane_ids=(),
                                      d_is_noise=None, d_is_comfort_noise=None, ext_offsets=None):
        """decode_spans_lossy_rates_dev on the packed layout (see encode_spans_packed_dev): span s gets exactly n_frames *
        sample_rates[s] / 50 samples from ext_offsets[s] of the flat d_pcm_ext, nothing else of it is written.  Blocks the host
        once, at its start."""
        F = d_packets.shape[0]
        pb = self._span_packet_bytes(packet_bytes, F)
        a, _held = self._span_args(spans, lane_ids, F)
        rates = self._span_rates(sample_rates, a[1])
        p_off, _off = self._span_offsets(ext_offsets, a[1])
        n_ext = int(d_pcm_ext.numel())
        self._dev_call(self.L.lyra_hip_decode_spans_lossy_packed_dev, *a, self._p_packets(d_packets, F, MAX_PACKET_BYTES),
                       pb.ctypes.data, rates.ctypes.data, self._dev_ptr(d_pcm16, "int16", (F, HOP), "16 kHz pcm"),
                       self._dev_ptr(d_pcm_ext, "int16", (n_ext,), "external-rate pcm"), n_ext, p_off,
                       *self._p_noise_flags(d_is_noise, d_is_comfort_noise, F))

    def decode_spans_packed_dev(self, spans, d_packets, num_bits, sample_rates, d_pcm16, d_pcm_ext, lane_ids=(), ext_offsets=None):
        """decode_spans_rates_dev (no loss, one num_bits) on the packed layout.  Enqueues and does not synchronise."""
        F = d_packets.shape[0]
        a, _held = self._span_args(spans, lane_ids, F)
        rates = self._span_rates(sample_rates, a[1])
        p_off, _off = self._span_offsets(ext_offsets, a[1])
        n_ext = int(d_pcm_ext.numel())
        self._dev_call(self.L.lyra_hip_decode_spans_packed_dev, *a, self._p_packets(d_packets, F, packet_size(num_bits)), num_bits,
                       rates.ctypes.data, self._dev_ptr(d_pcm16, "int16", (F, HOP), "16 kHz pcm"),
                       self._dev_ptr(d_pcm_ext, "int16", (n_ext,), "external-rate pcm"), n_ext, p_off)

    def encode_spans_packed(self, spans, pcm_ext, sample_rates, num_bits, lane_ids=(), dtx=False, ext_offsets=None):
        """encode_spans_packed_dev from host arrays: pcm_ext int16 [n_ext_samples] flat, num_bits int32 [frames].  Uploads exactly
        the spans' samples.  Returns (packets uint8 [frames][23], packet_bytes int32 [frames]); bytes past a row's size, rows of
        noise frames and rows outside every span are 0."""
        pcm_ext = _np(pcm_ext, np.int16, (-1,))
        bits = np.ascontiguousarray(np.asarray(num_bits, np.int32).reshape(-1))
        F = bits.size
        out = np.zeros((F, MAX_PACKET_BYTES), np.uint8)
        nbytes = np.zeros(F, np.int32)
        a, _held = self._span_args(spans, lane_ids, F)
        rates = self._span_rates(sample_rates, a[1])
        p_off, _off = self._span_offsets(ext_offsets, a[1])
        self._chk(self.L.lyra_hip_encode_spans_packed(self.h, *a, pcm_ext.ctypes.data, pcm_ext.size, p_off, rates.ctypes.data,
                                                      bits.ctypes.data, int(bool(dtx)), out.ctypes.data, nbytes.ctypes.data))
        return out, nbytes

    def decode_spans_lossy_packed(self, spans, packets, packet_bytes, sample_rates, n_ext_samples=None, lane_ids=(),
                                  ext_offsets=None):
        """decode_spans_lossy_packed_dev from host arrays: packets uint8 [frames][23], packet_bytes int32 [frames] in {0, 8, 15,
        23}.  n_ext_samples: the length of the flat output (None: that of the back-to-back layout).  Returns (pcm16 int16
        [frames][320], pcm_ext int16 [n_ext_samples], is_noise, is_comfort_noise int32 [frames]); everything outside the spans is 0."""
        packets = _np(packets, np.uint8, (-1, MAX_PACKET_BYTES))
        F = packets.shape[0]
        pb = self._span_packet_bytes(packet_bytes, F)
        a, _held = self._span_args(spans, lane_ids, F)
        rates = self._span_rates(sample_rates, a[1])
        p_off, _off = self._span_offsets(ext_offsets, a[1])
        if n_ext_samples is None:
            n_ext_samples = spans_packed_layout(_held[0], rates, self.L)[1]
        pcm16, ext = np.zeros((F, HOP), np.int16), np.zeros(int(n_ext_samples), np.int16)
        is_noise, is_cn = np.zeros(F, np.int32), np.zeros(F, np.int32)
        self._chk(self.L.lyra_hip_decode_spans_lossy_packed(self.h, *a, packets.ctypes.data, pb.ctypes.data, rates.ctypes.data,
                                                            pcm16.ctypes.data, ext.ctypes.data, ext.size, p_off,
                                                            is_noise.ctypes.data, is_cn.ctypes.data))
        return pcm16, ext, is_noise, is_cn

    def decode_spans_packed(self, spans, packets, num_bits, sample_rates, n_ext_samples=None, lane_ids=(), ext_offsets=None):
        """decode_spans_packed_dev from host arrays: packets uint8 [frames][bytes of num_bits].  Returns (pcm16 int16
        [frames][320], pcm_ext int16 [n_ext_samples])."""
        packets = _np(packets, np.uint8, (-1, packet_size(num_bits)))
        F = packets.shape[0]
        a, _held = self._span_args(spans, lane_ids, F)
        rates = self._span_rates(sample_rates, a[1])
        p_off, _off = self._span_offsets(ext_offsets, a[1])
        if n_ext_samples is None:
            n_ext_samples = spans_packed_layout(_held[0], rates, self.L)[1]
        pcm16, ext = np.zeros((F, HOP), np.int16), np.zeros(int(n_ext_samples), np.int16)
        self._chk(self.L.lyra_hip_decode_spans_packed(self.h, *a, packets.ctypes.data, num_bits, rates.ctypes.data,
                                                      pcm16.ctypes.data, ext.ctypes.data, ext.size, p_off))
        return pcm16, ext

    # -- a recording through the bridge, time-parallel (include/lyra_hip_bridge_spans.h) ------------------------------------------
    bridge_spans_plan = staticmethod(bridge_spans_plan)

    def _bridge_spans_frames(self, spans, rooms, lane_ids, frames):
        """the host arguments of the three calls below on buffers of `frames` frames, and the arrays they point into"""
        sp, labels = _bridge_spans_args(spans, rooms)
        a, held = self._span_args(sp, lane_ids, frames)
        return a, labels, (held, labels)

    def bridge_spans_mix_dev(self, spans, rooms, d_pcm16, d_mix, max_speakers=0, d_muted=None, d_is_comfort_noise=None,
                             d_levels=None, d_is_speaker=None):
        """The bridge's mix as one pass over all ticks (lyra_hip_spans_bridge_mix_dev): participant p's tick t is frame
        spans[p].first_frame + t of d_pcm16 / d_mix int16 [frames][320]; rooms int32 [P] host labels.  max_speakers 0: the full
        mix of bridge_mix_dev per tick; 1 .. SPEAKERS_MAX: the selection of speakers_mix_dev with d_levels int64 [frames] /
        d_is_speaker int32 [frames] (optional).  d_muted / d_is_comfort_noise int32 [frames] or None.  Frames outside the spans
        are untouched.  Completes on the encode-side stream."""
        F = d_pcm16.shape[0]
        a, labels, _held = self._bridge_spans_frames(spans, rooms, (), F)
        self._dev_call(self.L.lyra_hip_spans_bridge_mix_dev, a[0], a[1], labels.ctypes.data, self._p_pcm(d_pcm16, F),
                       self._opt_dev_ptr(d_muted, "int32", (F,), "muted"),
                       self._opt_dev_ptr(d_is_comfort_noise, "int32", (F,), "is_comfort_noise"), int(max_speakers),
                       self._p_pcm(d_mix, F), self._opt_dev_ptr(d_levels, "int64", (F,), "levels"),
                       self._opt_dev_ptr(d_is_speaker, "int32", (F,), "is_speaker"))

    def bridge_spans_dev(self, spans, rooms, d_packets, packet_bytes, num_bits, d_out_packets, d_out_packet_bytes, d_pcm16,
                         d_mix, lane_ids=(), d_muted=None, dtx=None, flags=0, max_speakers=0, d_is_noise=None,
                         d_is_comfort_noise=None, d_levels=None, d_is_speaker=None):
        """A meeting recording through the bridge in one call (lyra_hip_spans_bridge_dev): bit for bit bridge_tick_dev
        (max_speakers 0) or speakers_tick_dev over the T ticks of the spans.  spans, rooms [P], lane_ids, packet_bytes int32
        [frames] (0 / 8 / 15 / 23), num_bits int32 [frames] and dtx [P] or None stay host arrays; d_packets / d_out_packets uint8
        [frames][23], d_out_packet_bytes int32 [frames], d_pcm16 / d_mix int16 [frames][320] (required workspace and output),
        d_muted int32 [frames] or None; d_is_noise / d_is_comfort_noise / d_is_speaker int32 [frames], d_levels int64 [frames]:
        optional outputs.  Blocks the host once at its start, and once more where dtx names a participant; with DTX the
        context's encoder rate must be 16000."""
        F = d_packets.shape[0]
        a, labels, _held = self._bridge_spans_frames(spans, rooms, lane_ids, F)
        pb = self._span_packet_bytes(packet_bytes, F)
        bits = self._span_packet_bytes(num_bits, F, "num_bits")
        d = None if dtx is None else _np(np.asarray(dtx) != 0, np.int32, (a[1],))
        call = BridgeSpansCall(a[0], a[1], a[2], a[3], labels.ctypes.data, self._p_packets(d_packets, F, MAX_PACKET_BYTES),
                               pb.ctypes.data, self._opt_dev_ptr(d_muted, "int32", (F,), "muted"), int(flags), bits.ctypes.data,
                               None if d is None else d.ctypes.data, self._p_packets(d_out_packets, F, MAX_PACKET_BYTES),
                               self._p_packet_bytes(d_out_packet_bytes, F), self._p_pcm(d_pcm16, F), self._p_pcm(d_mix, F),
                               *self._p_noise_flags(d_is_noise, d_is_comfort_noise, F), int(max_speakers),
                               self._opt_dev_ptr(d_levels, "int64", (F,), "levels"),
                               self._opt_dev_ptr(d_is_speaker, "int32", (F,), "is_speaker"))
        self._dev_call(self.L.lyra_hip_spans_bridge_dev, C.addressof(call))

    def bridge_spans(self, spans, rooms, packets, packet_bytes, num_bits, lane_ids=(), muted=None, dtx=None, flags=0,
                     max_speakers=0):
        """bridge_spans_dev from host arrays (lyra_hip_spans_bridge): packets uint8 [frames][23], packet_bytes / num_bits int32
        [frames], muted [frames] or None, dtx [P] or None.  Returns a dict of frame-indexed arrays: out_packets uint8
        [frames][23] (zero behind each packet's bytes), out_packet_bytes, is_noise, is_comfort_noise int32 [frames], pcm16 and
        mix int16 [frames][320], and with max_speakers >= 1 levels int64 [frames] and is_speaker int32 [frames]; rows outside
        every span are 0."""
        packets = _np(packets, np.uint8, (-1, MAX_PACKET_BYTES))
        F = packets.shape[0]
        a, labels, _held = self._bridge_spans_frames(spans, rooms, lane_ids, F)
        pb = self._span_packet_bytes(packet_bytes, F)
        bits = self._span_packet_bytes(num_bits, F, "num_bits")
        m = None if muted is None else self._span_packet_bytes(np.asarray(muted) != 0, F, "muted")
        d = None if dtx is None else _np(np.asarray(dtx) != 0, np.int32, (a[1],))
        out = {"out_packets": np.zeros((F, MAX_PACKET_BYTES), np.uint8), "out_packet_bytes": np.zeros(F, np.int32),
               "pcm16": np.zeros((F, HOP), np.int16), "mix": np.zeros((F, HOP), np.int16),
               "is_noise": np.zeros(F, np.int32), "is_comfort_noise": np.zeros(F, np.int32)}
        if max_speakers:
            out["levels"], out["is_speaker"] = np.zeros(F, np.int64), np.zeros(F, np.int32)
        sel = [out[k].ctypes.data if k in out else None for k in ("levels", "is_speaker")]
        self._chk(self.L.lyra_hip_spans_bridge(self.h, *a, labels.ctypes.data, packets.ctypes.data, pb.ctypes.data,
                                               None if m is None else m.ctypes.data, int(flags), bits.ctypes.data,
                                               None if d is None else d.ctypes.data, int(max_speakers),
                                               out["out_packets"].ctypes.data, out["out_packet_bytes"].ctypes.data,
                                               out["pcm16"].ctypes.data, out["mix"].ctypes.data, out["is_noise"].ctypes.data,
                                               out["is_comfort_noise"].ctypes.data, *sel))
        return out

    # -- a meeting with a schedule, time-parallel (include/lyra_hip_spans_meeting.h) ----------------------------------------------
    meeting_plan = staticmethod(meeting_plan)

    def _meeting_frames(self, spans, stays, lane_ids, frames):
        """the host arguments of the three calls below on buffers of `frames` frames, and the arrays they point into"""
        sp, st = _meeting_args(spans, stays)
        a, held = self._span_args(sp, lane_ids, frames)
        return a, (st.ctypes.data if st.size else None, st.size), (held, st)

    def meeting_spans_mix_dev(self, spans, stays, d_pcm16, d_mix, max_speakers=0, d_muted=None, d_is_comfort_noise=None,
                              d_levels=None, d_is_speaker=None):
        """The bridge's mix over a meeting with a schedule as one pass (lyra_hip_spans_meeting_mix_dev): participant p's k-th
        present tick is frame spans[p].first_frame + k of d_pcm16 / d_mix int16 [frames][320]; stays (participant, room,
        first_tick, n_ticks) say who is present where.  max_speakers, d_muted, d_is_comfort_noise, d_levels and d_is_speaker as
        bridge_spans_mix_dev.  Frames outside the spans are untouched.  Completes on the encode-side stream."""
        F = d_pcm16.shape[0]
        a, s, _held = self._meeting_frames(spans, stays, (), F)
        self._dev_call(self.L.lyra_hip_spans_meeting_mix_dev, a[0], a[1], s[0], s[1], self._p_pcm(d_pcm16, F),
                       self._opt_dev_ptr(d_muted, "int32", (F,), "muted"),
                       self._opt_dev_ptr(d_is_comfort_noise, "int32", (F,), "is_comfort_noise"), int(max_speakers),
                       self._p_pcm(d_mix, F), self._opt_dev_ptr(d_levels, "int64", (F,), "levels"),
                       self._opt_dev_ptr(d_is_speaker, "int32", (F,), "is_speaker"))

    def meeting_spans_dev(self, spans, stays, d_packets, packet_bytes, num_bits, d_out_packets, d_out_packet_bytes, d_pcm16,
                          d_mix, lane_ids=(), d_muted=None, dtx=None, flags=0, max_speakers=0, d_is_noise=None,
                          d_is_comfort_noise=None, d_levels=None, d_is_speaker=None):
        """A recorded meeting whose participants join, leave and move rooms, through the bridge in one call
        (lyra_hip_spans_meeting_dev): bit for bit bridge_tick_dev (max_speakers 0) or speakers_tick_dev over the meeting's ticks
        with the present participants as rows.  spans [P] (n_frames = present ticks), stays, lane_ids, packet_bytes / num_bits
        int32 [frames] and dtx [P] or None stay host arrays; the device buffers are those of bridge_spans_dev."""
        F = d_packets.shape[0]
        a, s, _held = self._meeting_frames(spans, stays, lane_ids, F)
        pb = self._span_packet_bytes(packet_bytes, F)
        bits = self._span_packet_bytes(num_bits, F, "num_bits")
        d = None if dtx is None else _np(np.asarray(dtx) != 0, np.int32, (a[1],))
        call = MeetingSpansCall(a[0], a[1], a[2], a[3], s[0], s[1], self._p_packets(d_packets, F, MAX_PACKET_BYTES),
                                pb.ctypes.data, self._opt_dev_ptr(d_muted, "int32", (F,), "muted"), int(flags), bits.ctypes.data,
                                None if d is None else d.ctypes.data, self._p_packets(d_out_packets, F, MAX_PACKET_BYTES),
                                self._p_packet_bytes(d_out_packet_bytes, F), self._p_pcm(d_pcm16, F), self._p_pcm(d_mix, F),
                                *self._p_noise_flags(d_is_noise, d_is_comfort_noise, F), int(max_speakers),
                                self._opt_dev_ptr(d_levels, "int64", (F,), "levels"),
                                self._opt_dev_ptr(d_is_speaker, "int32", (F,), "is_speaker"))
        self._dev_call(self.L.lyra_hip_spans_meeting_dev, C.addressof(call))

    def meeting_spans(self, spans, stays, packets, packet_bytes, num_bits, lane_ids=(), muted=None, dtx=None, flags=0,
                      max_speakers=0):
        """meeting_spans_dev from host arrays (lyra_hip_spans_meeting); arguments and the returned dict of frame-indexed arrays
        as bridge_spans, with stays in place of rooms; rows outside every span are 0."""
        packets = _np(packets, np.uint8, (-1, MAX_PACKET_BYTES))
        F = packets.shape[0]
        a, s, _held = self._meeting_frames(spans, stays, lane_ids, F)
        pb = self._span_packet_bytes(packet_bytes, F)
        bits = self._span_packet_bytes(num_bits, F, "num_bits")
        m = None if muted is None else self._span_packet_bytes(np.asarray(muted) != 0, F, "muted")
        d = None if dtx is None else _np(np.asarray(dtx) != 0, np.int32, (a[1],))
        out = {"out_packets": np.zeros((F, MAX_PACKET_BYTES), np.uint8), "out_packet_bytes": np.zeros(F, np.int32),
               "pcm16": np.zeros((F, HOP), np.int16), "mix": np.zeros((F, HOP), np.int16),
               "is_noise": np.zeros(F, np.int32), "is_comfort_noise": np.zeros(F, np.int32)}
        if max_speakers:
            out["levels"], out["is_speaker"] = np.zeros(F, np.int64), np.zeros(F, np.int32)
        sel = [out[k].ctypes.data if k in out else None for k in ("levels", "is_speaker")]
        self._chk(self.L.lyra_hip_spans_meeting(self.h, *a, s[0], s[1], packets.ctypes.data, pb.ctypes.data,
                                                None if m is None else m.ctypes.data, int(flags), bits.ctypes.data,
                                                None if d is None else d.ctypes.data, int(max_speakers),
                                                out["out_packets"].ctypes.data, out["out_packet_bytes"].ctypes.data,
                                                out["pcm16"].ctypes.data, out["mix"].ctypes.data, out["is_noise"].ctypes.data,
                                                out["is_comfort_noise"].ctypes.data, *sel))
        return out

    def noise_receive_dev(self, d_ids, d_pcm, d_is_noise, side="decoder"):
        """NoiseEstimator::ReceiveSamples on device buffers: pcm int16 [B][320] -> is_noise int32 [B]."""
        B = d_pcm.shape[0]
        self._dev_call(self.L.lyra_hip_noise_receive_dev, self._SIDES[side], self._p_ids(d_ids, B), B,
                       self._p_pcm(d_pcm, B), self._dev_ptr(d_is_noise, "int32", (B,), "is_noise"))

    def resample_dev(self, d_ids, d_in, in_rate, out_rate, d_out, side="encoder"):
        """Resampler::Resample per stream on device buffers: int16 [B][n_in] -> int16 [B][n_in * out_rate / in_rate]."""
        B, n_in = d_in.shape
        self._dev_call(self.L.lyra_hip_resample_dev, self._SIDES[side], self._p_ids(d_ids, B), B,
                       self._dev_ptr(d_in, "int16", (B, n_in), "input audio"), n_in, in_rate, out_rate,
                       self._dev_ptr(d_out, "int16", (B, n_in * out_rate // in_rate), "output audio"))

    def comfort_noise_dev(self, d_ids, d_features, d_pcm):
        """ComfortNoiseGenerator on device buffers; d_features float32 [B][160] or None (= decoder-side noise estimate)."""
        B = d_pcm.shape[0]
        self._dev_call(self.L.lyra_hip_comfort_noise_dev, self._p_ids(d_ids, B), B,
                       self._opt_dev_ptr(d_features, "float32", (B, NUM_MEL), "features"), self._p_pcm(d_pcm, B))

    def run_steps_dev(self, d_ids, num_bits, n_steps, first_step=0, d_pcm_ring=None, d_packets=None, d_pcm_out=None,
                      d_features=None, d_packet_bytes=None, d_is_noise=None, external_rate=16000, d_ext_out=None,
                      encode=True, decode=True, dtx=False, decoder_noise=False, d_packet_ring=None,
                      d_received_ring=None, d_is_comfort_noise=None, packet_loss=False, d_bits_ring=None,
                      d_rates=None):
        """lyra_hip_run_steps_dev: n_steps hops of every stream from ONE C call.  d_pcm_ring int16
        [ring][B][320 * external_rate / 16000]; d_packets / d_pcm_out / d_packet_bytes / d_ext_out: pairs of tensors
        (step i uses element (first_step + i) & 1).  packet_loss: the decode leg is decode_lossy_dev; d_received_ring
        uint8 [n][B] (None = all received; step i reads row (first_step + i) % n), with dtx DTX's empty packets are not
        received either.  d_bits_ring int32 [n][B] sets STEP_MIXED_BITRATE: step i encodes (and, decode-only, decodes) at
        the bit counts of row (first_step + i) % n, num_bits must be 0, packet rows are MAX_PACKET_BYTES long.
        d_rates int32 [B] sets STEP_MIXED_RATE (the call then passes a lyra_hip_steps_rates): each stream at its own sample rate (encode_rates_dev /
        decode_lossy_rates_dev); external_rate must be left alone, d_pcm_ring is [ring][B][MAX_EXT_HOP], d_ext_out are
        [B][MAX_EXT_HOP], packet rows are MAX_PACKET_BYTES long."""
        B = d_ids.shape[0]
        nbytes = MAX_PACKET_BYTES if (d_bits_ring is not None or d_rates is not None) else packet_size(num_bits)
        n_ext = HOP * external_rate // 16000
        if d_rates is not None:
            if external_rate not in (0, 16000):   # (16000: this wrapper's "none", as without d_rates)
                raise ValueError("run_steps_dev: d_rates and external_rate=%d exclude each other" % external_rate)
            n_ext, external_rate = MAX_EXT_HOP, 0
        R = StepsDescRates()
        S = R.steps
        S.d_stream_ids = self._p_ids(d_ids, B)
        S.B, S.num_bits, S.first_step, S.n_steps = B, num_bits, first_step, n_steps
        S.flags = (STEP_ENCODE if encode else 0) | (STEP_DECODE if decode else 0) | (STEP_DTX if dtx else 0) | \
            (STEP_DECODER_NOISE if decoder_noise else 0) | (STEP_PACKET_LOSS if packet_loss else 0) | \
            (STEP_MIXED_BITRATE if d_bits_ring is not None else 0) | (STEP_MIXED_RATE if d_rates is not None else 0)
        if d_rates is not None:
            R.d_rates = self._dev_ptr(d_rates, "int32", (B,), "sample rates")
        if d_bits_ring is not None:
            S.n_bits_ring = d_bits_ring.shape[0]
            S.d_bits_ring = self._dev_ptr(d_bits_ring, "int32", (S.n_bits_ring, B), "bits ring")
        S.external_rate = external_rate
        if d_received_ring is not None:
            S.n_received_ring = d_received_ring.shape[0]
            S.d_received_ring = self._dev_ptr(d_received_ring, "uint8", (S.n_received_ring, B), "received ring")
        if d_is_comfort_noise is not None:
            S.d_is_comfort_noise = self._dev_ptr(d_is_comfort_noise, "int32", (B,), "is_comfort_noise")
        if d_pcm_ring is not None:
            S.ring = d_pcm_ring.shape[0]
            S.d_pcm_ring = self._dev_ptr(d_pcm_ring, "int16", (S.ring, B, n_ext), "pcm ring")
        for i in range(2):
            if d_packets is not None:
                S.d_packets[i] = self._p_packets(d_packets[i], B, nbytes)
            if d_pcm_out is not None:
                S.d_pcm_out[i] = self._dev_ptr(d_pcm_out[i], "int16", (B, HOP), "pcm out")
            if d_packet_bytes is not None:
                S.d_packet_bytes[i] = self._p_packet_bytes(d_packet_bytes[i], B)
            if d_ext_out is not None:
                S.d_ext_out[i] = self._dev_ptr(d_ext_out[i], "int16", (B, n_ext), "external-rate out")
        if d_features is not None:     # [B][64], or [n][B][64]: step i generates from frame (first_step + i) % n
            S.n_features = d_features.shape[0] if d_features.dim() == 3 else 1
            S.d_features = self._dev_ptr(d_features, "float32", (S.n_features, B, NUM_FEATURES) if d_features.dim() == 3
                                         else (B, NUM_FEATURES), "features")
        if d_packet_ring is not None:  # decode-only: received packets [n][B][bytes], step i decodes frame (first_step + i) % n
            S.n_packet_ring = d_packet_ring.shape[0]
            S.d_packet_ring = self._dev_ptr(d_packet_ring, "uint8", (S.n_packet_ring, B, nbytes), "packet ring")
        if d_is_noise is not None:
            S.d_is_noise = self._dev_ptr(d_is_noise, "int32", (B,), "is_noise")
        self._dev_call(self.L.lyra_hip_run_steps_dev, C.byref(R.steps))

    def decode_dev(self, d_ids, d_packets, num_bits, d_pcm):
        B = d_pcm.shape[0]
        self._dev_call(self.L.lyra_hip_decode_dev, self._p_ids(d_ids, B), B,
                       self._p_packets(d_packets, B, packet_size(num_bits)), num_bits, self._p_pcm(d_pcm, B))

    def extract_dev(self, d_ids, d_pcm, d_feat):
        B = d_pcm.shape[0]
        self._dev_call(self.L.lyra_hip_extract_dev, self._p_ids(d_ids, B), B, self._p_pcm(d_pcm, B),
                       self._dev_ptr(d_feat, "float32", (B, NUM_FEATURES), "features"))

    def generate_dev(self, d_ids, d_feat, d_pcm):
        B = d_feat.shape[0]
        self._dev_call(self.L.lyra_hip_generate_dev, self._p_ids(d_ids, B), B,
                       self._dev_ptr(d_feat, "float32", (B, NUM_FEATURES), "features"), self._p_pcm(d_pcm, B))

    def logmel_dev(self, d_ids, d_pcm, d_mel):
        B = d_pcm.shape[0]
        self._dev_call(self.L.lyra_hip_logmel_dev, self._p_ids(d_ids, B), B, self._p_pcm(d_pcm, B),
                       self._dev_ptr(d_mel, "float32", (B, NUM_MEL), "mel"))

    def rvq_encode_dev(self, d_feat, num_bits, d_idx):
        B = d_feat.shape[0]
        self._dev_call(self.L.lyra_hip_rvq_encode_dev, B, self._dev_ptr(d_feat, "float32", (B, NUM_FEATURES), "features"),
                       num_bits, self._dev_ptr(d_idx, "int32", (B, 46), "indices"))

    def rvq_decode_dev(self, d_idx, d_feat):
        B = d_idx.shape[0]
        self._dev_call(self.L.lyra_hip_rvq_decode_dev, B, self._dev_ptr(d_idx, "int32", (B, 46), "indices"),
                       self._dev_ptr(d_feat, "float32", (B, NUM_FEATURES), "features"))


# ---------------------------------------------------------------------------------------------------
# single-stream plugin objects with the reference's method names and error behaviour
# ---------------------------------------------------------------------------------------------------
class _Plugin:
    def __init__(self, ctx, stream_id=0):
        self.ctx = ctx
        self.sid = np.array([stream_id], np.int32)


class SoundStreamEncoder(_Plugin):
    """FeatureExtractorInterface (lyra/soundstream_encoder.h)."""

    def Extract(self, audio):
        audio = np.asarray(audio)
        if audio.size != HOP:
            return None
        return self.ctx.extract(audio.astype(np.int16), self.sid)[0]


class ResidualVectorQuantizer(_Plugin):
    """VectorQuantizerInterface (lyra/residual_vector_quantizer.h): bit strings of '0'/'1', first
    quantizer in the most significant position."""

    def Quantize(self, features, num_bits):
        if num_bits > MAX_BITS or num_bits % 4 != 0 or num_bits < 0:
            return None  # residual_vector_quantizer.cc:79-89
        if num_bits == 0:
            return ""
        idx = self.ctx.rvq_encode(np.asarray(features, np.float32).reshape(1, 64), num_bits)[0]
        return "".join(format(int(i), "04b") for i in idx[:num_bits // 4])

    def DecodeToLossyFeatures(self, quantized_features):
        n = len(quantized_features)
        if n > MAX_BITS or n % 4 != 0:
            return None  # residual_vector_quantizer.cc:116-126
        idx = np.full(46, -1, np.int32)
        for i in range(n // 4):
            idx[i] = int(quantized_features[4 * i:4 * i + 4], 2)
        return self.ctx.rvq_decode(idx.reshape(1, 46))[0]


class LyraGanModel(_Plugin):
    """GenerativeModel FIFO semantics (lyra/generative_model_interface.h:45-134)."""

    def __init__(self, ctx, stream_id=0):
        super().__init__(ctx, stream_id)
        self._queue = []
        self._next = 0
        self._hop = None

    def AddFeatures(self, features):
        features = np.asarray(features, np.float32)
        if features.size != NUM_FEATURES:
            return False
        self._queue.append(features.copy())
        return True

    def num_samples_available(self):
        return len(self._queue) * HOP - self._next

    def GenerateSamples(self, num_samples):
        if num_samples < 0:
            return None
        if num_samples == 0:
            return np.zeros(0, np.int16)
        if self.num_samples_available() == 0:
            return None
        if self._next == 0:
            self._hop = self.ctx.generate(self._queue[0].reshape(1, 64), self.sid)[0]  # RunConditioning
        if num_samples > HOP - self._next:
            return None
        out = self._hop[self._next:self._next + num_samples].copy()  # RunModel
        self._next += num_samples
        if self._next == HOP:
            self._next = 0
            self._queue.pop(0)
        return out


class LogMelSpectrogramExtractor(_Plugin):
    """FeatureExtractorInterface (lyra/log_mel_spectrogram_extractor_impl.h), NoiseEstimator instantiation."""

    def Extract(self, audio):
        audio = np.asarray(audio)
        if audio.size != HOP:
            return None
        return self.ctx.logmel(audio.astype(np.int16), self.sid)[0]
