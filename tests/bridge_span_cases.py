"""A meeting recording through the bridge as the GPU tests hold the device to it (include/lyra_hip_bridge_spans.h): the layout
of P participants' spans in frame-major buffers with filler frames, a recording's per-frame inputs, the twin that runs the same
ticks one by one through bridge_tick_dev / speakers_tick_dev, the one call on prefilled buffers, and the comparison frame by
frame.  No tests here; torch and lyra_amd are imported inside the functions."""
import numpy as np

from bridge_models import np_bridge_plan
from gpu_plumbing import FILL, _dev, _filled, _t
from receiver_models import _full_batch_mask
from row_cases import _draw_bits

ROW = 23
SIZES = np.array([8, 15, 23], np.int32)
OUTPUTS = ("out_packet_bytes", "out_packets", "pcm16", "mix", "is_noise", "is_comfort_noise", "levels", "is_speaker")
WIDTH = {"out_packet_bytes": (1, np.int32), "out_packets": (ROW, np.uint8), "pcm16": (320, np.int16), "mix": (320, np.int16),
         "is_noise": (1, np.int32), "is_comfort_noise": (1, np.int32), "levels": (1, np.int64), "is_speaker": (1, np.int32)}


def recording_layout(ids, T, gaps=(0, 1, 3), tail=2, at=0):
    """participant p's T frames behind gaps[p % len(gaps)] filler frames, `tail` filler frames behind the last, the first
    participant's gap from frame `at` -> (spans [(id, first_frame, T)], frames of the buffer)"""
    spans = []
    for p, i in enumerate(ids):
        at += gaps[p % len(gaps)]
        spans.append((int(i), at, T))
        at += T
    return spans, at + tail


def frames_of(spans, t):
    """the buffer frames of tick t, in span order"""
    return np.array([first + t for (_, first, _) in spans], np.int64)


def by_frame(spans, F, per_tick, dtype):
    """[T][P][...] values of the participants' ticks -> [F][...] by frame, FILL bytes in the frames outside the spans"""
    per_tick = np.asarray(per_tick)
    shape = (F,) + per_tick.shape[2:]
    out = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype).reshape(shape).copy()
    for p, (_, first, n) in enumerate(spans):
        out[first:first + n] = per_tick[:n, p]
    return out


def draw_recording(rng, P, T, outage=None, mute_rate=0.15):
    """the per-tick inputs of a recording, [T][P] each: packets [T][P][23] random bytes, sizes from {8, 15, 23} under a bursty
    loss mask (outage = (participant, first tick, ticks): that stretch lost as well, 14 ticks reach comfort noise), outgoing
    bit counts, mutes that change from tick to tick"""
    mask = _full_batch_mask(T, P, rng).astype(bool)
    if outage is not None:
        p, t0, n = outage
        mask[:, p] = True
        mask[t0:t0 + n, p] = False
    packets = rng.integers(0, 256, (T, P, ROW), dtype=np.uint8)
    sizes = np.where(mask, rng.choice(SIZES, (T, P)), 0).astype(np.int32)
    bits = np.stack([_draw_bits(rng, P) for _ in range(T)]).astype(np.int32)
    muted = (rng.random((T, P)) < mute_rate).astype(np.int32)
    return dict(packets=packets, sizes=sizes, bits=bits, muted=muted)


class FilledBufs:
    """one device buffer per output, `rows` rows each (the P rows of a tick on the twin, the F frames of the one call), every
    byte FILL"""

    def __init__(self, rows):
        self.rows = rows
        self.t = {k: _filled(_dev(), rows, w, dt) for k, (w, dt) in WIDTH.items()}

    def refill(self):
        for v in self.t.values():
            v.view(_u8()).fill_(FILL)

    def flat(self, k):
        return self.t[k] if WIDTH[k][0] > 1 else self.t[k].view(-1)

    def read(self):
        return {k: self.flat(k).cpu().numpy().copy() for k in OUTPUTS}


def _u8():
    import torch
    return torch.uint8


def twin_ticks(u, ids, rooms, rec, dtx, flags, max_speakers, t0=0, t1=None, bufs=None):
    """ticks t0 .. t1 - 1 of the recording on the twin, one bridge_tick_dev (max_speakers 0) or speakers_tick_dev call each,
    rows in span order -> {output: [ticks][P][...]}; levels and is_speaker stay FILL for the full mix"""
    P = len(ids)
    t1 = rec["sizes"].shape[0] if t1 is None else t1
    order, start = np_bridge_plan(rooms)
    d_order, d_start, d_ids, d_dtx = _t(order), _t(start), _t(np.asarray(ids, np.int32)), _t(np.asarray(dtx, np.int32))
    bufs = bufs or [FilledBufs(P), FilledBufs(P)]
    out = {k: [] for k in OUTPUTS}
    for t in range(t0, t1):
        b = bufs[t & 1]
        b.refill()
        args = (d_ids, _t(rec["packets"][t]), _t(rec["sizes"][t]), d_order, d_start, _t(rec["bits"][t]), b.t["out_packets"],
                b.flat("out_packet_bytes"))
        kw = dict(d_muted=_t(rec["muted"][t]), d_dtx=d_dtx, flags=flags, d_pcm16=b.t["pcm16"], d_mix=b.t["mix"],
                  d_is_noise=b.flat("is_noise"), d_is_comfort_noise=b.flat("is_comfort_noise"))
        if max_speakers:
            u.speakers_tick_dev(*args, max_speakers, d_levels=b.flat("levels"), d_is_speaker=b.flat("is_speaker"), **kw)
        else:
            u.bridge_tick_dev(*args, **kw)
        u.synchronize()
        for k, v in b.read().items():
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


def span_call(a, spans, F, rooms, rec, dtx, flags, max_speakers, lanes, t0=0, t1=None, bufs=None, noise_flags=True):
    """ticks t0 .. t1 - 1 of the recording through bridge_spans_dev, in one call on FILL-prefilled buffers of F frames: the spans
    are `spans` cut to those ticks (tick t0 at each span's first frame) -> ({output: [F][...]}, the spans of the call);
    noise_flags=False: the call is given neither d_is_noise nor d_is_comfort_noise"""
    t1 = rec["sizes"].shape[0] if t1 is None else t1
    n = t1 - t0
    part = [(i, first, n) for (i, first, _) in spans]
    sl = slice(t0, t1)
    bufs = bufs or FilledBufs(F)
    d_pk = _t(by_frame(part, F, rec["packets"][sl], np.uint8))
    d_muted = _t(by_frame(part, F, rec["muted"][sl], np.int32))
    sel = dict(d_levels=bufs.flat("levels"), d_is_speaker=bufs.flat("is_speaker")) if max_speakers else {}
    a.bridge_spans_dev(part, rooms, d_pk, by_frame(part, F, rec["sizes"][sl], np.int32), by_frame(part, F, rec["bits"][sl], np.int32),
                       bufs.t["out_packets"], bufs.flat("out_packet_bytes"), bufs.t["pcm16"], bufs.t["mix"], lane_ids=lanes,
                       d_muted=d_muted, dtx=dtx, flags=flags, max_speakers=max_speakers,
                       d_is_noise=bufs.flat("is_noise") if noise_flags else None,
                       d_is_comfort_noise=bufs.flat("is_comfort_noise") if noise_flags else None, **sel)
    a.synchronize()
    return bufs.read(), part


def check_frames(where, got, want, spans, selection):
    """every span frame of every output equals the twin's tick (the twin's buffers were FILL before each tick, so bytes behind
    a packet and the rows of empty DTX packets must still hold FILL here too); every frame outside the spans holds FILL"""
    for k in OUTPUTS:
        g = got[k].reshape(len(got[k]), -1)
        covered = np.zeros(len(g), bool)
        for p, (i, first, n) in enumerate(spans):
            covered[first:first + n] = True
            if k in ("levels", "is_speaker") and not selection:
                assert (g[first:first + n].view(np.uint8) == FILL).all(), f"{where}: {k} written by the full mix (stream {i})"
                continue
            w = want[k][:n, p].reshape(n, -1)
            bad = np.flatnonzero((g[first:first + n] != w).any(axis=1))
            assert bad.size == 0, f"{where}: {k} of stream {i} differs at ticks {bad[:8].tolist()} ({bad.size} of {n})"
        assert (g[~covered].view(np.uint8) == FILL).all(), f"{where}: {k}: frames outside every span were written"
