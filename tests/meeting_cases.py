"""A meeting with a schedule as the tests hold the library to it (include/lyra_hip_spans_meeting.h): the planner restated in
numpy, drawn schedules, the layout of the participants' present ticks in frame-major buffers, the twin that runs the meeting's
ticks one by one through bridge_tick_dev / speakers_tick_dev with the present participants as rows, the one call on prefilled
buffers, and the comparison frame by frame.  No tests here; torch and lyra_amd are imported inside the functions."""
import numpy as np

from bridge_models import np_bridge_plan
from bridge_span_cases import OUTPUTS, WIDTH, FilledBufs
from gpu_plumbing import FILL, _t


def as_stays(stays):
    """[(participant, room, first_tick, n_ticks)] sorted by (participant, first_tick), as plain ints"""
    return sorted(((int(p), int(r), int(t), int(n)) for (p, r, t, n) in stays), key=lambda s: (s[0], s[2]))


def schedule_tables(P, stays):
    """-> (present bool [T][P], room int32 [T][P] (labels; meaningless where absent), T)"""
    T = max([t + n for (_, _, t, n) in stays], default=0)
    present, room = np.zeros((T, P), bool), np.full((T, P), -1, np.int32)
    for (p, r, t, n) in stays:
        assert not present[t:t + n, p].any(), "overlapping stays"
        present[t:t + n, p] = True
        room[t:t + n, p] = r
    return present, room, T


def np_meeting_plan(spans, stays):
    """lyra_hip_spans_meeting_plan restated: -> dict(n_ticks, epoch_tick [E + 1], epoch_entry [E + 1], entry_participant,
    entry_room).  Boundaries are the distinct values of {first_tick, first_tick + n_ticks}; inside an epoch rooms come in
    ascending label order under dense numbers, participants ascending inside a room, then the participants in no room (-1)."""
    P = len(spans)
    present, room, T = schedule_tables(P, stays)
    bounds = sorted({t for (_, _, t, n) in stays} | {t + n for (_, _, t, n) in stays})
    epoch_tick = np.array(bounds if bounds else [0], np.int64)
    epoch_entry, part, dense = [0], [], []
    for t0 in bounds[:-1]:
        here = np.flatnonzero(present[t0])
        labels = room[t0, here]
        inside = here[labels >= 0]
        inside = inside[np.argsort(room[t0, inside], kind="stable")]
        names = {label: i for i, label in enumerate(sorted(set(room[t0, inside].tolist())))}
        part += inside.tolist() + here[labels < 0].tolist()
        dense += [names[int(room[t0, p])] for p in inside] + [-1] * int((labels < 0).sum())
        epoch_entry.append(len(part))
    return dict(n_ticks=T, epoch_tick=epoch_tick, epoch_entry=np.array(epoch_entry, np.int64),
                entry_participant=np.array(part, np.int32), entry_room=np.array(dense, np.int32))


def draw_schedule(rng, P, T, n_rooms=3, events=12, no_room=0.1):
    """a schedule of `events` membership events over T ticks: everyone starts present in a room (or, now and then, in none);
    an event makes one participant leave, rejoin (where it was absent) or move rooms at a drawn tick.  One participant never
    shows up at all -> stays sorted by (participant, first_tick)"""
    def label():
        return -1 - int(rng.integers(0, 3)) if rng.random() < no_room else int(rng.integers(0, n_rooms)) * 7 + 2
    room = np.zeros((T, P), np.int64)
    present = np.ones((T, P), bool)
    for p in range(P):
        room[:, p] = label()
    for _ in range(events):
        p, t = int(rng.integers(0, P)), int(rng.integers(1, max(T, 2)))
        if t >= T:
            continue
        if not present[t, p]:
            present[t:, p] = True
            room[t:, p] = label()
        elif rng.random() < 0.5:
            present[t:, p] = False
        else:
            room[t:, p] = label()
    if P > 2:
        present[:, int(rng.integers(0, P))] = False
    stays = []
    for p in range(P):
        t = 0
        while t < T:
            if not present[t, p]:
                t += 1
                continue
            e = t
            while e < T and present[e, p] and room[e, p] == room[t, p]:
                e += 1
            stays.append((p, int(room[t, p]), t, e - t))
            t = e
    return as_stays(stays)


def present_ticks(stays, p):
    """the meeting ticks on which participant p is present, ascending"""
    ticks = [np.arange(t, t + n) for (q, _, t, n) in stays if q == p]
    return np.concatenate(ticks) if ticks else np.zeros(0, np.int64)


def meeting_layout(ids, stays, gaps=(0, 1, 3), tail=2, at=0):
    """participant p's present ticks behind gaps[p % len(gaps)] filler frames, `tail` filler frames behind the last
    -> (spans [(id, first_frame, present ticks)], frames of the buffer)"""
    spans = []
    for p, i in enumerate(ids):
        n = len(present_ticks(stays, p))
        at += gaps[p % len(gaps)]
        spans.append((int(i), at, n))
        at += n
    return spans, at + tail


def frames_of_tick(spans, stays, t):
    """-> (participants present on meeting tick t ascending, their buffer frames, their room labels)"""
    rows, frames, rooms = [], [], []
    for p, (_, first, _) in enumerate(spans):
        k = 0
        for (q, r, t0, n) in stays:
            if q != p:
                continue
            if t0 <= t < t0 + n:
                rows.append(p)
                frames.append(first + k + t - t0)
                rooms.append(r)
            k += n
    return np.array(rows, np.int64), np.array(frames, np.int64), np.array(rooms, np.int32)


def by_present_frame(spans, stays, F, per_tick, dtype):
    """[T][P][...] values of the meeting's ticks -> [F][...] by frame: participant p's k-th present tick at first_frame + k,
    FILL bytes in the frames outside the spans"""
    per_tick = np.asarray(per_tick)
    shape = (F,) + per_tick.shape[2:]
    out = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype).reshape(shape).copy()
    for p, (_, first, n) in enumerate(spans):
        ticks = present_ticks(stays, p)
        assert len(ticks) == n
        out[first:first + n] = per_tick[ticks, p]
    return out


def drawn_ids_and_lanes(seed, max_streams, n_ids, n_lanes):
    """distinct stream ids of a context of max_streams, drawn: the participants' and the lanes'"""
    perm = np.random.default_rng(seed).permutation(max_streams).astype(np.int32)
    return perm[:n_ids], perm[n_ids:n_ids + n_lanes]


def assert_warmup_chunks_on_both_sides(spans, lanes, max_streams):
    """the legs' plans over spans of different lengths lend lanes: a chunk with warm-up on the decode and on the encode side"""
    import lyra_amd.codec as codec
    live = [s for s in spans if s[2]]
    for side in ("decoder", "encoder"):
        chunks, _ = codec.spans_plan(side, live, lanes, max_streams)
        assert (chunks["n_warmup"] > 0).any(), f"{side}: the plan uses no lane chunk with warm-up"


def filled_frames(F):
    """{output: [F][...]} with every byte FILL"""
    return {k: np.full(F * w * np.dtype(dt).itemsize, FILL, np.uint8).view(dt).reshape((F, w) if w > 1 else (F,)).copy()
            for k, (w, dt) in WIDTH.items()}


def twin_meeting_ticks(u, ids, spans, stays, rec, dtx, flags, max_speakers, F, t0=0, t1=None, tick_of=lambda t: t, want=None):
    """meeting ticks t0 .. t1 - 1 on the twin, one bridge_tick_dev (max_speakers 0) or speakers_tick_dev call each with the
    participants present on that tick as rows in ascending participant number (a tick with nobody present is no call);
    rec is [ticks][P], read at tick_of(t).  -> {output: [F][...]} by frame, FILL where no tick wrote (bytes behind a packet and
    the rows of empty DTX packets included: the twin's buffers are FILL before each tick)"""
    ids, dtx = np.asarray(ids, np.int32), np.asarray(dtx, np.int32)
    T = max([t + n for (_, _, t, n) in stays], default=0)
    t1 = T if t1 is None else t1
    want = want or filled_frames(F)
    bufs = [FilledBufs(len(ids)), FilledBufs(len(ids))]
    for t in range(t0, t1):
        rows, frames, rooms = frames_of_tick(spans, stays, t)
        B = len(rows)
        if not B:
            continue
        order, start = np_bridge_plan(rooms)
        b = bufs[t & 1]
        b.refill()
        r = tick_of(t)
        args = (_t(ids[rows]), _t(rec["packets"][r][rows]), _t(rec["sizes"][r][rows]), _t(order), _t(start), _t(rec["bits"][r][rows]),
                b.t["out_packets"][:B], b.flat("out_packet_bytes")[:B])
        kw = dict(d_muted=_t(rec["muted"][r][rows]), d_dtx=_t(dtx[rows]), flags=flags, d_pcm16=b.t["pcm16"][:B], d_mix=b.t["mix"][:B],
                  d_is_noise=b.flat("is_noise")[:B], d_is_comfort_noise=b.flat("is_comfort_noise")[:B])
        if max_speakers:
            u.speakers_tick_dev(*args, max_speakers, d_levels=b.flat("levels")[:B], d_is_speaker=b.flat("is_speaker")[:B], **kw)
        else:
            u.bridge_tick_dev(*args, **kw)
        u.synchronize()
        for k, v in b.read().items():
            want[k][frames] = v[:B]
    return want


def meeting_call(a, spans, F, stays, rec, dtx, flags, max_speakers, lanes, tick_of=lambda t: t, noise_flags=True):
    """the meeting through meeting_spans_dev, in one call on FILL-prefilled buffers of F frames -> {output: [F][...]}"""
    T = max([t + n for (_, _, t, n) in stays], default=0)
    pick = np.array([tick_of(t) for t in range(T)], np.int64)
    bufs = FilledBufs(F)
    d_pk = _t(by_present_frame(spans, stays, F, rec["packets"][pick], np.uint8))
    d_muted = _t(by_present_frame(spans, stays, F, rec["muted"][pick], np.int32))
    sel = dict(d_levels=bufs.flat("levels"), d_is_speaker=bufs.flat("is_speaker")) if max_speakers else {}
    a.meeting_spans_dev(spans, stays, d_pk, by_present_frame(spans, stays, F, rec["sizes"][pick], np.int32),
                        by_present_frame(spans, stays, F, rec["bits"][pick], np.int32), bufs.t["out_packets"],
                        bufs.flat("out_packet_bytes"), bufs.t["pcm16"], bufs.t["mix"], lane_ids=lanes, d_muted=d_muted, dtx=dtx,
                        flags=flags, max_speakers=max_speakers, d_is_noise=bufs.flat("is_noise") if noise_flags else None,
                        d_is_comfort_noise=bufs.flat("is_comfort_noise") if noise_flags else None, **sel)
    a.synchronize()
    return bufs.read()


def check_meeting_frames(where, got, want, spans):
    """every frame of every output equals the twin's (FILL where the twin wrote nothing: outside the spans, behind a packet, in
    the rows of empty DTX packets, and levels / speaker flags under the full mix)"""
    for k in OUTPUTS:
        g, w = got[k].reshape(len(got[k]), -1), want[k].reshape(len(want[k]), -1)
        bad = np.flatnonzero((g != w).any(axis=1))
        if bad.size:
            owner = {f: (p, f - first) for p, (_, first, n) in enumerate(spans) for f in range(first, first + n)}
            raise AssertionError(f"{where}: {k} differs at {bad.size} frames, first (participant, present tick): "
                                 f"{[owner.get(int(f), 'outside') for f in bad[:8]]}")
