"""A recorded meeting with a schedule through the bridge in one call (include/lyra_hip_spans_meeting.h): the pass against the
formula, the call against the tick calls on a twin context with the present participants as rows (full mix and loudest-N),
against consecutive recording calls where only rooms change, continuation across calls and ticks, the host form against the
`_dev` form, the refusals, and bridge_demo mode 3.  Helpers: tests/meeting_cases.py.

Shapes.  The pass serves one (room, tick) or one (8 positions, tick) per wavefront, members in chunks of 8, rooms above 64
through parked keys, and every wavefront looks its epoch up in a table: the 330-participant shape of the tick kernels' tests
over 5 ticks in three epochs whose boundaries take rooms across 8 and 64 members.  The legs need lane chunks with warm-up (25
hops on both sides): 120 meeting ticks on 24 lanes."""
import os
import subprocess

import numpy as np
import pytest

from bridge_models import SKIP_CN, np_bridge_mix, np_bridge_plan
from bridge_span_cases import WIDTH, ROW, draw_recording, span_call
from gpu_plumbing import FILL, _dev, _filled, _t, make_ctx as _ctx
from meeting_cases import (as_stays, assert_warmup_chunks_on_both_sides, by_present_frame, check_meeting_frames, drawn_ids_and_lanes,
                           filled_frames, frames_of_tick, meeting_call, meeting_layout, twin_meeting_ticks)
from span_cases import _check_state
from speaker_models import _source, np_levels, np_speakers_mix, speakers_kernel_case, tie_decided

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
EINVAL = -1
FILL16 = 21845


# ---- 1. the pass against the formula ---------------------------------------------------------------------------------------

PASS_T = 5


def _pass_case():
    """speakers_kernel_case() over 5 ticks in three epochs of 2, 1 and 2 ticks -> (xs, muted, cns: [T][B] per tick, stays)"""
    x0, rooms, muted0, is_cn0, _, _ = speakers_kernel_case()
    B = x0.shape[0]
    rng = np.random.default_rng(17)
    members = {int(lab): np.flatnonzero(rooms == lab) for lab in set(rooms.tolist()) if lab >= 0}
    assert sorted(len(m) for m in members.values()) == [1, 2, 3, 8, 9, 16, 17, 257]
    lone = np.flatnonzero(rooms < 0)
    stay = {p: [(p, int(rooms[p]), 0, PASS_T)] for p in range(B)}
    # at tick 2 enough members leave that 9 becomes 8, 17 becomes 16 and 257 becomes 64
    for lab, n in ((4, 1), (40, 1), (6, 257 - 64)):
        for p in members[lab][-n:]:
            stay[int(p)] = [(int(p), lab, 0, 2)]
    for p in members[1]:                                   # the 2-room empties at tick 3
        stay[int(p)] = [(int(p), 1, 0, 3)]
    late = int(lone[0])                                    # a late joiner founds a room at tick 2
    stay[late] = [(late, 99, 2, 3)]
    mover = int(members[2][0])                             # from the 3-room into the 8-room at tick 3: 8 becomes 9
    stay[mover] = [(mover, 2, 0, 3), (mover, 3, 3, 2)]
    away = int(members[5][3])                              # absent on the middle tick only: 4 frames, two stays
    stay[away] = [(away, 5, 0, 2), (away, 5, 3, 2)]
    stays = as_stays([s for p in range(B) for s in stay[p]])
    in8 = members[3]
    cn_rows = [int(np.flatnonzero(is_cn0)[0])] + [int(v) for v in in8[1:PASS_T]]
    xs = [np.roll(x0, 5 * t, axis=1) if t else x0 for t in range(PASS_T)]
    muted, cns = [muted0.copy() for _ in range(PASS_T)], []
    for t in range(PASS_T):
        if t:
            muted[t][rng.choice(B, 12, replace=False)] ^= 1
        cn = np.zeros(B, np.int32)
        cn[cn_rows[t]] = 1
        cns.append(cn)
    assert any((muted[t] != muted[0]).any() for t in range(1, PASS_T))
    return np.stack(xs), np.stack(muted), np.stack(cns), stays, dict(late=late, mover=mover, away=away)


def _sizes_on(spans, stays, t):
    _, _, rooms = frames_of_tick(spans, stays, t)
    return sorted(np.diff(np_bridge_plan(rooms)[1]).tolist())


def _run_pass(a, spans, stays, F, xs, muted, cns, N):
    d_x = _t(by_present_frame(spans, stays, F, xs, np.int16))
    d_m = _t(by_present_frame(spans, stays, F, muted, np.int32))
    d_c = _t(by_present_frame(spans, stays, F, cns, np.int32))
    d_mix = _filled(_dev(), F, 320, np.int16)
    d_lv, d_sp = _filled(_dev(), F, 1, np.int64).view(-1), _filled(_dev(), F, 1, np.int32).view(-1)
    a.meeting_spans_mix_dev(spans, stays, d_x, d_mix, N, d_m, d_c, d_lv if N else None, d_sp if N else None)
    a.synchronize()
    return d_mix.cpu().numpy(), d_lv.cpu().numpy(), d_sp.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [0, 1, 3, 8])
def test_pass_equals_the_formula_on_every_present_row(N):
    xs, muted, cns, stays, who = _pass_case()
    B = xs.shape[1]
    spans, F = meeting_layout(np.arange(B), stays)
    assert spans[who["away"]][2] == 4 and spans[who["late"]][2] == 3
    assert _sizes_on(spans, stays, 0) == [1, 2, 3, 8, 9, 16, 17, 257]
    assert _sizes_on(spans, stays, 2) == [1, 1, 2, 3, 8, 8, 15, 16, 64]        # the late joiner's room; 16 - 1 on the middle tick
    assert _sizes_on(spans, stays, 4) == [1, 1, 2, 8, 9, 16, 16, 64]           # the 2-room is gone; 3 - 1 and 8 + 1 by the move
    covered = np.zeros(F, bool)
    for (_, first, n) in spans:
        covered[first:first + n] = True
    assert (~covered).sum() >= 3
    a = _ctx(512)
    try:
        mix, lv, sp = _run_pass(a, spans, stays, F, xs, muted, cns, N)
        sat_hi = sat_lo = False
        seen = np.zeros(F, bool)
        for t in range(PASS_T):
            rows, frames, rooms = frames_of_tick(spans, stays, t)
            seen[frames] = True
            order, start = np_bridge_plan(rooms)
            x, m, c = xs[t][rows], muted[t][rows], cns[t][rows]
            if N:
                want, w_lv, w_sp = np_speakers_mix(x, order, start, N, m, c)
                assert np.array_equal(lv[frames], w_lv), f"tick {t}: levels"
                assert np.array_equal(sp[frames], w_sp), (f"tick {t}: is_speaker differs in rows", rows[sp[frames] != w_sp][:16])
                if N < 5 and t == 0:
                    assert tie_decided(np_levels(x), order, start, _source(len(rows), m, c), N), "no tie is decided by position"
            else:
                want = np_bridge_mix(x, order, start, m, c)
            bad = np.flatnonzero((mix[frames] != want).any(axis=1))
            assert bad.size == 0, (f"tick {t}: rows differ from the formula", rows[bad[:16]], rooms[bad[:16]])
            assert not mix[frames][rooms < 0].any(), f"tick {t}: a participant in no room hears something"
            sat_hi |= bool((want == 32767).any())
            sat_lo |= bool((want == -32768).any())
        assert sat_hi and sat_lo, "the case must saturate on both sides"
        assert np.array_equal(seen, covered), "the ticks name every span frame once"
        assert (mix[~covered] == FILL16).all(), "a frame between or behind the spans was written"
        if N:
            assert (lv[~covered].view(np.uint8) == FILL).all() and (sp[~covered].view(np.uint8) == FILL).all()
        else:
            assert (lv.view(np.uint8) == FILL).all() and (sp.view(np.uint8) == FILL).all(), "written by the full mix"
        assert a.bridge_errors() == 0
    finally:
        a.close()


# ---- 2. the call equals the ticks -------------------------------------------------------------------------------------------

MS, P, T, LANES = 64, 11, 120, 24
ROOMS = np.array([0, 0, 0, 1, 1, 2, 3, 3, 3, 3, -1], np.int32)
DTX = (np.arange(P) % 2).astype(np.int32)


def _ids_and_lanes(seed):
    return drawn_ids_and_lanes(seed, MS, P, LANES)


def _everyone(rooms, n, at=0):
    return as_stays([(p, int(r), at, n) for p, r in enumerate(rooms)])


def _churn_schedule():
    """2 joins at tick 30; 8 leaves at 90; 1 is away for ticks 40 .. 59; 4 moves from room 1 to room 2 at 70; 10 is in no room
    throughout; room 2 is empty on ticks 20 .. 49 (its only member, 5, is away)"""
    stay = {p: [(p, int(ROOMS[p]), 0, T)] for p in range(P)}
    stay[2] = [(2, 0, 30, T - 30)]
    stay[8] = [(8, 3, 0, 90)]
    stay[1] = [(1, 0, 0, 40), (1, 0, 60, T - 60)]
    stay[4] = [(4, 1, 0, 70), (4, 2, 70, T - 70)]
    stay[5] = [(5, 2, 0, 20), (5, 2, 50, T - 50)]
    return as_stays([s for p in range(P) for s in stay[p]])


def _equal_case(serial=False, flags=0, max_speakers=0):
    rng = np.random.default_rng(500 + max_speakers)
    ids, lanes = _ids_and_lanes(3)
    stays = _churn_schedule()
    spans, F = meeting_layout(ids, stays)
    assert [s[2] for s in spans] == [120, 100, 90, 120, 120, 90, 120, 120, 90, 120, 120]
    assert_warmup_chunks_on_both_sides(spans, lanes, MS)
    rec = draw_recording(rng, P, T, outage=(0, 6, 14))          # participant 0 of room 0: 14 ticks lost, into comfort noise
    rec["sizes"][36:64, 1] = 0                                   # participant 1's loss burst spans its gap: it rejoins mid-burst
    rec["sizes"][[35, 64], 1] = 23
    assert set(np.unique(rec["sizes"])) == {0, 8, 15, 23} and (rec["muted"][0] != rec["muted"][1]).any()
    if flags & SKIP_CN:
        rec["muted"][:, :3] = 0
    a, u = _ctx(MS), _ctx(MS)
    try:
        if serial:
            a.set_serial(True)
            u.set_serial(True)
        want = twin_meeting_ticks(u, ids, spans, stays, rec, DTX, flags, max_speakers, F)
        got = meeting_call(a, spans, F, stays, rec, DTX, flags, max_speakers, lanes)
        f0 = spans[0][1]
        assert want["is_comfort_noise"][f0:f0 + T].any(), "the outage never reached comfort noise"
        sizes = [want["out_packet_bytes"][first:first + n] for (_, first, n) in spans]
        assert any((s == 0).any() for s in sizes) and any((s > 0).all() for s in sizes), \
            "the case needs empty DTX packets and streams without any"
        check_meeting_frames("one call", got, want, spans)
        _check_state("after the call", a, u, ids, lanes)
        assert a.decode_lossy_errors() == 0 and a.encode_mixed_errors() == 0 and a.bridge_errors() == 0
        if flags & SKIP_CN:
            changed = 0
            for t in range(T):
                rows, frames, rooms = frames_of_tick(spans, stays, t)
                order, start = np_bridge_plan(rooms)
                plain = np_bridge_mix(want["pcm16"][frames], order, start, rec["muted"][t][rows], None)
                changed += int(not np.array_equal(plain, want["mix"][frames]))
            assert changed >= 1, "SKIP_COMFORT_NOISE never changed a mix row"
        if max_speakers:
            on = np.concatenate([want["is_speaker"][first:first + n] for (_, first, n) in spans])
            assert on.any() and not on.all()
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [0, 2])
def test_call_equals_the_ticks(N):
    _equal_case(max_speakers=N)


@pytest.mark.gpu
def test_call_skips_comfort_noise_rows_when_asked():
    _equal_case(flags=SKIP_CN)


@pytest.mark.gpu
def test_call_equals_the_ticks_in_serial_order():
    _equal_case(serial=True)


# ---- 3. everyone present, only room moves: the recording calls cut at the moves ---------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("N", [0, 2])
def test_call_equals_recording_calls_cut_at_the_moves(N):
    rng = np.random.default_rng(520)
    ids, lanes = _ids_and_lanes(6)
    ticks, cuts = 60, [0, 25, 40, 60]
    rooms = [ROOMS, np.array([1, 0, -1, 1, 0, 0, 2, 2, 5, 5, 5], np.int32), np.array([0, 0, 0, 0, 0, 0, 0, 3, 3, -2, 3], np.int32)]
    stays = as_stays([(p, int(rooms[i][p]), cuts[i], cuts[i + 1] - cuts[i]) for p in range(P) for i in range(3)])
    spans, F = meeting_layout(ids, stays)
    rec = draw_recording(rng, P, ticks)
    a, u = _ctx(MS), _ctx(MS)
    try:
        got = meeting_call(a, spans, F, stays, rec, DTX, 0, N, lanes)
        want = filled_frames(F)
        for i in range(3):
            seg, part = span_call(u, spans, F, rooms[i], rec, DTX, 0, N, lanes, cuts[i], cuts[i + 1])
            for k in want:
                for (_, first, n) in part:
                    want[k][first + cuts[i]:first + cuts[i] + n] = seg[k][first:first + n]
        check_meeting_frames("against the cut calls", got, want, spans)
        _check_state("against the cut calls", a, u, ids, lanes)
    finally:
        a.close()
        u.close()


# ---- 4. continuation --------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_calls_continue_live_streams_and_ticks_continue_calls():
    """4 lossy ticks on both contexts (mid-burst), a meeting call of 50 ticks, a second one of 40 ticks with another schedule,
    5 ticks: the whole equals the twin's 99 ticks with the present rows, state included"""
    rng = np.random.default_rng(77)
    ids, lanes = _ids_and_lanes(5)
    pre, n1, n2, post = 4, 50, 40, 5
    rec = draw_recording(rng, P, pre + n1 + n2 + post)
    rec["sizes"][2:pre + 3, 4] = 0                      # participant 4 is inside a burst when the first call begins
    rooms2 = np.array([1, 0, -1, 1, 0, 0, 2, 2, 5, 5, 5], np.int32)
    one = {p: [(p, int(ROOMS[p]), 0, n1)] for p in range(P)}
    one[3] = [(3, 1, 10, n1 - 10)]
    one[6] = [(6, 3, 0, 20), (6, 0, 35, n1 - 35)]
    two = {p: [(p, int(rooms2[p]), 0, n2)] for p in range(P)}
    two[6] = [(6, 2, 5, 30)]                             # 6 comes back late, mid-call, and leaves early
    two[0] = []                                          # 0 takes no part in the second call
    parts = [(_everyone(ROOMS, pre), 0), (as_stays([s for p in range(P) for s in one[p]]), pre),
             (as_stays([s for p in range(P) for s in two[p]]), pre + n1), (_everyone(ROOMS, post), pre + n1 + n2)]
    a, u = _ctx(MS), _ctx(MS)
    try:
        for i, (stays, off) in enumerate(parts):
            spans, F = meeting_layout(ids, stays)
            want = twin_meeting_ticks(u, ids, spans, stays, rec, DTX, 0, 0, F, tick_of=lambda t, off=off: t + off)
            if i in (0, 3):
                got = twin_meeting_ticks(a, ids, spans, stays, rec, DTX, 0, 0, F, tick_of=lambda t, off=off: t + off)
            else:
                got = meeting_call(a, spans, F, stays, rec, DTX, 0, 0, lanes, tick_of=lambda t, off=off: t + off)
            check_meeting_frames(f"part {i}", got, want, spans)
        _check_state("after the sequence", a, u, ids, lanes)
        assert a.decode_lossy_errors() == 0 and a.encode_mixed_errors() == 0 and a.bridge_errors() == 0
    finally:
        a.close()
        u.close()


# ---- 5. the host form equals the `_dev` form ----------------------------------------------------------------------------------

def _small_schedule(ticks):
    stay = {p: [(p, int(ROOMS[p]), 0, ticks)] for p in range(P)}
    stay[2] = [(2, 0, 12, ticks - 12)]
    stay[7] = [(7, 3, 0, 10), (7, 1, 20, ticks - 20)]
    stay[9] = []
    return as_stays([s for p in range(P) for s in stay[p]])


@pytest.mark.gpu
@pytest.mark.parametrize("N", [0, 3])
def test_host_form_equals_the_dev_form(N):
    from lyra_amd.codec import MEETING_STAY_DTYPE, SPAN_DTYPE
    rng = np.random.default_rng(61)
    ids, lanes = _ids_and_lanes(9)
    ticks = 40
    stays = _small_schedule(ticks)
    spans, F = meeting_layout(ids, stays)
    rec = draw_recording(rng, P, ticks)
    a, u = _ctx(MS), _ctx(MS)
    try:
        want = meeting_call(u, spans, F, stays, rec, DTX, SKIP_CN, N, lanes)
        sp, st = np.array(spans, SPAN_DTYPE), np.array(stays, MEETING_STAY_DTYPE)
        host = {k: _filled(None, F, w, dt) for k, (w, dt) in WIDTH.items()}
        pk, sz = by_present_frame(spans, stays, F, rec["packets"], np.uint8), by_present_frame(spans, stays, F, rec["sizes"], np.int32)
        bits, mu = by_present_frame(spans, stays, F, rec["bits"], np.int32), by_present_frame(spans, stays, F, rec["muted"], np.int32)
        ln = np.ascontiguousarray(lanes, np.int32)
        ptr = lambda k: host[k].ctypes.data   # noqa: E731
        rc = a.L.lyra_hip_spans_meeting(a.h, sp.ctypes.data, P, ln.ctypes.data, ln.size, st.ctypes.data, st.size, pk.ctypes.data,
                                        sz.ctypes.data, mu.ctypes.data, SKIP_CN, bits.ctypes.data, DTX.ctypes.data, N,
                                        ptr("out_packets"), ptr("out_packet_bytes"), ptr("pcm16"), ptr("mix"), ptr("is_noise"),
                                        ptr("is_comfort_noise"), ptr("levels") if N else None, ptr("is_speaker") if N else None)
        assert rc == 0, a.last_error()
        out = np.ones(F, bool)
        for (_, first, n) in spans:
            out[first:first + n] = False
        assert out[spans[9][1]] or spans[9][2] == 0
        for k, g in host.items():
            g = g.reshape(F, -1)
            assert (g[out].view(np.uint8) == FILL).all(), f"{k}: the caller's array was written outside the spans"
            if k in ("levels", "is_speaker") and not N:
                assert (g.view(np.uint8) == FILL).all(), k
                continue
            w = want[k].reshape(F, -1).copy()
            if k == "out_packets":                       # the host form: zero behind each packet's bytes, empty packets included
                for f in np.flatnonzero(~out):
                    w[f, want["out_packet_bytes"][f]:] = 0
            assert np.array_equal(g[~out], w[~out]), (k, np.flatnonzero((g != w).any(axis=1) & ~out)[:8])
        _check_state("host form", a, u, ids, lanes)
        # ... and the binding returns the same, zeros outside the spans
        a.reset()
        u.reset()
        res = a.meeting_spans(spans, stays, pk, sz, bits, lanes, mu, DTX, SKIP_CN, N)
        want2 = meeting_call(u, spans, F, stays, rec, DTX, SKIP_CN, N, lanes)
        assert np.array_equal(res["out_packet_bytes"][~out], want2["out_packet_bytes"][~out]) and not res["mix"][out].any()
        assert np.array_equal(res["mix"][~out], want2["mix"][~out])
        pkw = want2["out_packets"].copy()
        for f in np.flatnonzero(~out):
            pkw[f, want2["out_packet_bytes"][f]:] = 0
        assert np.array_equal(res["out_packets"][~out], pkw[~out])
    finally:
        a.close()
        u.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals_enqueue_nothing_and_change_nothing():
    import torch
    from lyra_amd.codec import MEETING_STAY_DTYPE, SPAN_DTYPE, C, MeetingSpansCall
    rng = np.random.default_rng(71)
    ids, lanes = _ids_and_lanes(13)
    ticks, pre = 40, 6
    stays = _small_schedule(ticks)
    spans, F = meeting_layout(ids, stays)
    rec = draw_recording(rng, P, ticks + pre)
    a, u = _ctx(MS), _ctx(MS)
    L = a.L
    try:
        head = _everyone(ROOMS, pre)
        head_spans, head_F = meeting_layout(ids, head)
        for c in (a, u):                                  # live streams, mid-burst: what a refused call must not move
            twin_meeting_ticks(c, ids, head_spans, head, rec, DTX, 0, 0, head_F)
        everyone = np.concatenate([ids, lanes])
        before = a.export_streams(everyone)
        sp, st = np.array(spans, SPAN_DTYPE), np.array(stays, MEETING_STAY_DTYPE)
        late = {k: v[pre:] for k, v in rec.items()}
        sz, bits = by_present_frame(spans, stays, F, late["sizes"], np.int32), by_present_frame(spans, stays, F, late["bits"], np.int32)
        ln = np.ascontiguousarray(lanes, np.int32)
        dtx = DTX.copy()
        keep = dict(pk=_t(by_present_frame(spans, stays, F, late["packets"], np.uint8)), out=_filled(_dev(), F, ROW, np.uint8),
                    out_n=_filled(_dev(), F, 1, np.int32), x=_filled(_dev(), F + 1, 320, np.int16),
                    mix=_filled(_dev(), F + 1, 320, np.int16), lv=_filled(_dev(), F + 1, 1, np.int64))
        p = {k: v.data_ptr() for k, v in keep.items()}
        torch.cuda.synchronize()   # (the calls below go to the library directly, without the binding's stream ordering)

        def call(**change):
            f = dict(spans=sp.ctypes.data, P=P, lane_ids=ln.ctypes.data, n_lanes=ln.size, stays=st.ctypes.data, n_stays=st.size,
                     d_packets=p["pk"], packet_bytes=sz.ctypes.data, d_muted=None, flags=0, num_bits=bits.ctypes.data,
                     dtx=dtx.ctypes.data, d_out_packets=p["out"], d_out_packet_bytes=p["out_n"], d_pcm16=p["x"], d_mix=p["mix"],
                     d_is_noise=None, d_is_comfort_noise=None, max_speakers=0, d_levels=None, d_is_speaker=None)
            f.update(change)
            t = MeetingSpansCall(**f)
            return L.lyra_hip_spans_meeting_dev(a.h, C.addressof(t))

        def changed(arr, **change):
            s = arr.copy()
            for k, (row, v) in change.items():
                s[k][row] = v
            return s

        i7 = int(np.flatnonzero(st["participant"] == 7)[0])      # participant 7's two stays: rows i7 and i7 + 1
        bad_stays = {"a sum above n_frames": changed(st, n_ticks=(0, ticks + 1)),
                     "a sum below n_frames": changed(st, n_ticks=(i7, 9)),
                     "n_ticks 0": changed(st, n_ticks=(i7, 0)),
                     "overlapping stays": changed(st, first_tick=(i7 + 1, 9)),
                     "a negative first_tick": changed(st, first_tick=(0, -1)),
                     "a participant out of range": changed(st, participant=(st.size - 1, P)),
                     "a negative participant": changed(st, participant=(0, -1)),
                     "unsorted": np.concatenate([st[1:], st[:1]]),
                     "unsorted ticks": np.concatenate([st[:i7], st[i7 + 1:i7 + 2], st[i7:i7 + 1], st[i7 + 2:]])}
        for what, s in bad_stays.items():
            assert call(stays=s.ctypes.data) == EINVAL, what
        bad_spans = {"an id out of range": changed(sp, stream_id=(0, MS)), "an id named twice": changed(sp, stream_id=(1, int(sp["stream_id"][0]))),
                     "a lane's id": changed(sp, stream_id=(2, int(lanes[0]))), "n_frames off the stays": changed(sp, n_frames=(3, ticks - 1)),
                     "frames without a stay": changed(sp, n_frames=(9, 1)),
                     "a negative range": changed(sp, first_frame=(0, -1)), "overlapping ranges": changed(sp, first_frame=(1, int(sp["first_frame"][0]) + 1))}
        for what, s in bad_spans.items():
            assert call(spans=s.ctypes.data) == EINVAL, what
        bad_lane = ln.copy(); bad_lane[3] = bad_lane[2]
        bad_sz = sz.copy(); bad_sz[spans[4][1] + 7] = 9
        bad_bits = bits.copy(); bad_bits[spans[5][1] + 1] = 186
        for change in (dict(lane_ids=bad_lane.ctypes.data), dict(n_lanes=-1), dict(lane_ids=None), dict(packet_bytes=bad_sz.ctypes.data),
                       dict(num_bits=bad_bits.ctypes.data), dict(spans=None), dict(stays=None), dict(n_stays=-1), dict(d_packets=None),
                       dict(packet_bytes=None), dict(num_bits=None), dict(d_out_packets=None), dict(d_out_packet_bytes=None),
                       dict(d_pcm16=None), dict(d_mix=None), dict(d_pcm16=p["x"] + 2), dict(d_mix=p["mix"] + 8),
                       dict(d_mix=p["x"]), dict(d_levels=p["lv"] + 4, max_speakers=2), dict(flags=2), dict(max_speakers=-1),
                       dict(max_speakers=9), dict(P=0), dict(P=MS + 1)):
            assert call(**change) == EINVAL, change
        assert L.lyra_hip_spans_meeting_dev(a.h, None) == EINVAL

        def mix(s=sp.ctypes.data, n=P, y=st.ctypes.data, ny=st.size, x=p["x"], out=p["mix"], N=0, lv=None):   # the pass alone
            return L.lyra_hip_spans_meeting_mix_dev(a.h, s, n, y, ny, x, None, None, N, out, lv, None)
        for kw in (dict(s=None), dict(y=None), dict(ny=-1), dict(x=None), dict(out=None), dict(n=0), dict(n=MS + 1), dict(x=p["x"] + 2),
                   dict(out=p["mix"] + 4), dict(out=p["x"]), dict(N=9), dict(N=-1), dict(N=2, lv=p["lv"] + 4),
                   dict(y=bad_stays["overlapping stays"].ctypes.data), dict(y=bad_stays["unsorted"].ctypes.data),
                   dict(s=bad_spans["overlapping ranges"].ctypes.data)):
            assert mix(**kw) == EINVAL, kw
        a.synchronize()
        for k in ("out", "out_n", "x", "mix"):
            assert (keep[k].cpu().numpy().view(np.uint8) == FILL).all(), f"a refused call wrote {k}"
        assert np.array_equal(a.export_streams(everyone), before), "a refused call changed stream state"
        assert a.decode_lossy_errors() == 0 and a.encode_mixed_errors() == 0 and a.bridge_errors() == 0
        # a valid call now equals a twin that never saw a bad call
        want = twin_meeting_ticks(u, ids, spans, stays, rec, DTX, 0, 0, F, tick_of=lambda t: t + pre)
        got = meeting_call(a, spans, F, stays, rec, DTX, 0, 0, lanes, tick_of=lambda t: t + pre)
        check_meeting_frames("after the refusals", got, want, spans)
        _check_state("after the refusals", a, u, ids, lanes)
        # DTX needs the context's encoder rate at 16000, as the header says; without DTX the rate is not read
        a.set_encoder_sample_rate(48000)
        after = a.export_streams(everyone)
        assert call() == EINVAL and "16000" in a.last_error()
        assert np.array_equal(a.export_streams(everyone), after)
        assert call(dtx=None) == 0, a.last_error()
        a.synchronize()
    finally:
        a.close()
        u.close()


# ---- 7. bridge_demo mode 3 ---------------------------------------------------------------------------------------------------

def _demo(tmp_path, mode, streams, script, packets, lengths, present, max_speakers):
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "bridge_demo")
    assert os.path.exists(demo), "lyra_amd/bridge_demo not built (__graft_entry__.build())"
    (tmp_path / "streams.txt").write_text("".join(f"{b} {d}\n" for b, d in streams))
    for name, arr in (("script.i32", script), ("pk.bin", packets), ("len.i32", lengths), ("present.i32", present)):
        arr.tofile(tmp_path / name)
    tag = f"{mode}_{max_speakers}"
    out, out_n, spk = (tmp_path / f"out{tag}.bin", tmp_path / f"out{tag}.i32", tmp_path / f"spk{tag}.i32")
    sel = [f"--max-speakers={max_speakers}", f"--speakers-out={spk}"] if max_speakers else []
    r = subprocess.run([demo, lyra_amd.default_model_dir(), str(tmp_path / "streams.txt"), str(tmp_path / "script.i32"),
                        str(tmp_path / "pk.bin"), str(tmp_path / "len.i32"), str(out), str(out_n), str(mode), "1"] + sel +
                       [f"--present={tmp_path / 'present.i32'}"] + (["--lanes=26"] if mode == 3 else []),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (mode, r.returncode, r.stderr[-3000:])
    return out.read_bytes(), out_n.read_bytes(), spk.read_bytes() if max_speakers else b""


@pytest.mark.gpu
@pytest.mark.parametrize("N", [0, 3])
def test_bridge_demo_mode_3_equals_mode_0(tmp_path, N):
    ticks, n = 120, 13
    rng = np.random.default_rng(81)
    rates = (3200, 6000, 9200)
    streams = [(rates[s % 3], s % 2) for s in range(n)]
    script = np.zeros((ticks, n, 3), np.int32)
    script[:, :, 0] = (np.arange(n) // 4)[None, :]
    script[70:, :, 0] = rng.integers(-1, 3, n)[None, :]                # room moves at tick 70 ...
    script[95:, 3, 0] = 2
    script[:, :, 1] = rng.random((ticks, n)) < 0.1                     # ... mutes come and go ...
    script[:, :, 2] = np.array(rates)[rng.integers(0, 3, (ticks, n))]  # ... and bitrates change from tick to tick
    present = np.ones((ticks, n), np.int32)
    present[:25, 1] = 0                                                # a join,
    present[100:, 6] = 0                                               # a leave,
    present[40:60, 9] = 0                                              # a gap,
    present[:, 12] = 0                                                 # and somebody who never shows up
    rec = draw_recording(rng, n, ticks)
    tick_by_tick = _demo(tmp_path, 0, streams, script, rec["packets"], rec["sizes"], present, N)
    whole = _demo(tmp_path, 3, streams, script, rec["packets"], rec["sizes"], present, N)
    assert len(tick_by_tick[0]) == ticks * n * ROW and len(tick_by_tick[1]) == ticks * n * 4
    lens = np.frombuffer(tick_by_tick[1], np.int32).reshape(ticks, n)
    assert (lens[present == 1] == 0).any() and (lens > 0).any() and not lens[present == 0].any()
    assert whole[1] == tick_by_tick[1], "outgoing lengths"
    assert whole[0] == tick_by_tick[0], "outgoing packets"
    assert whole[2] == tick_by_tick[2], "speaker flags"
    if N:
        assert np.frombuffer(whole[2], np.int32).any()
