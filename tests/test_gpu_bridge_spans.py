"""A meeting recording through the bridge in one call (include/lyra_hip_bridge_spans.h): the pass against the formula, the call
against the tick calls on a twin context (full mix and loudest-N), continuation across calls and ticks, the call against the
reference model, the host form against the `_dev` form, the refusals, and bridge_demo mode 2.  Helpers: tests/bridge_span_cases.py.

Shapes.  The pass serves one (room, tick) or one (8 positions, tick) per wavefront, four per workgroup, members in chunks of 8,
rooms above 64 through parked keys: the 330-participant shape of the tick kernels' tests (rooms of 1, 2, 3, 8, 9, 16, 17 and 257)
over 3 ticks.  The legs need lane chunks with warm-up (25 hops on both sides): T = 120 on 24 lanes gives every span two."""
import os
import subprocess

import numpy as np
import pytest

from bridge_models import SKIP_CN, BridgeModel, bridge_kernel_case, np_bridge_mix, np_bridge_plan
from bridge_span_cases import (WIDTH, FilledBufs, ROW, by_frame, check_frames, draw_recording, frames_of, recording_layout, span_call,
                               twin_ticks)
from gpu_plumbing import FILL, _dev, _filled, _t, make_ctx as _ctx, stream_cases
from receiver_models import _model_packets
from span_cases import _check_state
from speaker_models import _source, np_levels, np_speakers_mix, speakers_kernel_case, tie_decided

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
EINVAL = -1
FILL16 = 21845


# ---- 1. the pass against the formula ---------------------------------------------------------------------------------------

def _pass_inputs(x0, muted0, cn_row_of_tick, T=3):
    """T ticks from one tick's rows: the samples rotated (rows of a constant stay what they are: both saturations stay), mutes
    that differ from tick to tick, one comfort-noise row per tick"""
    rng = np.random.default_rng(17)
    B = x0.shape[0]
    xs = [np.roll(x0, 5 * t, axis=1) if t else x0 for t in range(T)]
    muted = [muted0.copy() for _ in range(T)]
    cns = []
    for t in range(T):
        if t:
            flip = rng.choice(B, 12, replace=False)
            muted[t][flip] ^= 1
        cn = np.zeros(B, np.int32)
        cn[cn_row_of_tick[t]] = 1
        cns.append(cn)
    assert any((muted[t] != muted[0]).any() for t in range(1, T))
    return xs, muted, cns


def _run_pass(a, spans, F, rooms, xs, muted, cns, max_speakers):
    """bridge_spans_mix_dev on FILL-prefilled buffers -> (mix [F][320], levels [F], is_speaker [F])"""
    T = len(xs)
    d_x = _t(by_frame(spans, F, np.stack(xs), np.int16))
    d_m = _t(by_frame(spans, F, np.stack(muted), np.int32))
    d_c = _t(by_frame(spans, F, np.stack(cns), np.int32))
    d_mix = _filled(_dev(), F, 320, np.int16)
    d_lv, d_sp = _filled(_dev(), F, 1, np.int64).view(-1), _filled(_dev(), F, 1, np.int32).view(-1)
    a.bridge_spans_mix_dev(spans, rooms, d_x, d_mix, max_speakers, d_m, d_c, d_lv if max_speakers else None,
                           d_sp if max_speakers else None)
    a.synchronize()
    assert T == spans[0][2]
    return d_mix.cpu().numpy(), d_lv.cpu().numpy(), d_sp.cpu().numpy()


def _outside(spans, F):
    covered = np.zeros(F, bool)
    for (_, first, n) in spans:
        covered[first:first + n] = True
    return ~covered


@pytest.mark.gpu
def test_full_mix_pass_equals_the_formula_on_every_tick():
    x0, rooms, muted0, is_cn0 = bridge_kernel_case()
    B = x0.shape[0]
    order, start = np_bridge_plan(rooms)
    assert sorted(np.diff(start).tolist()) == [1, 2, 3, 8, 9, 16, 17, 257] and (rooms < 0).any()
    in8 = np.flatnonzero((rooms == 3))
    xs, muted, cns = _pass_inputs(x0, muted0, [int(np.flatnonzero(is_cn0)[0]), int(in8[1]), int(in8[2])])
    spans, F = recording_layout(np.arange(B), 3)
    assert sorted(set(np.diff([s[1] for s in spans]).tolist())) == [3, 4, 6], "gaps of 0, 1 and 3 frames between the spans"
    a = _ctx(512)
    try:
        mix, lv, sp = _run_pass(a, spans, F, rooms, xs, muted, cns, 0)
        sat_hi = sat_lo = False
        for t in range(3):
            want = np_bridge_mix(xs[t], order, start, muted[t], cns[t])
            got = mix[frames_of(spans, t)]
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, (f"tick {t}: rows differ from the formula", bad[:16], rooms[bad[:16]])
            assert not got[rooms < 0].any(), f"tick {t}: a participant in no room hears something"
            sat_hi |= bool((want == 32767).any())
            sat_lo |= bool((want == -32768).any())
        assert sat_hi and sat_lo, "the case must saturate on both sides"
        out = _outside(spans, F)
        assert out.sum() >= 3 and (mix[out] == FILL16).all(), "a sentinel frame between or behind the spans was written"
        assert (lv.view(np.uint8) == FILL).all() and (sp.view(np.uint8) == FILL).all()
        assert a.bridge_errors() == 0
    finally:
        a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 3, 8])
def test_selection_pass_equals_the_model_on_every_tick(N):
    x0, rooms, muted0, is_cn0, _, _ = speakers_kernel_case()
    B = x0.shape[0]
    order, start = np_bridge_plan(rooms)       # the library builds the index itself: rows ascending inside a room
    in8 = np.flatnonzero((rooms == 3))
    xs, muted, cns = _pass_inputs(x0, muted0, [int(np.flatnonzero(is_cn0)[0]), int(in8[1]), int(in8[2])])
    # the constructed tie: the 16-room's five identical rows of +32767 -- on tick 0 the position rule decides for N < 5
    lv0 = np_levels(xs[0])
    if N < 5:
        assert tie_decided(lv0, order, start, _source(B, muted[0], cns[0]), N), "no tie is decided by position"
    spans, F = recording_layout(np.arange(B), 3)
    a = _ctx(512)
    try:
        mix, lv, sp = _run_pass(a, spans, F, rooms, xs, muted, cns, N)
        for t in range(3):
            want, w_lv, w_sp = np_speakers_mix(xs[t], order, start, N, muted[t], cns[t])
            f = frames_of(spans, t)
            assert np.array_equal(lv[f], w_lv), f"tick {t}: levels"
            assert np.array_equal(sp[f], w_sp), (f"tick {t}: is_speaker differs in rows", np.flatnonzero(sp[f] != w_sp)[:16])
            bad = np.flatnonzero((mix[f] != want).any(axis=1))
            assert bad.size == 0, (f"tick {t}: rows differ from the model", bad[:16], rooms[bad[:16]])
        out = _outside(spans, F)
        assert (mix[out] == FILL16).all() and (lv[out].view(np.uint8) == FILL).all() and (sp[out].view(np.uint8) == FILL).all()
        if N == 8:
            # at most 8 candidates per room: the selection is the full mix, bit for bit
            few = [np.ones(B, np.int32) for _ in range(3)]
            for r in range(len(start) - 1):
                for t in range(3):
                    few[t][order[start[r]:start[r + 1]][t:t + 8]] = 0
            sel, _, _ = _run_pass(a, spans, F, rooms, xs, few, cns, 8)
            full, _, _ = _run_pass(a, spans, F, rooms, xs, few, cns, 0)
            assert np.array_equal(sel, full)
            for t in range(3):
                assert np.array_equal(full[frames_of(spans, t)], np_bridge_mix(xs[t], order, start, few[t], cns[t])), t
            assert full[~out].any()
    finally:
        a.close()


# ---- 2, 3. the call equals the tick ----------------------------------------------------------------------------------------

MS, P, T, LANES = 64, 11, 120, 24
ROOMS = np.array([0, 0, 0, 1, 1, 2, 3, 3, 3, 3, -1], np.int32)
DTX = (np.arange(P) % 2).astype(np.int32)


def _ids_and_lanes(seed):
    perm = np.random.default_rng(seed).permutation(MS).astype(np.int32)
    return perm[:P], perm[P:P + LANES]


def _assert_lane_chunks(spans, lanes):
    import lyra_amd.codec as codec
    for side in ("decoder", "encoder"):
        chunks, _ = codec.spans_plan(side, spans, lanes, MS)
        assert (chunks["n_warmup"] > 0).any(), f"{side}: the plan uses no lane chunk with warm-up"


def _equal_case(mode="xnnpack", serial=False, flags=0, max_speakers=0, **kw):
    rng = np.random.default_rng(200 + max_speakers)
    ids, lanes = _ids_and_lanes(3)
    spans, F = recording_layout(ids, T)
    _assert_lane_chunks(spans, lanes)
    rec = draw_recording(rng, P, T, outage=(1, 6, 14))        # participant 1 of room 0: 14 ticks lost, into comfort noise
    assert set(np.unique(rec["sizes"])) == {0, 8, 15, 23} and (rec["muted"][0] != rec["muted"][1]).any()
    if flags & SKIP_CN:
        rec["muted"][:, :3] = 0
    a, u = _ctx(MS, mode, **kw), _ctx(MS, mode, **kw)
    try:
        if serial:
            a.set_serial(True)
            u.set_serial(True)
        want = twin_ticks(u, ids, ROOMS, rec, DTX, flags, max_speakers)
        got, _ = span_call(a, spans, F, ROOMS, rec, DTX, flags, max_speakers, lanes)
        assert want["is_comfort_noise"][:, 1].any(), "the outage never reached comfort noise"
        assert (want["out_packet_bytes"] == 0).any() and (want["out_packet_bytes"] > 0).all(axis=0).any(), \
            "the case needs empty DTX packets and streams without any"
        check_frames("one call", got, want, spans, max_speakers != 0)
        _check_state("after the call", a, u, ids, lanes)
        assert a.decode_lossy_errors() == 0 and a.encode_mixed_errors() == 0 and a.bridge_errors() == 0
        if flags & SKIP_CN:
            changed = 0
            order, start = np_bridge_plan(ROOMS)
            for t in range(T):
                plain = np_bridge_mix(want["pcm16"][t], order, start, rec["muted"][t], None)
                changed += int(not np.array_equal(plain[:3], want["mix"][t][:3]))
            assert changed >= 1, "SKIP_COMFORT_NOISE never changed a mix row of the room with the lost member"
        if max_speakers:
            assert want["is_speaker"].any() and not want["is_speaker"].all()
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode,streams", stream_cases(["xnnpack", "builtin_mixed"], plain="xnnpack"))
def test_call_equals_the_ticks_full_mix(mode, streams):
    _equal_case(mode, streams=streams)


@pytest.mark.gpu
def test_call_equals_the_ticks_in_serial_order():
    _equal_case(serial=True)


@pytest.mark.gpu
def test_call_equals_the_ticks_on_a_split_context():
    _equal_case(sub_batches=2)


@pytest.mark.gpu
def test_call_skips_comfort_noise_rows_when_asked():
    """SKIP_COMFORT_NOISE with no d_is_comfort_noise would use the library's scratch; here the array is given and compared"""
    _equal_case(flags=SKIP_CN)


@pytest.mark.gpu
def test_call_with_library_scratch_for_the_comfort_noise_flags():
    """SKIP_COMFORT_NOISE without d_is_comfort_noise (and without d_is_noise): the library's own flag array is written by the
    decode leg and read by the pass; everything else is what the call that was given every buffer delivers"""
    rng = np.random.default_rng(210)
    ids, lanes = _ids_and_lanes(4)
    ticks = 60
    spans, F = recording_layout(ids, ticks)
    rec = draw_recording(rng, P, ticks, outage=(1, 6, 14))
    rec["muted"][:, :3] = 0
    a, u = _ctx(MS), _ctx(MS)
    try:
        want, part = span_call(u, spans, F, ROOMS, rec, DTX, SKIP_CN, 0, lanes)
        got, _ = span_call(a, spans, F, ROOMS, rec, DTX, SKIP_CN, 0, lanes, noise_flags=False)
        f1 = np.arange(part[1][1], part[1][1] + ticks)
        assert want["is_comfort_noise"][f1].any(), "the outage never reached comfort noise"
        for k in ("out_packet_bytes", "out_packets", "pcm16", "mix"):
            assert np.array_equal(got[k], want[k]), k
        for k in ("is_noise", "is_comfort_noise"):
            assert (got[k].view(np.uint8) == FILL).all(), f"{k} was written although the call was not given it"
        _check_state("library scratch", a, u, ids, lanes)
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 3])
def test_call_equals_the_ticks_loudest_n(N):
    _equal_case(max_speakers=N)


# ---- 4. continuation -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_calls_continue_live_streams_and_ticks_continue_calls():
    """a few lossy ticks on both contexts (mid-burst), a call of 70 ticks, a call of 50 ticks with other rooms, 5 ticks: the
    whole equals 4 + 125 ticks on the twin, state included"""
    rng = np.random.default_rng(77)
    ids, lanes = _ids_and_lanes(5)
    pre, n1, n2, post = 4, 70, 50, 5
    total = pre + n1 + n2 + post
    rec = draw_recording(rng, P, total)
    rec["sizes"][2:pre + 3, 4] = 0                      # participant 4 is inside a burst when the first call begins
    rooms2 = np.array([1, 0, -1, 1, 0, 0, 2, 2, 5, 5, 5], np.int32)
    spans, F = recording_layout(ids, n1)
    a, u = _ctx(MS), _ctx(MS)
    try:
        want = [twin_ticks(u, ids, ROOMS, rec, DTX, 0, 0, 0, pre + n1), twin_ticks(u, ids, rooms2, rec, DTX, 0, 0, pre + n1, pre + n1 + n2),
                twin_ticks(u, ids, ROOMS, rec, DTX, 0, 0, pre + n1 + n2, total)]
        head = twin_ticks(a, ids, ROOMS, rec, DTX, 0, 0, 0, pre)
        for k in head:
            assert np.array_equal(head[k], want[0][k][:pre]), k
        got1, part1 = span_call(a, spans, F, ROOMS, rec, DTX, 0, 0, lanes, pre, pre + n1)
        check_frames("first call", got1, {k: v[pre:] for k, v in want[0].items()}, part1, False)
        got2, part2 = span_call(a, spans, F, rooms2, rec, DTX, 0, 0, lanes, pre + n1, pre + n1 + n2)
        check_frames("second call, other rooms", got2, want[1], part2, False)
        tail = twin_ticks(a, ids, ROOMS, rec, DTX, 0, 0, pre + n1 + n2, total)
        for k in tail:
            assert np.array_equal(tail[k], want[2][k]), ("ticks behind the calls", k)
        _check_state("after the sequence", a, u, ids, lanes)
    finally:
        a.close()
        u.close()


# ---- 5. against the reference model ----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_call_against_the_reference_model(oracle_default, golden_dir):
    n, ticks = 6, 60
    rooms = np.array([0, 0, 0, 1, 1, 2], np.int32)
    muted = np.zeros(n, np.int32)
    muted[2] = 1
    three = (184, 120, 64)
    in_bits = [three[i % 3] for i in range(n)]
    out_bits = np.array([three[(i + 1) % 3] for i in range(n)], np.int32)
    dtx = np.ones(n, np.int32)
    packets, nbytes = _model_packets(oracle_default, golden_dir, in_bits, ticks)
    rx = np.ones((ticks, n), bool)
    rx[10:24, 3] = False                                  # one lost stretch, into comfort noise
    ids = np.arange(n, dtype=np.int32) + 3
    lanes = np.arange(12, dtype=np.int32) + 16
    rec = dict(packets=packets, sizes=(nbytes[None, :] * rx).astype(np.int32), bits=np.tile(out_bits, (ticks, 1)),
               muted=np.tile(muted, (ticks, 1)))
    model = BridgeModel(oracle_default, ids, rooms, muted, out_bits, dtx)
    spans, F = recording_layout(ids, ticks)
    a = _ctx(32)
    try:
        bufs = FilledBufs(F)
        bufs.t["out_packets"].zero_()                    # (the model's rows are zero behind each packet)
        got, _ = span_call(a, spans, F, rooms, rec, dtx, 0, 0, lanes, bufs=bufs)
        order, start = np_bridge_plan(rooms)
        for t in range(ticks):
            f = frames_of(spans, t)
            hops, reach, _, _, _, m_cn = model.tick(packets[t], rec["sizes"][t])
            for b in range(n):
                model.tally.check(got["pcm16"][f[b]], hops[b], reach[b], f"tick {t}, row {b}, 16 kHz")
            assert np.array_equal(got["is_comfort_noise"][f], m_cn), f"tick {t}: is_comfort_noise"
            mix = got["mix"][f]
            assert np.array_equal(mix, np_bridge_mix(got["pcm16"][f], order, start, muted)), f"tick {t}: the mix over the device's own hop"
            want_pk, want_sz = model.encode_of(mix)
            assert np.array_equal(got["out_packet_bytes"][f], want_sz), (f"tick {t}: outgoing sizes", got["out_packet_bytes"][f], want_sz)
            assert np.array_equal(got["out_packets"][f], want_pk), f"tick {t}: outgoing packets"
        model.tally.report("bridge_spans d_pcm16")
        assert got["is_comfort_noise"][frames_of(spans, 20)[3]] == 1
    finally:
        a.close()


# ---- 6. the host form equals the `_dev` form --------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("N", [0, 3])
def test_host_form_equals_the_dev_form(N):
    from lyra_amd.codec import SPAN_DTYPE
    rng = np.random.default_rng(61)
    ids, lanes = _ids_and_lanes(9)
    ticks = 40
    spans, F = recording_layout(ids, ticks)
    rec = draw_recording(rng, P, ticks)
    a, u = _ctx(MS), _ctx(MS)
    try:
        want, part = span_call(u, spans, F, ROOMS, rec, DTX, SKIP_CN, N, lanes)
        sp = np.array(part, SPAN_DTYPE)
        host = {k: _filled(None, F, w, dt) for k, (w, dt) in WIDTH.items()}
        pk, sz = by_frame(part, F, rec["packets"], np.uint8), by_frame(part, F, rec["sizes"], np.int32)
        bits, mu = by_frame(part, F, rec["bits"], np.int32), by_frame(part, F, rec["muted"], np.int32)
        ln = np.ascontiguousarray(lanes, np.int32)
        ptr = lambda k: host[k].ctypes.data   # noqa: E731
        rc = a.L.lyra_hip_spans_bridge(a.h, sp.ctypes.data, P, ln.ctypes.data, ln.size, ROOMS.ctypes.data, pk.ctypes.data,
                                       sz.ctypes.data, mu.ctypes.data, SKIP_CN, bits.ctypes.data, DTX.ctypes.data, N,
                                       ptr("out_packets"), ptr("out_packet_bytes"), ptr("pcm16"), ptr("mix"), ptr("is_noise"),
                                       ptr("is_comfort_noise"), ptr("levels") if N else None, ptr("is_speaker") if N else None)
        assert rc == 0, a.last_error()
        out = _outside(part, F)
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
        res = a.bridge_spans(part, ROOMS, pk, sz, bits, lanes, mu, DTX, SKIP_CN, N)
        want2, _ = span_call(u, spans, F, ROOMS, rec, DTX, SKIP_CN, N, lanes)
        assert np.array_equal(res["out_packet_bytes"][~out], want2["out_packet_bytes"][~out]) and not res["mix"][out].any()
        assert np.array_equal(res["mix"][~out], want2["mix"][~out])
    finally:
        a.close()
        u.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals_enqueue_nothing_and_change_nothing():
    import torch
    from lyra_amd.codec import SPAN_DTYPE, BridgeSpansCall, C
    rng = np.random.default_rng(71)
    ids, lanes = _ids_and_lanes(13)
    ticks = 40
    spans, F = recording_layout(ids, ticks)
    rec = draw_recording(rng, P, ticks + 6)
    a, u = _ctx(MS), _ctx(MS)
    L = a.L
    try:
        for c in (a, u):                                  # live streams, mid-burst: what a refused call must not move
            twin_ticks(c, ids, ROOMS, rec, DTX, 0, 0, 0, 6)
        everyone = np.concatenate([ids, lanes])
        before = a.export_streams(everyone)
        part = [(i, first, ticks) for (i, first, _) in spans]
        sp = np.array(part, SPAN_DTYPE)
        sl = slice(6, 6 + ticks)
        sz, bits = by_frame(part, F, rec["sizes"][sl], np.int32), by_frame(part, F, rec["bits"][sl], np.int32)
        ln = np.ascontiguousarray(lanes, np.int32)
        dtx = DTX.copy()
        keep = dict(pk=_t(by_frame(part, F, rec["packets"][sl], np.uint8)), out=_filled(_dev(), F, ROW, np.uint8),
                    out_n=_filled(_dev(), F, 1, np.int32), x=_filled(_dev(), F + 1, 320, np.int16),
                    mix=_filled(_dev(), F + 1, 320, np.int16), lv=_filled(_dev(), F + 1, 1, np.int64))
        p = {k: v.data_ptr() for k, v in keep.items()}
        torch.cuda.synchronize()   # (the calls below go to the library directly, without the binding's stream ordering)

        def call(**change):
            f = dict(spans=sp.ctypes.data, P=P, lane_ids=ln.ctypes.data, n_lanes=ln.size, rooms=ROOMS.ctypes.data,
                     d_packets=p["pk"], packet_bytes=sz.ctypes.data, d_muted=None, flags=0, num_bits=bits.ctypes.data,
                     dtx=dtx.ctypes.data, d_out_packets=p["out"], d_out_packet_bytes=p["out_n"], d_pcm16=p["x"], d_mix=p["mix"],
                     d_is_noise=None, d_is_comfort_noise=None, max_speakers=0, d_levels=None, d_is_speaker=None)
            f.update(change)
            t = BridgeSpansCall(**f)
            return L.lyra_hip_spans_bridge_dev(a.h, C.addressof(t))

        def spans_with(**change):
            s = sp.copy()
            for k, (row, v) in change.items():
                s[k][row] = v
            return s

        bad_spans = {"an id out of range": spans_with(stream_id=(0, MS)), "an id named twice": spans_with(stream_id=(1, int(sp["stream_id"][0]))),
                     "a lane's id": spans_with(stream_id=(2, int(lanes[0]))), "unequal n_frames": spans_with(n_frames=(3, ticks - 1)),
                     "a negative range": spans_with(first_frame=(0, -1)), "overlapping ranges": spans_with(first_frame=(1, int(sp["first_frame"][0]) + 1))}
        for what, s in bad_spans.items():
            assert call(spans=s.ctypes.data) == EINVAL, what
        bad_lane = ln.copy(); bad_lane[3] = bad_lane[2]
        bad_sz = sz.copy(); bad_sz[part[4][1] + 7] = 9
        bad_bits = bits.copy(); bad_bits[part[5][1] + 1] = 186
        # (a room above LYRA_HIP_BRIDGE_MAX_ROOM needs more participants than these contexts hold streams: it has a context
        # of its own in test_a_room_above_the_bound_is_refused_by_the_device_calls)
        for change in (dict(lane_ids=bad_lane.ctypes.data), dict(n_lanes=-1), dict(lane_ids=None), dict(packet_bytes=bad_sz.ctypes.data),
                       dict(num_bits=bad_bits.ctypes.data), dict(spans=None), dict(rooms=None), dict(d_packets=None),
                       dict(packet_bytes=None), dict(num_bits=None), dict(d_out_packets=None), dict(d_out_packet_bytes=None),
                       dict(d_pcm16=None), dict(d_mix=None), dict(d_pcm16=p["x"] + 2), dict(d_mix=p["mix"] + 8),
                       dict(d_mix=p["x"]), dict(d_levels=p["lv"] + 4, max_speakers=2), dict(flags=2), dict(max_speakers=-1),
                       dict(max_speakers=9), dict(P=0), dict(P=MS + 1)):
            assert call(**change) == EINVAL, change
        assert L.lyra_hip_spans_bridge_dev(a.h, None) == EINVAL
        # the pass alone
        def mix(s=sp.ctypes.data, n=P, r=ROOMS.ctypes.data, x=p["x"], out=p["mix"], N=0, lv=None):
            return L.lyra_hip_spans_bridge_mix_dev(a.h, s, n, r, x, None, None, N, out, lv, None)
        for kw in (dict(s=None), dict(r=None), dict(x=None), dict(out=None), dict(n=0), dict(n=MS + 1), dict(x=p["x"] + 2),
                   dict(out=p["mix"] + 4), dict(out=p["x"]), dict(N=9), dict(N=-1), dict(N=2, lv=p["lv"] + 4),
                   dict(s=bad_spans["unequal n_frames"].ctypes.data), dict(s=bad_spans["overlapping ranges"].ctypes.data)):
            assert mix(**kw) == EINVAL, kw
        a.synchronize()
        for k in ("out", "out_n", "x", "mix"):
            assert (keep[k].cpu().numpy().view(np.uint8) == FILL).all(), f"a refused call wrote {k}"
        assert np.array_equal(a.export_streams(everyone), before), "a refused call changed stream state"
        assert a.decode_lossy_errors() == 0 and a.encode_mixed_errors() == 0 and a.bridge_errors() == 0
        # a valid call now equals a twin that never saw a bad call
        want = twin_ticks(u, ids, ROOMS, rec, DTX, 0, 0, 6, 6 + ticks)
        got, _ = span_call(a, spans, F, ROOMS, rec, DTX, 0, 0, lanes, 6, 6 + ticks)
        check_frames("after the refusals", got, want, part, False)
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


@pytest.mark.gpu
def test_a_room_above_the_bound_is_refused_by_the_device_calls():
    """LYRA_HIP_BRIDGE_MAX_ROOM + 1 participants in one room, one tick, on a context that holds them and one lane: a call that
    is valid in everything else (the same spans with one participant outside the room pass the planner), so the refusal is
    the room's.  State: the blobs of 64 participants spread over the id range, the last one and the lane stand for all of
    them -- a refusal is decided on the host arrays before anything is enqueued, for every participant alike."""
    import torch
    from bridge_models import MAX_ROOM
    from lyra_amd import codec
    from lyra_amd.codec import SPAN_DTYPE, BridgeSpansCall, C
    n = MAX_ROOM + 1
    a = _ctx(n + 1)
    L = a.L
    try:
        sp = np.zeros(n, SPAN_DTYPE)
        sp["stream_id"] = np.arange(n)
        sp["first_frame"] = np.arange(n)
        sp["n_frames"] = 1
        rooms = np.full(n, 4, np.int32)
        fits = rooms.copy()
        fits[n // 2] = -1
        order, start = codec.bridge_spans_plan(sp, fits)[:2]
        assert start.tolist() == [0, MAX_ROOM] and order.size == MAX_ROOM
        lane = np.array([n], np.int32)
        sz, bits = np.full(n, 23, np.int32), np.full(n, 184, np.int32)
        probe = np.unique(np.concatenate([np.linspace(0, n - 1, 64).astype(np.int32), lane]))
        before = a.export_streams(probe)
        keep = dict(pk=_filled(_dev(), n, ROW, np.uint8), out=_filled(_dev(), n, ROW, np.uint8), out_n=_filled(_dev(), n, 1, np.int32),
                    x=_filled(_dev(), n, 320, np.int16), mix=_filled(_dev(), n, 320, np.int16))
        p = {k: v.data_ptr() for k, v in keep.items()}
        torch.cuda.synchronize()
        for N in (0, 3):
            t = BridgeSpansCall(spans=sp.ctypes.data, P=n, lane_ids=lane.ctypes.data, n_lanes=1, rooms=rooms.ctypes.data,
                                d_packets=p["pk"], packet_bytes=sz.ctypes.data, d_muted=None, flags=0, num_bits=bits.ctypes.data,
                                dtx=None, d_out_packets=p["out"], d_out_packet_bytes=p["out_n"], d_pcm16=p["x"], d_mix=p["mix"],
                                d_is_noise=None, d_is_comfort_noise=None, max_speakers=N, d_levels=None, d_is_speaker=None)
            assert L.lyra_hip_spans_bridge_dev(a.h, C.addressof(t)) == EINVAL
            assert f"a room of more than {MAX_ROOM} members" in a.last_error(), a.last_error()
            assert L.lyra_hip_spans_bridge_mix_dev(a.h, sp.ctypes.data, n, rooms.ctypes.data, p["x"], None, None, N, p["mix"],
                                                   None, None) == EINVAL
            assert f"a room of more than {MAX_ROOM} members" in a.last_error(), a.last_error()
        a.synchronize()
        for k, v in keep.items():
            assert bool((v.view(torch.uint8) == FILL).all()), f"a refused call wrote {k}"
        assert np.array_equal(a.export_streams(probe), before), "a refused call changed stream state"
        assert a.decode_lossy_errors() == 0 and a.encode_mixed_errors() == 0 and a.bridge_errors() == 0
    finally:
        a.close()


# ---- 8. bridge_demo mode 2 -------------------------------------------------------------------------------------------------

def _demo(tmp_path, mode, streams, script, packets, lengths, max_speakers):
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "bridge_demo")
    assert os.path.exists(demo), "lyra_amd/bridge_demo not built (__graft_entry__.build())"
    (tmp_path / "streams.txt").write_text("".join(f"{b} {d}\n" for b, d in streams))
    for name, arr in (("script.i32", script), ("pk.bin", packets), ("len.i32", lengths)):
        arr.tofile(tmp_path / name)
    tag = f"{mode}_{max_speakers}"
    out, out_n, spk = (tmp_path / f"out{tag}.bin", tmp_path / f"out{tag}.i32", tmp_path / f"spk{tag}.i32")
    sel = [f"--max-speakers={max_speakers}", f"--speakers-out={spk}"] if max_speakers else []
    r = subprocess.run([demo, lyra_amd.default_model_dir(), str(tmp_path / "streams.txt"), str(tmp_path / "script.i32"),
                        str(tmp_path / "pk.bin"), str(tmp_path / "len.i32"), str(out), str(out_n), str(mode), "1"] + sel +
                       (["--lanes=26"] if mode == 2 else []), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (mode, r.returncode, r.stderr[-3000:])
    return out.read_bytes(), out_n.read_bytes(), spk.read_bytes() if max_speakers else b""


@pytest.mark.gpu
@pytest.mark.parametrize("N", [0, 3])
def test_bridge_demo_mode_2_equals_mode_0(tmp_path, N):
    ticks, n = 120, 13
    rng = np.random.default_rng(81)
    rates = (3200, 6000, 9200)
    streams = [(rates[s % 3], s % 2) for s in range(n)]
    script = np.zeros((ticks, n, 3), np.int32)
    script[:, :, 0] = (np.arange(n) // 4)[None, :]
    script[70:, :, 0] = rng.integers(-1, 3, n)[None, :]                # the membership changes at tick 70 ...
    assert (script[70, :, 0] != script[69, :, 0]).any(), "mode 2 must run more than one segment"
    script[:, :, 1] = rng.random((ticks, n)) < 0.1                     # ... mutes come and go ...
    script[:, :, 2] = np.array(rates)[rng.integers(0, 3, (ticks, n))]  # ... and bitrates change from tick to tick
    rec = draw_recording(rng, n, ticks)
    tick_by_tick = _demo(tmp_path, 0, streams, script, rec["packets"], rec["sizes"], N)
    whole = _demo(tmp_path, 2, streams, script, rec["packets"], rec["sizes"], N)
    assert len(tick_by_tick[0]) == ticks * n * ROW and len(tick_by_tick[1]) == ticks * n * 4
    lens = np.frombuffer(tick_by_tick[1], np.int32)
    assert (lens == 0).any() and (lens > 0).any()
    assert whole[1] == tick_by_tick[1], "outgoing lengths"
    assert whole[0] == tick_by_tick[0], "outgoing packets"
    assert whole[2] == tick_by_tick[2], "speaker flags"
    if N:
        assert np.frombuffer(whole[2], np.int32).any()
