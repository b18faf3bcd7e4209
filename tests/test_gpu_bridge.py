"""The conference bridge on the device (include/lyra_hip_bridge.h): the mix kernel against the formula, the tick against the
three calls it composes, the tick against the reference model, the two-deep host form against the `_dev` call, bridge_demo, and
the argument checks.  Helpers: tests/bridge_models.py, tests/bridge_tick_cases.py.

Shapes.  lossy_mix and the resampler serve 4 rows per workgroup, the estimators 2, the mix kernel one room per wavefront and 4
per workgroup with member chunks of 8: B = 37 and B = 5 for the tick (the shapes of test_gpu_decode_streams.py), B = 330 with
rooms of 1, 2, 3, 8, 9, 16, 17 and 257 (313 rows; the rest in no room) for the kernel.

Stream kind: the contexts here (32 to 512 streams) run on the CU-masked streams the library picks up to 1,024 streams, which
are blocking streams with respect to the NULL stream; the cases with streams="plain" run on hipStreamNonBlocking streams, the
kind of a 4,096-stream context (tests/gpu_plumbing.py make_ctx)."""
import numpy as np
import pytest

from bridge_models import SKIP_CN, BridgeModel, bridge_kernel_case, np_bridge_mix, np_bridge_plan
from bridge_tick_cases import (SIZES, Bufs, TickKind, begin, begin_end_ticks, compose_case, demo_conference, host_script,
                               rooms_of_six_then_random, run_demo)
from gpu_plumbing import _dev, _ids, _t, make_ctx as _ctx, stream_cases
from receiver_models import _full_batch_mask, _model_packets
from row_cases import _draw_bits, _same_state

EINVAL = -1


def _index(rooms):
    order, start = np_bridge_plan(rooms)
    return order, start


def _dev_index(order, start):
    import torch
    d_order = _t(order) if len(order) else torch.zeros(0, dtype=torch.int32, device=_dev())
    return d_order, _t(start)


# ---- 1. the kernel against the formula ------------------------------------------------------------------------------------

def _mix_dev(a, x, order, start, muted, is_cn):
    """bridge_mix_dev into the first B rows of a buffer with two sentinel rows behind it -> (mix [B][320], sentinel rows)"""
    import torch
    B = x.shape[0]
    buf = torch.full((B + 2, 320), 0x3333, dtype=torch.int16, device=_dev())
    a.bridge_mix_dev(_t(x), *_dev_index(order, start), buf[:B], _t(muted), _t(is_cn))
    a.synchronize()
    out = buf.cpu().numpy()
    return out[:B], out[B:]


@pytest.mark.gpu
def test_mix_kernel_equals_the_formula_and_survives_a_bad_index():
    x, rooms, muted, is_cn = bridge_kernel_case()
    B = x.shape[0]
    order, start = _index(rooms)
    sizes = np.diff(start)
    assert sorted(sizes.tolist()) == [1, 2, 3, 8, 9, 16, 17, 257] and (rooms < 0).any()
    assert (np.diff(order[start[-2]:start[-1]]) > 1).any()               # the last room (label 40) is scattered ...
    perm = order.copy()
    lo, hi = start[-2], start[-1]
    perm[lo:hi] = perm[lo:hi][np.random.default_rng(3).permutation(hi - lo)]   # ... and handed over in permuted order
    want = np_bridge_mix(x, order, start, muted, is_cn)
    assert (want == 32767).any() and (want == -32768).any(), "the case must saturate on both sides"
    assert not want[rooms < 0].any() and not want[rooms == 2].any()      # no room; every member muted: silence
    a = _ctx(512)
    try:
        got, behind = _mix_dev(a, x, perm, start, muted, is_cn)
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, ("rows differ from the formula", bad[:16], rooms[bad[:16]])
        assert (behind == 0x3333).all(), "rows behind the buffer were written"
        assert a.bridge_errors() == 0
        # the same shape with three bad entries: one in a small room, one in the 257-room, one in the scattered room
        broken = perm.copy()
        hit = [int(start[3]), int(start[6]) + 100, int(start[7]) + 5]   # rooms sorted by label: 0..6 then 40
        victims = broken[hit].copy()
        broken[hit] = [-1, B, 2 ** 30]
        got, behind = _mix_dev(a, x, broken, start, muted, is_cn)
        assert (behind == 0x3333).all()
        assert a.bridge_errors(clear=True) == 3 and a.bridge_errors() == 0
        touched = np.isin(rooms, rooms[victims])
        assert np.array_equal(got[~touched], want[~touched]), "rooms with a good index changed"
        # a room that lost a member to a bad entry: that row hears silence and is not heard, the others are the formula without it
        less = rooms.copy()
        less[victims] = -1
        assert np.array_equal(got, np_bridge_mix(x, *_index(less), muted, is_cn))
        # room boundaries outside [0, n_members] are clamped: nothing faults, nothing behind the buffer is written
        wild = start.copy()
        wild[1], wild[-1] = -5, 2 ** 30
        got, behind = _mix_dev(a, x, perm, wild, muted, is_cn)
        assert (behind == 0x3333).all() and a.bridge_errors() == 0
    finally:
        a.close()


# ---- 2. the tick equals its composition -----------------------------------------------------------------------------------

NAMES = ("out sizes", "out packets", "pcm16", "mix", "is_noise", "is_comfort_noise")


def _Bufs(B):
    return Bufs(B, NAMES)


def _tick(a, bufs, ids, pk, sz, rooms, muted, bits, dtx, flags):
    bufs.out.zero_()
    a.bridge_tick_dev(_t(ids), _t(pk), _t(sz), *_dev_index(*_index(rooms)), _t(bits), bufs.out, bufs.out_n, _t(muted), _t(dtx),
                      flags, bufs.pcm16, bufs.mix, bufs.isn, bufs.icn)
    a.synchronize()
    return bufs.read()


def _composed(u, bufs, ids, pk, sz, rooms, muted, bits, dtx, flags):
    """The three calls in a row on the twin: the lossy decode at 16 kHz, a synchronise, the numpy mix, the encode."""
    import torch
    B = ids.size
    bufs.out.zero_()
    u.decode_lossy_mixed_dev(_t(ids), _t(pk), _t(sz), 16000, bufs.pcm16, None, bufs.isn, bufs.icn)
    u.synchronize()
    x, icn = bufs.pcm16.cpu().numpy(), bufs.icn.cpu().numpy()
    mix = np_bridge_mix(x, *_index(rooms), muted, icn if flags & SKIP_CN else None)
    bufs.mix.copy_(torch.from_numpy(mix))
    u.encode_streams_dev(_t(ids), bufs.mix, _t(np.full(B, 16000, np.int32)), _t(bits), bufs.out, bufs.out_n, _t(dtx),
                         _t(np.arange(B, dtype=np.int32) * 320), 320 * B)
    u.synchronize()
    return bufs.read()


class _FullMix(TickKind):
    names = NAMES

    def tick(self, c, a, bufs, pk, sz, rooms):
        return _tick(a, bufs, c.ids, pk, sz, rooms, c.muted, c.bits, c.dtx, c.flags)

    def composed(self, c, u, bufs, pk, sz, rooms):
        return _composed(u, bufs, c.ids, pk, sz, rooms, c.muted, c.bits, c.dtx, c.flags)

    def observe(self, c, t, rooms, got, want):
        if c.flags & SKIP_CN and t < 20:
            plain = np_bridge_mix(want[2], *_index(rooms), c.muted, None)
            c.count["flag"] += int(not np.array_equal(plain[:4], want[3][:4]))

    def verdict(self, c):
        if c.flags & SKIP_CN:
            assert c.count["flag"] >= 1, "SKIP_COMFORT_NOISE never changed the mix of the room with the lost member"


def _compose_case(B, mode="xnnpack", **kw):
    compose_case(_FullMix(), B, mode, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("B,mode,streams", stream_cases([(37, "xnnpack"), (5, "xnnpack"), (37, "builtin_mixed")],
                                                        plain=(37, "xnnpack")))
def test_tick_equals_its_composition(B, mode, streams):
    _compose_case(B, mode, streams=streams)


@pytest.mark.gpu
def test_tick_equals_its_composition_in_serial_order():
    _compose_case(37, serial=True)


@pytest.mark.gpu
def test_tick_equals_its_composition_on_a_split_context():
    _compose_case(37, sub_batches=2)


@pytest.mark.gpu
def test_tick_skips_comfort_noise_rows_when_asked():
    _compose_case(37, flags=SKIP_CN)


@pytest.mark.gpu
def test_tick_with_library_scratch_for_the_optional_outputs():
    """d_pcm16, d_mix and the flags left out (and SKIP_COMFORT_NOISE on, so the library's own flag array is read): the packets
    and the stream state are those of the call that was given every buffer."""
    import torch
    B, ms, T = 37, 64, 24
    rng = np.random.default_rng(5)
    ids = _ids(B, ms, 1)
    mask = _full_batch_mask(T, B, rng)
    rooms = (np.arange(B) // 5).astype(np.int32)
    muted, dtx = np.zeros(B, np.int32), np.ones(B, np.int32)
    a, u = _ctx(ms), _ctx(ms)
    try:
        bufs = _Bufs(B)
        out, out_n = torch.zeros((B, 23), dtype=torch.uint8, device=_dev()), torch.zeros(B, dtype=torch.int32, device=_dev())
        for t in range(T):
            pk = rng.integers(0, 256, (B, 23), dtype=np.uint8)
            sz = (rng.choice(SIZES, B) * mask[t]).astype(np.int32)
            bits = _draw_bits(rng, B)
            want = _tick(u, bufs, ids, pk, sz, rooms, muted, bits, dtx, SKIP_CN)
            out.zero_()
            a.bridge_tick_dev(_t(ids), _t(pk), _t(sz), *_dev_index(*_index(rooms)), _t(bits), out, out_n, None, _t(dtx), SKIP_CN)
            a.synchronize()
            assert np.array_equal(out_n.cpu().numpy(), want[0]) and np.array_equal(out.cpu().numpy(), want[1]), f"tick {t}"
        _same_state(a, u, ids, "after the last tick")
    finally:
        a.close()
        u.close()


# ---- 3. against the reference model ---------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_tick_against_the_reference_model(oracle_default, golden_dir):
    T = 50
    rooms = np.array([0, 0, 0, 1, 1, 2, 3, 3, 3, 3, 3], np.int32)
    B = rooms.size
    muted = np.zeros(B, np.int32)
    muted[2] = 1
    three = (184, 120, 64)
    in_bits = [three[i % 3] for i in range(B)]
    out_bits = np.array([three[(i + 1) % 3] for i in range(B)], np.int32)
    dtx = np.ones(B, np.int32)
    packets, nbytes = _model_packets(oracle_default, golden_dir, in_bits, T)
    rx = np.ones((T, B), bool)
    rx[10:24, 3:5] = False
    rx[5:9, 0] = False
    ids = np.arange(B, dtype=np.int32) + 7
    model = BridgeModel(oracle_default, ids, rooms, muted, out_bits, dtx)
    a = _ctx(32)
    try:
        bufs = [_Bufs(B), _Bufs(B)]
        sat = 0
        empty = np.zeros(B, int)
        for t in range(T):
            sz = (nbytes * rx[t]).astype(np.int32)
            hops, reach, m_mix, m_pk, m_sz, m_cn = model.tick(packets[t], sz)
            # the model's own run must be a hard input
            sat += int((np.abs(m_mix[rooms == 3].astype(np.int32)) >= 32767).sum())
            empty += m_sz == 0
            out_n, out, pcm16, mix, isn, icn = _tick(a, bufs[t & 1], ids, packets[t], sz, rooms, muted, out_bits, dtx, 0)
            for b in range(B):
                model.tally.check(pcm16[b], hops[b], reach[b], f"tick {t}, row {b}, 16 kHz")
            assert np.array_equal(icn, m_cn), f"tick {t}: is_comfort_noise"
            assert np.array_equal(mix, np_bridge_mix(pcm16, *_index(rooms), muted)), f"tick {t}: the mix over the device's own hop"
            want_pk, want_sz = model.encode_of(mix)
            assert np.array_equal(out_n, want_sz), (f"tick {t}: outgoing sizes", out_n, want_sz)
            assert np.array_equal(out, want_pk), f"tick {t}: outgoing packets"
        model.tally.report("bridge d_pcm16")
        print("model: saturated samples in room 3:", sat, "empty packets per row:", empty)
        assert sat >= 1, "no mix sample saturates in room 3"
        in1 = empty[rooms == 1]
        assert (in1 > 0).any() and (in1 < T).all(), "room 1 needs an empty and a non-empty outgoing packet"
        assert empty[5] == T - 1, "row 5, alone in its room, hears silence: empty packets from the second tick on"
    finally:
        a.close()


# ---- 4. bridge_begin / bridge_end equal the `_dev` call -------------------------------------------------------------------

def _host_script(B, T, seed):
    return host_script(B, T, seed, rooms_of_six_then_random(B, T))


@pytest.mark.gpu
@pytest.mark.parametrize("depth,streams", stream_cases([1, 2], plain=2))
def test_begin_end_equal_the_dev_call(depth, streams):
    B, ms, T = 37, 64, 24
    ids = _ids(B, ms, 11)
    script = _host_script(B, T, 21)
    a, u = _ctx(ms, streams=streams), _ctx(ms, streams=streams)
    try:
        bufs = _Bufs(B)
        want = [_tick(u, bufs, ids, s["pk"], s["sz"], s["rooms"], s["muted"], s["bits"], s["dtx"], SKIP_CN) for s in script]
        got = begin_end_ticks(a, script, a.bridge_end, depth, ids, SKIP_CN)
        for t in range(T):
            out, out_n, isn, icn = got[t]
            w = want[t]
            assert np.array_equal(out_n, w[0]) and np.array_equal(out, w[1]), f"tick {t}: packets"
            assert np.array_equal(isn, w[4]) and np.array_equal(icn, w[5]), f"tick {t}: flags"
        _same_state(a, u, ids, "after the last tick")
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
def test_a_larger_tick_begun_behind_one_in_flight():
    """A tick of 5 rows begun while a tick of 2 rows is in flight, on a context of 8 streams: the scratch of both legs grows
    under a tick in flight.  Against the `_dev` call on the twin."""
    ms, sizes = 8, (2, 5)
    a, u = _ctx(ms), _ctx(ms)
    try:
        ids = np.arange(ms, dtype=np.int32)
        ticks = [_host_script(B, 1, 23 + B)[0] for B in sizes]
        for s in ticks:
            s["rooms"][:] = 0   # everybody in one room
        want = [_tick(u, _Bufs(B), ids[:B], s["pk"], s["sz"], s["rooms"], s["muted"], s["bits"], s["dtx"], SKIP_CN)
                for B, s in zip(sizes, ticks)]
        for B, s in zip(sizes, ticks):
            begin(a, s, ids[:B], SKIP_CN)
        for k in range(len(sizes)):
            out, out_n, isn, icn = a.bridge_end()
            w = want[k]
            assert np.array_equal(out_n, w[0]) and np.array_equal(out, w[1]), f"tick {k}: packets"
            assert np.array_equal(isn, w[4]) and np.array_equal(icn, w[5]), f"tick {k}: flags"
        _same_state(a, u, ids, "after the last tick")
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
def test_begin_refusals_enqueue_nothing_and_pipelines_exclude_each_other():
    import lyra_amd
    B, ms = 37, 64
    ids = _ids(B, ms, 12)
    s = _host_script(B, 3, 22)
    a, u = _ctx(ms), _ctx(ms)
    L = a.L
    try:
        for c in (a, u):
            begin(c, s[0], ids)
            c.bridge_end()
        before = a.export_streams(ids)

        def refused(**change):
            k = dict(s[1], ids=ids, flags=0)
            k.update(change)
            with pytest.raises(lyra_amd.codec.LyraHipError):
                a.bridge_begin(k["pk"], k["sz"], k["rooms"], k["bits"], k["muted"], k["dtx"], k["flags"], k["ids"])

        dup = ids.copy(); dup[5] = dup[4]
        far = ids.copy(); far[0] = ms
        bad_sz = s[1]["sz"].copy(); bad_sz[3] = 9
        bad_bits = s[1]["bits"].copy(); bad_bits[7] = 186
        refused(ids=dup)
        refused(ids=far)
        refused(sz=bad_sz)
        refused(bits=bad_bits)
        refused(flags=2)
        with pytest.raises(lyra_amd.codec.LyraHipError):
            a.bridge_end()                                   # nothing in flight
        assert np.array_equal(a.export_streams(ids), before), "a refused begin() changed stream state"
        # a third begin() is refused; the two in flight complete as on the twin
        for t in (1, 2):
            begin(a, s[t], ids)
        refused()
        # ... and so are the other pipelined forms while a tick is in flight, and export / import
        rates = np.full(B, 16000, np.int32)
        with pytest.raises(lyra_amd.codec.LyraHipError, match="bridge"):
            a.decode_streams_begin(s[1]["pk"], s[1]["sz"], rates, ids)
        with pytest.raises(lyra_amd.codec.LyraHipError, match="bridge"):
            a.encode_streams_begin(np.zeros(B * 320, np.int16), rates, s[1]["bits"], None, ids)
        with pytest.raises(lyra_amd.codec.LyraHipError):
            a.export_streams(ids)
        got = [a.bridge_end(), a.bridge_end()]
        bufs = _Bufs(B)
        for t in (1, 2):
            w = _tick(u, bufs, ids, s[t]["pk"], s[t]["sz"], s[t]["rooms"], s[t]["muted"], s[t]["bits"], s[t]["dtx"], 0)
            assert np.array_equal(got[t - 1][1], w[0]) and np.array_equal(got[t - 1][0], w[1]), f"tick {t}"
        _same_state(a, u, ids, "after the refusals")
        # the other direction: a hop of either streams pipeline in flight refuses a tick
        a.decode_streams_begin(s[1]["pk"], s[1]["sz"], rates, ids)
        refused()
        a.decode_streams_end()
        a.encode_streams_begin(np.zeros(B * 320, np.int16), rates, s[1]["bits"], None, ids)
        refused()
        a.encode_streams_end()
        assert L.lyra_hip_bridge_end(a.h, None, None, None, None) == EINVAL
    finally:
        a.close()
        u.close()


# ---- 5. the class, through bridge_demo ------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_bridge_demo_both_modes_equal_begin_end_from_python(tmp_path):
    T, n = 30, 13
    streams, script, packets, lengths = demo_conference(31, T, n, 4, 3)
    blocking = run_demo(tmp_path, 0, streams, script, packets, lengths, True)
    pipelined = run_demo(tmp_path, 1, streams, script, packets, lengths, True)
    assert np.array_equal(blocking[1], pipelined[1]) and np.array_equal(blocking[0], pipelined[0])
    assert (blocking[1] == 0).any() and (blocking[1] > 0).any()
    a = _ctx(n)
    try:
        dtx = np.array([d for _, d in streams], np.int32)
        for t in range(T):
            a.bridge_begin(packets[t], lengths[t], script[t, :, 0], script[t, :, 2] // 50, script[t, :, 1], dtx, SKIP_CN)
            out, out_n, _, _ = a.bridge_end()
            assert np.array_equal(out_n, blocking[1][t]) and np.array_equal(out, blocking[0][t]), f"tick {t}"
    finally:
        a.close()


# ---- 6. argument checks of the `_dev` calls -------------------------------------------------------------------------------

@pytest.mark.gpu
def test_dev_argument_checks_refuse_and_leave_the_context_alone():
    import torch
    from lyra_amd.codec import BridgeTick, C
    B, ms = 12, 32
    ids = _ids(B, ms, 2)
    rng = np.random.default_rng(9)
    rooms = (np.arange(B) // 3).astype(np.int32)
    order, start = _index(rooms)
    muted, dtx = np.zeros(B, np.int32), np.ones(B, np.int32)
    a, u = _ctx(ms), _ctx(ms)
    L = a.L
    try:
        keep = dict(ids=_t(ids), pk=_t(rng.integers(0, 256, (B, 23), dtype=np.uint8)), sz=_t(np.full(B, 23, np.int32)),
                    order=_t(order), start=_t(start), bits=_t(np.full(B, 64, np.int32)),
                    out=torch.zeros((B, 23), dtype=torch.uint8, device=_dev()), out_n=torch.zeros(B, dtype=torch.int32, device=_dev()),
                    x=torch.zeros((B + 1, 320), dtype=torch.int16, device=_dev()), mix=torch.zeros((B + 1, 320), dtype=torch.int16, device=_dev()))
        p = {k: v.data_ptr() for k, v in keep.items()}
        torch.cuda.synchronize()   # (the calls below go to the library directly, without the binding's stream ordering)

        def tick(**change):
            f = dict(d_stream_ids=p["ids"], B=B, d_packets=p["pk"], d_packet_bytes=p["sz"], d_order=p["order"],
                     d_room_start=p["start"], n_rooms=start.size - 1, n_members=order.size, d_muted=None, flags=0,
                     d_num_bits=p["bits"], d_dtx=None, d_out_packets=p["out"], d_out_packet_bytes=p["out_n"], d_pcm16=p["x"],
                     d_mix=p["mix"], d_is_noise=None, d_is_comfort_noise=None)
            f.update(change)
            t = BridgeTick(**f)
            return L.lyra_hip_bridge_tick_dev(a.h, C.addressof(t))

        for change in (dict(d_stream_ids=None), dict(d_packets=None), dict(d_packet_bytes=None), dict(d_num_bits=None),
                       dict(d_out_packets=None), dict(d_out_packet_bytes=None), dict(d_order=None), dict(d_room_start=None),
                       dict(B=0), dict(B=ms + 1), dict(n_rooms=-1), dict(n_rooms=B + 1), dict(n_members=-1),
                       dict(n_members=B + 1), dict(flags=4), dict(d_pcm16=p["x"] + 2), dict(d_mix=p["mix"] + 8),
                       dict(d_mix=p["x"])):
            assert tick(**change) == EINVAL, change
        assert L.lyra_hip_bridge_tick_dev(a.h, None) == EINVAL

        def mix(x=p["x"], n=B, o=p["order"], s=p["start"], nr=start.size - 1, nm=order.size, out=p["mix"]):
            return L.lyra_hip_bridge_mix_dev(a.h, x, n, o, s, nr, nm, None, None, out)

        for kw in (dict(x=None), dict(out=None), dict(o=None), dict(s=None), dict(n=0), dict(n=ms + 1), dict(nr=-1),
                   dict(nr=B + 1), dict(nm=B + 1), dict(x=p["x"] + 2), dict(out=p["mix"] + 4), dict(out=p["x"])):
            assert mix(**kw) == EINVAL, kw
        assert mix() == 0 and mix(nr=0, nm=0, o=None, s=None) == 0      # an empty index is a valid one: everybody hears silence
        a.synchronize()
        assert not keep["mix"][:B].cpu().numpy().any()
        # a valid tick now matches a twin that never saw a bad call
        ba, bu = _Bufs(B), _Bufs(B)
        pk = rng.integers(0, 256, (B, 23), dtype=np.uint8)
        for t in range(3):
            args = (ids, pk, np.full(B, 15, np.int32), rooms, muted, np.full(B, 120, np.int32), dtx, 0)
            got, want = _tick(a, ba, *args), _tick(u, bu, *args)
            for name, g, w in zip(NAMES, got, want):
                assert np.array_equal(g, w), (t, name)
        _same_state(a, u, ids, "after the refused calls")
    finally:
        a.close()
        u.close()
