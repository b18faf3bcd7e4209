"""The conference bridge with loudest-N selection on the device (include/lyra_hip_speakers.h): the three kernels against the
formula, the equivalence with the full mix where nobody is left out, the tick against the three calls it composes, the two-deep
host form against the `_dev` call, bridge_demo --max-speakers, and the argument checks.  Helpers: tests/speaker_models.py,
tests/bridge_tick_cases.py.

Shapes.  The level kernel serves 4 rows per workgroup, the select kernel one room per wavefront (keys in registers up to 64
members, in memory above), the mix kernel 8 positions per wavefront and 32 per workgroup: B = 330 with rooms of 1, 2, 3, 8, 9,
16, 17 and 257, and again with rooms of 63, 64, 65 and 129, for the kernels; B = 37 and B = 5 for the tick.

Stream kind: the contexts here (up to 512 streams) run on the CU-masked streams the library picks up to 1,024 streams, which
are blocking streams with respect to the NULL stream; the cases with streams="plain" run on hipStreamNonBlocking streams, the
kind of a 4,096-stream context (tests/gpu_plumbing.py make_ctx)."""
import numpy as np
import pytest

from bridge_models import np_bridge_mix, np_bridge_plan
from bridge_tick_cases import (SIZES, Bufs, TickKind, begin, begin_end_ticks, compose_case, demo_conference, host_script,
                               rooms_redrawn_every_fourth_tick, run_demo)
from gpu_plumbing import _dev, _ids, _t, make_ctx as _ctx, stream_cases
from receiver_models import _full_batch_mask
from row_cases import _draw_bits, _same_state
from speaker_models import SKIP_CN, np_levels, np_speakers_mix, speakers_kernel_case, threshold_case

EINVAL = -1
MIX_FILL, LEVEL_FILL, FLAG_FILL = 0x3333, 0x5555555555555555, 0x77777777


# ---- 1. the kernels against the formula -----------------------------------------------------------------------------------

def _mix_dev(a, x, order, start, N, muted, is_cn):
    """speakers_mix_dev into the first B rows / words of buffers with sentinels behind them -> (mix, levels, is_speaker)"""
    import torch
    B = x.shape[0]
    mix = torch.full((B + 2, 320), MIX_FILL, dtype=torch.int16, device=_dev())
    levels = torch.full((B + 3,), LEVEL_FILL, dtype=torch.int64, device=_dev())
    flags = torch.full((B + 3,), FLAG_FILL, dtype=torch.int32, device=_dev())
    a.speakers_mix_dev(_t(x), _t(order), _t(start), mix[:B], N, _t(muted), None if is_cn is None else _t(is_cn),
                       levels[:B], flags[:B])
    a.synchronize()
    mix, levels, flags = mix.cpu().numpy(), levels.cpu().numpy(), flags.cpu().numpy()
    assert (mix[B:] == MIX_FILL).all(), "rows behind the mix were written"
    assert (levels[B:] == LEVEL_FILL).all() and (flags[B:] == FLAG_FILL).all(), "words behind the levels / flags were written"
    return mix[:B], levels[:B], flags[:B]


def _check(got, want, rooms, what):
    mix, levels, flags = got
    assert np.array_equal(levels, want[1]), (what, "levels differ in rows", np.flatnonzero(levels != want[1])[:16])
    bad = np.flatnonzero(flags != want[2])
    assert bad.size == 0, (what, "is_speaker differs in rows", bad[:16], rooms[bad[:16]])
    bad = np.flatnonzero((mix != want[0]).any(axis=1))
    assert bad.size == 0, (what, "mix rows differ from the formula", bad[:16], rooms[bad[:16]])


@pytest.fixture(scope="module")
def kernel_case():
    return speakers_kernel_case()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 3, 8])
def test_kernels_equal_the_formula_and_survive_a_bad_index(kernel_case, N):
    x, rooms, muted, is_cn, order, start = kernel_case
    B = x.shape[0]
    want = np_speakers_mix(x, order, start, N, muted, is_cn)
    assert want[1].max() == 320 * 2 ** 30
    a = _ctx(512)
    try:
        _check(_mix_dev(a, x, order, start, N, muted, is_cn), want, rooms, f"N = {N}")
        assert a.bridge_errors() == 0
        # three bad entries: one in a small room, one in the 257-room, one in the scattered room -- counted once each, although
        # two kernels read the index
        broken = order.copy()
        hit = [int(start[3]), int(start[6]) + 100, int(start[7]) + 5]   # rooms sorted by label: 0..6 then 40
        victims = broken[hit].copy()
        broken[hit] = [-1, B, 2 ** 30]
        got = _mix_dev(a, x, broken, start, N, muted, is_cn)
        assert a.bridge_errors(clear=True) == 3 and a.bridge_errors() == 0
        touched = np.isin(rooms, rooms[victims])
        assert np.array_equal(got[0][~touched], want[0][~touched]) and np.array_equal(got[2][~touched], want[2][~touched]), \
            "rooms with a good index changed"
        # the model with those rows in no room: the index without the bad entries (the other positions keep their order)
        keep = np.ones(order.size, bool)
        keep[hit] = False
        less_start = np.array([keep[:s].sum() for s in start], np.int32)
        _check(got, np_speakers_mix(x, order[keep], less_start, N, muted, is_cn), rooms, f"N = {N}, bad entries")
        # room boundaries outside [0, n_members] are clamped: nothing faults, nothing behind the buffers is written
        wild = start.copy()
        wild[1], wild[-1] = -5, 2 ** 30
        got = _mix_dev(a, x, order, wild, N, muted, is_cn)
        assert np.array_equal(got[1], want[1]) and a.bridge_errors() == 0
    finally:
        a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 3, 8])
def test_kernels_at_the_room_sizes_around_64(N):
    x, rooms, muted, order, start = threshold_case()
    assert np.diff(start).tolist() == [63, 64, 65, 129]
    a = _ctx(512)
    try:
        _check(_mix_dev(a, x, order, start, N, muted, None), np_speakers_mix(x, order, start, N, muted), rooms, f"N = {N}")
        assert a.bridge_errors() == 0
    finally:
        a.close()


# ---- 2. nobody left out: the full mix, bit for bit ------------------------------------------------------------------------

@pytest.mark.gpu
def test_with_at_most_eight_candidates_per_room_it_is_the_full_mix(kernel_case):
    import torch
    x, rooms, muted, is_cn, _, _ = kernel_case
    small = np.where(np.isin(rooms, (0, 1, 2, 3)), rooms, -1).astype(np.int32)      # rooms of 1, 2, 3 and 8 ...
    rest = np.flatnonzero(small < 0)
    small[rest] = 10 + np.arange(rest.size) // 8                                      # ... and the other rows in rooms of 8
    order, start = np_bridge_plan(small)
    assert np.diff(start).max() == 8
    B = x.shape[0]
    a = _ctx(512)
    try:
        got = _mix_dev(a, x, order, start, 8, muted, is_cn)
        full = torch.zeros((B, 320), dtype=torch.int16, device=_dev())
        a.bridge_mix_dev(_t(x), _t(order), _t(start), full, _t(muted), _t(is_cn))
        a.synchronize()
        assert np.array_equal(got[0], full.cpu().numpy())
        assert np.array_equal(got[0], np_bridge_mix(x, order, start, muted, is_cn))
    finally:
        a.close()


# ---- 3. the tick equals its composition -----------------------------------------------------------------------------------

NAMES = ("out sizes", "out packets", "pcm16", "mix", "is_noise", "is_comfort_noise", "levels", "is_speaker")


def _Bufs(B):
    return Bufs(B, NAMES)


def _tick(a, bufs, ids, pk, sz, rooms, muted, bits, dtx, flags, N):
    bufs.out.zero_()
    a.speakers_tick_dev(_t(ids), _t(pk), _t(sz), *map(_t, np_bridge_plan(rooms)), _t(bits), bufs.out, bufs.out_n, N,
                        _t(muted), _t(dtx), flags, bufs.pcm16, bufs.mix, bufs.isn, bufs.icn, bufs.levels, bufs.spk)
    a.synchronize()
    return bufs.read()


def _composed(u, bufs, ids, pk, sz, rooms, muted, bits, dtx, flags, N):
    """The three calls in a row on the twin: the lossy decode at 16 kHz, a synchronise, the numpy selection mix, the encode."""
    import torch
    B = ids.size
    bufs.out.zero_()
    u.decode_lossy_mixed_dev(_t(ids), _t(pk), _t(sz), 16000, bufs.pcm16, None, bufs.isn, bufs.icn)
    u.synchronize()
    x, icn = bufs.pcm16.cpu().numpy(), bufs.icn.cpu().numpy()
    mix, levels, spk = np_speakers_mix(x, *np_bridge_plan(rooms), N, muted, icn if flags & SKIP_CN else None)
    bufs.mix.copy_(torch.from_numpy(mix))
    bufs.levels.copy_(torch.from_numpy(levels))
    bufs.spk.copy_(torch.from_numpy(spk))
    u.encode_streams_dev(_t(ids), bufs.mix, _t(np.full(B, 16000, np.int32)), _t(bits), bufs.out, bufs.out_n, _t(dtx),
                         _t(np.arange(B, dtype=np.int32) * 320), 320 * B)
    u.synchronize()
    return bufs.read()


class _Selection(TickKind):
    names = NAMES

    def prepare(self, c, rng):
        if c.flags & SKIP_CN:
            c.muted[2:4] = 1        # ... and one of the room's two sources: a speaker (N = 2) unless the flag takes it out

    def tick(self, c, a, bufs, pk, sz, rooms):
        return _tick(a, bufs, c.ids, pk, sz, rooms, c.muted, c.bits, c.dtx, c.flags, c.N)

    def composed(self, c, u, bufs, pk, sz, rooms):
        return _composed(u, bufs, c.ids, pk, sz, rooms, c.muted, c.bits, c.dtx, c.flags, c.N)

    def observe(self, c, t, rooms, got, want):
        index = np_bridge_plan(rooms)
        c.count["selection"] += int(not np.array_equal(np_bridge_mix(want[2], *index, c.muted,
                                                                     want[5] if c.flags & SKIP_CN else None), want[3]))
        if c.flags & SKIP_CN and t < 20:
            _, _, plain = np_speakers_mix(want[2], *index, c.N, c.muted, None)
            c.count["flag"] += int(plain[1] == 1 and want[7][1] == 0)     # the lost row stops being a speaker

    def verdict(self, c):
        assert c.count["selection"] >= 1, "the selection never changed the mix"
        if c.flags & SKIP_CN:
            assert c.count["flag"] >= 1, "SKIP_COMFORT_NOISE never took the lost row off the speaker list"


def _compose_case(B, mode="xnnpack", N=2, **kw):
    compose_case(_Selection(), B, mode, N=N, **kw)


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
def test_tick_takes_comfort_noise_rows_off_the_speaker_list_when_asked():
    _compose_case(37, flags=SKIP_CN)


# ---- 4. library scratch ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_tick_with_library_scratch_for_the_optional_outputs():
    import torch
    B, ms, T, N = 37, 64, 12, 2
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
            want = _tick(u, bufs, ids, pk, sz, rooms, muted, bits, dtx, SKIP_CN, N)
            out.zero_()
            a.speakers_tick_dev(_t(ids), _t(pk), _t(sz), *map(_t, np_bridge_plan(rooms)), _t(bits), out, out_n, N, None,
                                _t(dtx), SKIP_CN)
            a.synchronize()
            assert np.array_equal(out_n.cpu().numpy(), want[0]) and np.array_equal(out.cpu().numpy(), want[1]), f"tick {t}"
        _same_state(a, u, ids, "after the last tick")
    finally:
        a.close()
        u.close()


# ---- 5. speakers_begin / speakers_end equal the `_dev` call ---------------------------------------------------------------

def _host_script(B, T, seed):
    return host_script(B, T, seed, rooms_redrawn_every_fourth_tick(B))


def _begin(c, s, N, ids, flags=0):
    begin(c, s, ids, flags, N)


@pytest.mark.gpu
@pytest.mark.parametrize("depth,streams", stream_cases([1, 2], plain=2))
def test_begin_end_equal_the_dev_call(depth, streams):
    B, ms, T, N = 37, 64, 16, 3
    ids = _ids(B, ms, 11)
    script = _host_script(B, T, 21)
    a, u = _ctx(ms, streams=streams), _ctx(ms, streams=streams)
    try:
        bufs = _Bufs(B)
        want = [_tick(u, bufs, ids, s["pk"], s["sz"], s["rooms"], s["muted"], s["bits"], s["dtx"], SKIP_CN, N) for s in script]
        got = begin_end_ticks(a, script, a.speakers_end, depth, ids, SKIP_CN, N)
        for t in range(T):
            out, out_n, isn, icn, levels, spk = got[t]
            w = want[t]
            assert np.array_equal(out_n, w[0]) and np.array_equal(out, w[1]), f"tick {t}: packets"
            assert np.array_equal(isn, w[4]) and np.array_equal(icn, w[5]), f"tick {t}: flags"
            assert np.array_equal(levels, w[6]) and np.array_equal(spk, w[7]), f"tick {t}: levels and speaker flags"
            assert np.array_equal(levels, np_levels(w[2]))
        _same_state(a, u, ids, "after the last tick")
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
def test_begin_refusals_enqueue_nothing_and_the_two_kinds_of_tick_share_one_queue():
    import lyra_amd
    Err = lyra_amd.codec.LyraHipError
    B, ms, N = 37, 64, 3
    ids = _ids(B, ms, 12)
    s = _host_script(B, 4, 22)
    a, u = _ctx(ms), _ctx(ms)
    L = a.L
    try:
        for c in (a, u):
            _begin(c, s[0], N, ids)
            c.speakers_end()
        before = a.export_streams(ids)
        for bad in (0, 9, -1):
            with pytest.raises(Err, match="max_speakers"):
                _begin(a, s[1], bad, ids)
        with pytest.raises(Err):
            a.speakers_end()                                 # nothing in flight
        assert np.array_equal(a.export_streams(ids), before), "a refused begin() changed stream state"
        # one queue of two for both kinds: a selection tick, then a full-mix tick; a third of either kind is refused
        _begin(a, s[1], N, ids)
        begin(a, s[2], ids)
        with pytest.raises(Err):
            _begin(a, s[3], N, ids)
        with pytest.raises(Err):
            begin(a, s[3], ids)
        # the other pipelined forms, export / import: refused while a tick is in flight
        rates = np.full(B, 16000, np.int32)
        with pytest.raises(Err):
            a.decode_streams_begin(s[1]["pk"], s[1]["sz"], rates, ids)
        with pytest.raises(Err):
            a.encode_streams_begin(np.zeros(B * 320, np.int16), rates, s[1]["bits"], None, ids)
        with pytest.raises(Err):
            a.export_streams(ids)
        # the oldest tick is a selection tick: the full-mix end() is refused and consumes nothing
        with pytest.raises(Err, match="speakers_begin"):
            a.bridge_end()
        got1 = a.speakers_end()
        with pytest.raises(Err, match="oldest tick"):
            a.speakers_end()                                 # ... and the reverse
        got2 = a.bridge_end()
        bufs = _Bufs(B)
        w1 = _tick(u, bufs, ids, s[1]["pk"], s[1]["sz"], s[1]["rooms"], s[1]["muted"], s[1]["bits"], s[1]["dtx"], 0, N)
        assert np.array_equal(got1[1], w1[0]) and np.array_equal(got1[0], w1[1]) and np.array_equal(got1[5], w1[7])
        begin(u, s[2], ids)
        w2 = u.bridge_end()
        assert np.array_equal(got2[1], w2[1]) and np.array_equal(got2[0], w2[0])
        _same_state(a, u, ids, "after the refusals")
        # the other direction: a hop of either streams pipeline in flight refuses a tick
        a.decode_streams_begin(s[1]["pk"], s[1]["sz"], rates, ids)
        with pytest.raises(Err):
            _begin(a, s[1], N, ids)
        a.decode_streams_end()
        a.encode_streams_begin(np.zeros(B * 320, np.int16), rates, s[1]["bits"], None, ids)
        with pytest.raises(Err):
            _begin(a, s[1], N, ids)
        a.encode_streams_end()
        assert L.lyra_hip_speakers_end(a.h, None, None, None, None, None, None) == EINVAL
    finally:
        a.close()
        u.close()


# ---- 6. argument checks of the `_dev` calls -------------------------------------------------------------------------------

@pytest.mark.gpu
def test_dev_argument_checks_refuse_and_leave_the_context_alone():
    import torch
    from lyra_amd.codec import C, SpeakersTick
    B, ms, N = 12, 32, 2
    ids = _ids(B, ms, 2)
    rng = np.random.default_rng(9)
    rooms = (np.arange(B) // 4).astype(np.int32)
    order, start = np_bridge_plan(rooms)
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
                     d_mix=p["mix"], d_is_noise=None, d_is_comfort_noise=None, max_speakers=N, d_levels=None, d_is_speaker=None)
            f.update(change)
            t = SpeakersTick(**f)
            return L.lyra_hip_speakers_tick_dev(a.h, C.addressof(t))

        for change in (dict(d_stream_ids=None), dict(d_packets=None), dict(d_packet_bytes=None), dict(d_num_bits=None),
                       dict(d_out_packets=None), dict(d_out_packet_bytes=None), dict(d_order=None), dict(d_room_start=None),
                       dict(B=0), dict(B=ms + 1), dict(n_rooms=-1), dict(n_rooms=B + 1), dict(n_members=-1),
                       dict(n_members=B + 1), dict(flags=4), dict(d_pcm16=p["x"] + 2), dict(d_mix=p["mix"] + 8),
                       dict(d_mix=p["x"]), dict(max_speakers=0), dict(max_speakers=9), dict(max_speakers=-1)):
            assert tick(**change) == EINVAL, change
        assert L.lyra_hip_speakers_tick_dev(a.h, None) == EINVAL

        def mix(x=p["x"], n=B, o=p["order"], s=p["start"], nr=start.size - 1, nm=order.size, out=p["mix"], k=N):
            return L.lyra_hip_speakers_mix_dev(a.h, x, n, o, s, nr, nm, None, None, k, out, None, None)

        for kw in (dict(x=None), dict(out=None), dict(o=None), dict(s=None), dict(n=0), dict(n=ms + 1), dict(nr=-1),
                   dict(nr=B + 1), dict(nm=B + 1), dict(x=p["x"] + 2), dict(out=p["mix"] + 4), dict(out=p["x"]), dict(k=0),
                   dict(k=9), dict(k=-1)):
            assert mix(**kw) == EINVAL, kw
        keep["mix"].fill_(7)
        torch.cuda.synchronize()
        assert mix() == 0 and mix(nr=0, nm=0, o=None, s=None) == 0      # an empty index is a valid one: everybody hears silence
        a.synchronize()
        got = keep["mix"].cpu().numpy()
        assert not got[:B].any() and (got[B] == 7).all()
        # a valid tick now matches a twin that never saw a bad call
        ba, bu = _Bufs(B), _Bufs(B)
        pk = rng.integers(0, 256, (B, 23), dtype=np.uint8)
        for t in range(3):
            args = (ids, pk, np.full(B, 15, np.int32), rooms, muted, np.full(B, 120, np.int32), dtx, 0, N)
            got, want = _tick(a, ba, *args), _tick(u, bu, *args)
            for name, g, w in zip(NAMES, got, want):
                assert np.array_equal(g, w), (t, name)
        _same_state(a, u, ids, "after the refused calls")
    finally:
        a.close()
        u.close()


# ---- 7. the class, through bridge_demo --max-speakers ---------------------------------------------------------------------

def _run_demo(tmp_path, mode, streams, script, packets, lengths, skip_cn, N):
    return run_demo(tmp_path, mode, streams, script, packets, lengths, skip_cn, (f"--max-speakers={N}",),
                    (("--speakers-out", "spk.i32"),))


@pytest.mark.gpu
def test_bridge_demo_with_max_speakers_equals_begin_end_from_python(tmp_path):
    T, n, N = 30, 13, 3
    streams, script, packets, lengths = demo_conference(31, T, n, 6, 2)
    blocking = _run_demo(tmp_path, 0, streams, script, packets, lengths, True, N)
    pipelined = _run_demo(tmp_path, 1, streams, script, packets, lengths, True, N)
    for b, p in zip(blocking, pipelined):
        assert np.array_equal(b, p)
    a = _ctx(n)
    try:
        dtx = np.array([d for _, d in streams], np.int32)
        left_out = 0
        for t in range(T):
            a.speakers_begin(packets[t], lengths[t], script[t, :, 0], script[t, :, 2] // 50, N, script[t, :, 1], dtx, SKIP_CN)
            out, out_n, _, _, levels, spk = a.speakers_end()
            assert np.array_equal(out_n, blocking[1][t]) and np.array_equal(out, blocking[0][t]), f"tick {t}"
            assert np.array_equal(spk, blocking[2][t]), f"tick {t}: speaker flags"
            left_out += int(((levels > 0) & (spk == 0) & (script[t, :, 0] >= 0) & (script[t, :, 1] == 0)).sum())
        assert blocking[2].any() and left_out >= 1, "the selection never left a talker out"
    finally:
        a.close()
