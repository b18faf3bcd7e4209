"""lyra_hip_decode_samples_streams_dev: DecodeSamples(n) on the device with a sample rate and a request size per stream in one
call.  Expectations: the reference model (RefLyraDecoder through receiver_models' Tally / CnReach, that module's bounds and none
of its own) and, bit for bit, lyra_hip_decode_samples_any_dev called once per (rate, size) class on a twin context: samples,
flags and the exported stream state.

Stream kind: the contexts here (64 to 512 streams) run on the CU-masked streams the library picks up to 1,024 streams, which
are blocking streams with respect to the NULL stream; the test named "on_plain_streams" runs on hipStreamNonBlocking streams,
the kind of a 4,096-stream context (tests/gpu_plumbing.py make_ctx)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from gpu_plumbing import make_ctx
from receiver_models import ROW, _model_packets as _packets
from receiver_models_any import DeviceAny
from receiver_models_streams import CANARY, STRIDE, DeviceStreams, ModelStreams, batch_rounds, packed, rounds, uniform_by_class

pytestmark = pytest.mark.gpu

# the lists of tests/test_gpu_decode_samples_any.py
SIZES = {48000: [128, 1024, 441, 1, 2, 0, 960, 3840, 959], 32000: [128, 1, 641, 2560, 75], 8000: [128, 161, 640, 1],
         16000: [321, 1024, 1280, 7]}
IDS = np.array([6, 1, 30, 14, 77, 3, 52, 9], np.int32)
RATES = np.array([48000, 48000, 32000, 32000, 8000, 8000, 16000, 16000], np.int32)
BITS = [64, 120, 184, 120, 184, 64, 120, 184]
SHIFT = [3, 0, 0, 2, 0, 2, 0, 1]          # where in its rate's list each stream starts: sizes differ within a call
TICKS, PACKETS = 24, 52
NAMES = ("pcm", "is_noise", "is_comfort_noise")


def _lost(s, t):
    """the first stream of each rate loses 12 hops (into comfort noise and back), stream 1 every fifth"""
    return 3 <= t < 15 if s % 2 == 0 else (s == 1 and t % 5 == 2)


@pytest.fixture(scope="module")
def session(golden_dir, oracle_default):
    """-> list of (tick, rows [8][23], packet bytes [8], sizes [8]): TICKS calls whose sizes cycle through each rate's list.  A
    call carries at most one packet per stream: a stream gets its next one when its own playout time asks for it, so a stream
    whose request was several hops long runs ahead of its packets and conceals, as a receiver that under-runs does."""
    rows, size = _packets(oracle_default, golden_dir, BITS, PACKETS, offset=555)
    played, sent, calls = np.zeros(8, np.int64), np.zeros(8, np.int64), []
    for c in range(TICKS):
        sizes = np.array([SIZES[r][(c + SHIFT[s]) % len(SIZES[r])] for s, r in enumerate(RATES)], np.int32)
        more = sent < np.minimum(played * 50 // RATES + 1, PACKETS)
        nb = np.array([size[s] if more[s] and not _lost(s, sent[s]) else 0 for s in range(8)], np.int32)
        pk = np.stack([rows[min(sent[s], PACKETS - 1), s] for s in range(8)])
        sent += more
        calls.append((c, pk, nb, sizes))
        played += sizes
    return calls


def _same(got, want, where):
    for g, w, what in zip(got, want, NAMES):
        for r in range(len(g)):
            assert np.array_equal(g[r], w[r]), f"{where}: {what} of row {r}"


def test_against_the_reference_model(session, oracle_default):
    model = ModelStreams(oracle_default, IDS, RATES)
    ctx = make_ctx(256)
    spread = 0
    try:
        devc = DeviceStreams(ctx, IDS, RATES)
        for k, (c, pk, nb, sizes) in enumerate(session):
            got = devc.call(pk, nb, sizes)
            before = [list(m.saw_rounds) for m in model.models.values()]
            model.call(f"call {k} (tick {c})", IDS, pk, nb, sizes, got)
            seen = {j for m, b in zip(model.models.values(), before) for j in range(5) if m.saw_rounds[j] > b[j]}
            spread = max(spread, len(seen))
            if k % 8 == 7:
                model.check_estimates(ctx, f"call {k}")
        model.check_estimates(ctx, "end")
        assert ctx.decode_samples_errors() == model.dropped and ctx.rates_errors() == 0
    finally:
        ctx.close()
    ms = model.models
    for r, m in ms.items():
        m.tally.report(f"decode_samples_streams {r} Hz")
        print(r, "rounds", m.saw_rounds, "leftover", m.saw_left, "from the leftover alone", m.saw_left_only)
        assert m.saw_cn and m.saw_back and m.saw_mix, f"{r} Hz: comfort noise {m.saw_cn}, back {m.saw_back}, cross-fade {m.saw_mix}"
        top = {48000: 2, 32000: 1, 16000: 0, 8000: 0}[r]
        assert all(m.saw_left[j] > 0 for j in range(top + 1)) and not any(m.saw_left[top + 1:]), (r, m.saw_left)
    # (no size of the copied lists maps to 641 .. 960 internal samples, so no row needs exactly three rounds;
    # test_ragged_edges has such rows: 2001 samples at 48 kHz)
    assert all(sum(m.saw_rounds[j] for m in ms.values()) > 0 for j in (0, 1, 2, 4)), [m.saw_rounds for m in ms.values()]
    assert spread >= 4, f"at most {spread} different round counts inside one call"
    assert sum(m.saw_left_only for m in ms.values()) > 0
    assert len(session) == TICKS <= 30


def test_bit_for_bit_against_the_uniform_call(session):
    """The session on a second context as one decode_samples_any_dev call per (rate, size) class; half-way rows 1 and 5 are
    served by the uniform call on the FIRST context too, for five calls, and come back."""
    _uniform_call_case(session, None)


def test_bit_for_bit_against_the_uniform_call_on_plain_streams(session):
    """The same on hipStreamNonBlocking streams, the kind a 4,096-stream context runs on (gpu_plumbing.make_ctx)."""
    _uniform_call_case(session, "plain")


def _uniform_call_case(session, streams):
    a, b = make_ctx(128, streams=streams), make_ctx(128, streams=streams)
    sw = np.array([1, 5])
    keep = np.setdiff1d(np.arange(8), sw)
    half = len(session) // 2
    try:
        full, rest = DeviceStreams(a, IDS, RATES), DeviceStreams(a, IDS[keep], RATES[keep])
        for k, (c, pk, nb, sizes) in enumerate(session):
            want = uniform_by_class(b, IDS, RATES, pk, nb, sizes)
            if half <= k < half + 5:
                x = rest.call(pk[keep], nb[keep], sizes[keep])
                y = uniform_by_class(a, IDS[sw], RATES[sw], pk[sw], nb[sw], sizes[sw])
                got = ([None] * 8, np.zeros(8, np.int32), np.zeros(8, np.int32))
                for part, sel in ((x, keep), (y, sw)):
                    for j, s in enumerate(sel):
                        got[0][s], got[1][s], got[2][s] = part[0][j], part[1][j], part[2][j]
            else:
                got = full.call(pk, nb, sizes)
            _same(got, want, f"call {k} (tick {c})")
        assert np.array_equal(a.export_streams(IDS), b.export_streams(IDS))
        assert a.decode_samples_errors() == b.decode_samples_errors() and a.rates_errors() == 0
    finally:
        a.close(); b.close()


def test_uniform_arguments_are_the_old_call():
    """Every row at 48 kHz with one size: without offsets (rows DSS_ROW_STRIDE apart) and in the dense [B][n] layout."""
    rate, B = 48000, 6
    rng = np.random.default_rng(11)
    ids = rng.permutation(64)[:B].astype(np.int32)
    rates = np.full(B, rate, np.int32)
    a, d, b = make_ctx(64), make_ctx(64), make_ctx(64)
    try:
        strided, dense, old = DeviceStreams(a, ids, rates), DeviceStreams(d, ids, rates), DeviceAny(b, ids, rate)
        for n in (961, 2, 3840):
            pk = rng.integers(0, 256, size=(B, ROW)).astype(np.uint8)
            nb = rng.choice([0, 8, 15, 23], size=B).astype(np.int32)
            want = old.call(pk, nb, n)
            hops = rounds(n, rate)
            assert hops == {961: 2, 2: 1, 3840: 4}[n]
            _same(strided.call(pk, nb, np.full(B, n), offsets=None, max_hops=hops), want, f"n {n}, no offsets")
            assert np.array_equal(strided.offs, np.arange(B) * STRIDE)
            _same(dense.call(pk, nb, np.full(B, n), offsets=np.arange(B) * n, max_hops=hops), want, f"n {n}, dense")
            assert np.array_equal(dense.last.reshape(B, n), want[0])
        blob = b.export_streams(ids)
        assert np.array_equal(a.export_streams(ids), blob) and np.array_equal(d.export_streams(ids), blob)
    finally:
        a.close(); d.close(); b.close()


def test_invalid_rows():
    B = 8
    rng = np.random.default_rng(3)
    ids = np.array([5, 60, 17, 2, 33, 8, 41, 20], np.int32)
    rates = np.array([48000, 48000, 32000, 48000, 8000, 16000, 48000, 16000], np.int32)
    pk = rng.integers(0, 256, size=(3, B, ROW)).astype(np.uint8)
    nb = np.full(B, 23, np.int32)
    a, b = make_ctx(64), make_ctx(64)
    try:
        da, db = DeviceStreams(a, ids, rates), DeviceStreams(b, ids, rates)
        for t in range(2):                                   # every stream mid-hop, the 48 kHz ones holding a leftover
            _same(da.call(pk[t], nb, np.full(B, 128)), db.call(pk[t], nb, np.full(B, 128)), f"warm-up {t}")
        before = a.export_streams(ids)
        bad_rates = rates.copy()
        bad_rates[1] = 44100
        sizes = np.array([441, 441, 4 * 640 + 1, 961, 160, 100, 128, 320], np.int32)
        n_pcm = 6000
        offs = np.array([0, 500, 1000, 1500, 2600, -1, n_pcm - 127, 3000], np.int64)
        valid = np.array([0, 4, 7])
        invalid = np.setdiff1d(np.arange(B), valid)
        got = da.call(pk[2], nb, sizes, offsets=offs, max_hops=1, n_pcm=n_pcm, rates=bad_rates, buffer_samples=n_pcm + 64)
        assert a.rates_errors() == invalid.size and a.decode_samples_errors() == 0
        want_buf = np.full(n_pcm + 64, CANARY, np.int16)
        sub = DeviceStreams(b, ids[valid], rates[valid])
        want = sub.call(pk[2][valid], nb[valid], sizes[valid], offsets=offs[valid], max_hops=1, n_pcm=n_pcm,
                        buffer_samples=n_pcm + 64)
        for j, r in enumerate(valid):
            want_buf[offs[r]:offs[r] + sizes[r]] = want[0][j]
            for x, y, what in zip(got, want, NAMES):
                assert np.array_equal(x[r], y[j]), f"valid row {r}: {what}"
        assert np.array_equal(da.last, want_buf), "the buffer changed outside the valid rows (or inside them)"
        after = a.export_streams(ids)
        assert np.array_equal(after[invalid], before[invalid]), "an invalid row's state changed although its packet was refused"
        # the flags of the invalid rows: those of a request of 0 samples without a packet, which changes nothing either
        zero = DeviceStreams(b, ids[invalid], rates[invalid]).call(pk[2][invalid], np.zeros(invalid.size, np.int32),
                                                                   np.zeros(invalid.size, np.int32))
        assert np.array_equal(got[1][invalid], zero[1]) and np.array_equal(got[2][invalid], zero[2])
        assert np.array_equal(after, b.export_streams(ids))
        assert b.rates_errors() == 0
        # argument errors: nothing enqueued
        from lyra_amd.codec import LyraHipError
        for hops in (0, 5):
            with pytest.raises(LyraHipError):
                da.call(pk[2], nb, sizes, max_hops=hops)
        with pytest.raises(LyraHipError):
            da.call(pk[2], nb, sizes, n_pcm=-1, buffer_samples=8000)
        assert np.array_equal(a.export_streams(ids), after)
    finally:
        a.close(); b.close()


def test_ragged_edges():
    """B = 261: two plan workgroups of 256 rows, a last splice workgroup of one row; rates and odd sizes per row, packed."""
    B = 261
    rng = np.random.default_rng(7)
    ids = rng.permutation(300)[:B].astype(np.int32)
    rates = rng.choice([8000, 16000, 32000, 48000], size=B).astype(np.int32)
    choice = {48000: [441, 1, 2001], 32000: [75, 641, 0], 8000: [161, 1, 640], 16000: [7, 321, 1280]}
    a, b = make_ctx(512), make_ctx(512)
    try:
        da = DeviceStreams(a, ids, rates)
        for c in range(3):
            sizes = np.array([choice[int(r)][rng.integers(3)] for r in rates], np.int32)
            pk = rng.integers(0, 256, size=(B, ROW)).astype(np.uint8)
            nb = rng.choice([0, 8, 15, 23, 23], size=B).astype(np.int32)
            got = da.call(pk, nb, sizes)
            assert da.last.size == max(1, int(sizes.sum())) and not (da.last == CANARY).all()
            _same(got, uniform_by_class(b, ids, rates, pk, nb, sizes), f"call {c}")
        assert len(set(rates[[255, 256, 260]].tolist()) | set(rates[:4].tolist())) > 1
        assert np.array_equal(a.export_streams(ids), b.export_streams(ids))
        assert a.decode_samples_errors() == 0 and b.decode_samples_errors() == 0 and a.rates_errors() == 0
    finally:
        a.close(); b.close()


def test_host_form_and_refusals(golden_dir, oracle_default):
    from lyra_amd.codec import LyraHipError
    ids = np.array([1, 2, 3, 4], np.int32)
    rates = np.array([48000, 8000, 32000, 16000], np.int32)
    rows, size = _packets(oracle_default, golden_dir, [120, 184, 64, 184], 6)
    none = np.zeros(4, np.int32)
    ctx, ref = make_ctx(64), make_ctx(64)
    try:
        fresh = ctx.export_streams(ids)
        with pytest.raises(LyraHipError):
            ctx.decode_samples_streams_end()                                              # nothing in flight
        for bad_rates, bad_sizes in ((np.array([48000, 8000, 44100, 16000]), [128, 160, 441, 7]),
                                     (rates, [128, 641, 75, 7]), (rates, [128, 160, -1, 7]), (rates, [3841, 160, 75, 7])):
            with pytest.raises(LyraHipError):
                ctx.decode_samples_streams_begin(rows[0], size, bad_rates, bad_sizes, ids)
        with pytest.raises(LyraHipError):
            ctx.decode_samples_streams_begin(rows[0], size, rates, [128, 160, 75, 7], [1, 2, 2, 4])   # duplicate id
        with pytest.raises(LyraHipError):
            ctx.decode_samples_streams_begin(rows[0], np.array([23, 23, 9, 23]), rates, [128, 160, 75, 7], ids)   # packet size
        assert np.array_equal(ctx.export_streams(ids), fresh), "a refused begin() changed stream state"
        # one decode pipeline at a time, in both directions
        L = ctx.L
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.lyra_hip_decode_samples_begin.restype, L.lyra_hip_decode_samples_begin.argtypes = ci, [vp, vp, ci, vp, vp, ci, ci]
        L.lyra_hip_decode_samples_end.restype, L.lyra_hip_decode_samples_end.argtypes = ci, [vp, vp]
        other = np.array([40, 41, 42, 43], np.int32)
        r48 = np.full(4, 48000, np.int32)

        def one_hop_begin():
            return L.lyra_hip_decode_samples_begin(ctx.h, other.ctypes.data, 4, rows[0].ctypes.data, none.ctypes.data, 0, 48000)

        begins = {
            "decode_begin": (lambda: ctx.decode_begin(rows[0][:, :8].copy(), 64, other), ctx.decode_end),
            "decode_streams_begin": (lambda: ctx.decode_streams_begin(rows[0], none, r48, other), ctx.decode_streams_end),
            "decode_samples_any_begin": (lambda: ctx.decode_samples_any_begin(rows[0], none, 0, 48000, other),
                                         ctx.decode_samples_any_end),
        }
        for name, (begin, end) in begins.items():
            begin()
            with pytest.raises(LyraHipError):
                ctx.decode_samples_streams_begin(rows[0], none, r48, none, other)
            end()
        assert one_hop_begin() == 0
        with pytest.raises(LyraHipError):
            ctx.decode_samples_streams_begin(rows[0], none, r48, none, other)
        assert L.lyra_hip_decode_samples_end(ctx.h, None) == 0
        ctx.decode_samples_streams_begin(rows[0], none, r48, none, other)
        for name, (begin, end) in begins.items():
            with pytest.raises(LyraHipError):
                begin()
        assert one_hop_begin() != 0
        with pytest.raises(LyraHipError):
            ctx.export_streams([40])
        ctx.decode_samples_streams_begin(rows[0], none, r48, none, other)
        with pytest.raises(LyraHipError):
            ctx.decode_samples_streams_begin(rows[0], none, r48, none, other)             # a third begin()
        for _ in range(2):
            pcm, isn, icn = ctx.decode_samples_streams_end()
            assert pcm.size == 0 and isn.shape == (4,) and icn.shape == (4,)
        # the host form two deep against the _dev form; the first request has all-zero sizes: it delivers packets only
        devc = DeviceStreams(ref, ids, rates)
        calls = [(0, size, [0, 0, 0, 0]), (1, none, [441, 161, 75, 321]), (1, none, [1024, 1, 641, 7]), (2, size, [2, 640, 2560, 1280]),
                 (3, size, [3840, 128, 1, 0]), (4, size, [959, 160, 128, 1024])]
        want = []
        for k, (t, x, n) in enumerate(calls):
            want.append(devc.call(rows[t], x, n))
            if k == 0:
                assert not np.array_equal(ref.export_streams(ids), fresh), "the all-zero request did not queue its packets"
        got = []
        for k, (t, x, n) in enumerate(calls):
            ctx.decode_samples_streams_begin(rows[t], x, rates, n, ids)
            if k:
                got.append(ctx.decode_samples_streams_end())
        got.append(ctx.decode_samples_streams_end())
        for k, (w, g) in enumerate(zip(want, got)):
            assert np.array_equal(np.concatenate(w[0] + [np.zeros(0, np.int16)]), g[0]), f"request {k}: packed pcm"
            assert g[0].size == packed(calls[k][2])[1]
            assert np.array_equal(w[1], g[1]) and np.array_equal(w[2], g[2]), f"request {k}: flags"
        assert np.array_equal(ctx.export_streams(ids), ref.export_streams(ids))
        assert ctx.decode_samples_errors() == 0 and ctx.rates_errors() == 0
    finally:
        ctx.close(); ref.close()


def test_a_larger_batch_begun_behind_one_in_flight(golden_dir, oracle_default):
    """A request of 5 rows begun while a request of 2 rows is in flight, on a context of 8 streams: the second slot is
    allocated for more rows than the first, and the scratch grows under a request in flight.  Then a request of 8 rows in the
    first slot, which has to grow.  Against the blocking `_dev` call on a second context."""
    rates = np.array([48000, 8000, 32000, 16000, 48000, 8000, 32000, 16000], np.int32)
    rows, size = _packets(oracle_default, golden_dir, [120, 184, 64, 184, 120, 64, 184, 120], 3)
    calls = [(2, [441, 161]), (5, [1024, 1, 641, 7, 3840]), (8, [2, 640, 2560, 1280, 959, 160, 128, 1024])]
    ctx, ref = make_ctx(8), make_ctx(8)
    try:
        ids = np.arange(8, dtype=np.int32)
        want = [DeviceStreams(ref, ids[:B], rates[:B]).call(rows[k][:B], size[:B], n) for k, (B, n) in enumerate(calls)]
        got = []
        for k, (B, n) in enumerate(calls):
            ctx.decode_samples_streams_begin(rows[k][:B].copy(), size[:B].copy(), rates[:B].copy(), n, ids[:B])
            if k:
                got.append(ctx.decode_samples_streams_end())
        got.append(ctx.decode_samples_streams_end())
        for k, (w, g) in enumerate(zip(want, got)):
            assert np.array_equal(np.concatenate(w[0]), g[0]), f"request {k}: packed pcm"
            assert np.array_equal(w[1], g[1]) and np.array_equal(w[2], g[2]), f"request {k}: flags"
        assert np.array_equal(ctx.export_streams(ids), ref.export_streams(ids))
        assert ctx.decode_samples_errors() == 0 and ctx.rates_errors() == 0
    finally:
        ctx.close(); ref.close()


def test_decode_pipelines_refuse_each_other_as_before():
    """Which decode pipeline's begin() is refused while which other one is in flight, for every ordered pair of the five decode
    pipelines and for a bridge tick against each of them in both directions.  The relation is written out here: every pair
    of different pipelines refuses, except decode <-> decode_samples (allowed, not known to be intended); a second begin() of
    the pipeline that is in flight is accepted (each is two deep).  Two streams, no packets, requests of 0 samples where the
    call has a size; lyra_hip_decode_begin, decode_streams_begin and the bridge tick run one real hop."""
    from lyra_amd.codec import LyraHipError
    ids = np.array([40, 41], np.int32)
    none, pk = np.zeros(2, np.int32), np.zeros((2, 23), np.uint8)
    r48 = np.full(2, 48000, np.int32)
    ctx = make_ctx(64)
    try:
        L = ctx.L
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.lyra_hip_decode_samples_begin.restype, L.lyra_hip_decode_samples_begin.argtypes = ci, [vp, vp, ci, vp, vp, ci, ci]
        L.lyra_hip_decode_samples_end.restype, L.lyra_hip_decode_samples_end.argtypes = ci, [vp, vp]

        def one_hop_begin():
            if L.lyra_hip_decode_samples_begin(ctx.h, ids.ctypes.data, 2, pk.ctypes.data, none.ctypes.data, 0, 48000) != 0:
                raise LyraHipError(ctx.last_error())

        def one_hop_end():
            assert L.lyra_hip_decode_samples_end(ctx.h, None) == 0

        pipes = {
            "decode": (lambda: ctx.decode_begin(pk[:, :8].copy(), 64, ids), ctx.decode_end),
            "decode_streams": (lambda: ctx.decode_streams_begin(pk, none, r48, ids), ctx.decode_streams_end),
            "decode_samples": (one_hop_begin, one_hop_end),
            "decode_samples_any": (lambda: ctx.decode_samples_any_begin(pk, none, 0, 48000, ids), ctx.decode_samples_any_end),
            "decode_samples_streams": (lambda: ctx.decode_samples_streams_begin(pk, none, r48, none, ids),
                                       ctx.decode_samples_streams_end),
            "bridge": (lambda: ctx.bridge_begin(pk, none, [0, 0], [64, 64], stream_ids=ids), ctx.bridge_end),
        }
        decoders = [p for p in pipes if p != "bridge"]
        refuses = {(x, y): x != y and {x, y} != {"decode", "decode_samples"} for x in pipes for y in pipes}
        pairs = [(x, y) for x in decoders for y in decoders] + [("bridge", y) for y in decoders] + \
                [(x, "bridge") for x in decoders]
        assert len(pairs) == 35 and sum(refuses[p] for p in pairs) == 28
        for x, y in pairs:
            pipes[x][0]()
            if refuses[x, y]:
                with pytest.raises(LyraHipError):
                    pipes[y][0]()
            else:
                pipes[y][0]()                  # accepted: it raises otherwise
                pipes[y][1]()
            pipes[x][1]()
            ctx.export_streams(ids)            # (refused while anything is in flight: both were ended, a refused begin left nothing)
    finally:
        ctx.close()


def test_a_leftover_travels(golden_dir, oracle_default):
    """A 48 kHz stream that holds 2 samples is exported from a context driven by the new call and imported into one driven by
    decode_samples_any_dev; both go on, bit for bit."""
    rate = 48000
    rows, size = _packets(oracle_default, golden_dir, [184], 8, offset=70)
    a, b = make_ctx(64), make_ctx(64)
    try:
        da, db = DeviceStreams(a, [5], [rate]), DeviceAny(b, [5], rate)
        none = np.zeros(1, np.int32)
        da.call(rows[0], size, [128])
        da.call(rows[1], size, [128])          # 128 + 128 = 256 = 3 * 86 - 2: two samples stay
        b.import_streams([5], a.export_streams([5]))
        for c, (n, t) in enumerate([(2, None), (1, None), (1024, 2), (441, 3), (3840, None), (128, 4), (3, None), (959, 5)]):
            nb, pk = (none, rows[0]) if t is None else (size, rows[t])
            x, y = da.call(pk, nb, [n]), db.call(pk, nb, n)
            _same(x, y, f"call {c} ({n} samples)")
        assert np.array_equal(a.export_streams([5]), b.export_streams([5]))
    finally:
        a.close(); b.close()


def test_the_class_on_the_device(tmp_path, golden_dir):
    """lyra_amd/device_decoder_demo with LYRA_DEMO_MIXED_ANY_SIZE=1: one MixedAnySizeDeviceLyraDecoder over streams at four rates
    with differing callback sizes against one AnySizeDeviceLyraDecoder per (rate, size) class over the same packets; it compares
    every sample itself and exits non-zero on a difference."""
    import lyra_amd
    from signals import _speech
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    exe = os.path.join(root, "lyra_amd", "device_decoder_demo")
    assert os.path.exists(exe), "demo not built (__graft_entry__.build())"
    n, T = 16, 20
    pin = tmp_path / "in.s16"
    _speech(golden_dir, n, T).astype(np.int16).tofile(pin)
    env = dict(os.environ, LYRA_DEMO_MIXED_ANY_SIZE="1")
    r = subprocess.run([exe, lyra_amd.default_model_dir(), str(pin), str(n), str(T)], capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "mixed any-size: " in r.stdout and " samples equal" in r.stdout, r.stdout[-2000:]
