"""Decoders of any sample rate and packet size in one batch (include/lyra_hip_decode_streams.h):
lyra_hip_decode_streams_dev, its two-deep host form lyra_hip_decode_streams_begin / _end and the C++ class
MixedBatchLyraDecoder (through mixed_decoder_demo).  Expectation of the device calls: lyra_hip_decode_lossy_rates_dev on a
twin context `u` with the same comfort-noise seed, fed the same packets -- the 16 kHz hop, each row's rate / 50 samples, both
flags and every byte of the exported stream state.  Expectation of the class: oracle/lyra_codec_model.RefLyraDecoder per
stream, under the criteria of tests/receiver_models.py (Tally, CnReach).

Shapes.  The resampler and the mix serve 4 rows per workgroup, the estimator 2: B = 37 (10 workgroups, the last with one row)
and B = 5.  Packets are random bytes with sizes from a bursty loss pattern (signals._random_packets); rows 0..11 -- three
rows of every rate -- lose hops 2..13 and receive 23-byte packets on hops 14..23, the pattern of
test_gpu_mixed_rate._decode_case, which takes every rate group into comfort noise and back: asserted on `u`'s flags.

Stream kind: the contexts here (64 streams) run on the CU-masked streams the library picks up to 1,024 streams, which are
blocking streams with respect to the NULL stream; the case with streams="plain" runs on hipStreamNonBlocking streams, the kind
of a 4,096-stream context (tests/gpu_plumbing.py make_ctx)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_plumbing import _dev, _ids, _t, make_ctx as _ctx, stream_cases
from receiver_models import CnReach, Tally
from row_cases import ROW, _decode_rates, _rates, _same_state
from signals import RATES, _gilbert, _random_packets as _packets, _speech

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))

FILL = 0x3333
EINVAL = -1


def _case_packets(T, B, seed):
    pk, sz = _packets(np.random.default_rng(seed), T, B)
    sz[2:14, :min(B, 12)] = 0     # >= 5 consecutive losses in every rate group (rows 0..11 cover the four rates) ...
    sz[14:24, :min(B, 12)] = 23   # ... and packets again: the fade back
    return pk, sz


def _streams_dev(a, ids, pk_t, sz_t, rates, offsets=None, total=None, with16=True, n_pcm=None):
    """decode_streams_dev into a buffer of `total` samples filled with FILL -> (pcm16 or None, buffer, is_noise, is_cn)."""
    import torch
    B = ids.size
    total = B * ROW if total is None else total
    d16 = torch.zeros((B, 320), dtype=torch.int16, device=_dev()) if with16 else None
    buf = torch.full((total,), FILL, dtype=torch.int16, device=_dev())
    dn = torch.full((B,), -3, dtype=torch.int32, device=_dev())
    dc = torch.full((B,), -3, dtype=torch.int32, device=_dev())
    a.decode_streams_dev(_t(ids), _t(pk_t), _t(sz_t), _t(rates), buf, None if offsets is None else _t(offsets), d16, dn, dc,
                         n_pcm_samples=n_pcm)
    a.synchronize()
    return None if d16 is None else d16.cpu().numpy(), buf.cpu().numpy(), dn.cpu().numpy(), dc.cpu().numpy()


def _back_to_back(rates, order):
    """offsets [B] of rows laid back to back in `order`, and the buffer's length"""
    off = np.zeros(rates.size, np.int32)
    pos = 0
    for b in order:
        off[b] = pos
        pos += int(rates[b]) // 50
    return off, pos


def _check_packed(got, want, rates, offsets, where, skip=()):
    """got: _streams_dev's tuple; want: _decode_rates' on the twin.  Every row equals the twin's, every other sample of the
    buffer is FILL (`skip`: rows that must have written nothing)."""
    g16, buf, gn, gc = got
    w16, wx, wn, wc = want
    if g16 is not None:
        assert np.array_equal(g16, w16), where
    assert np.array_equal(gn, wn) and np.array_equal(gc, wc), where
    rest = np.ones(buf.size, bool)
    for b, r in enumerate(rates):
        if b in skip:
            continue
        n = int(r) // 50
        assert np.array_equal(buf[offsets[b]:offsets[b] + n], wx[b, :n]), (where, b, int(r))
        rest[offsets[b]:offsets[b] + n] = False
    assert (buf[rest] == FILL).all(), (where, "samples outside the rows were written", np.flatnonzero(buf[rest] != FILL)[:8])


def _cn_and_back(cn, rates):
    for r in np.unique(rates):
        g = cn[:, rates == r]
        assert (g == 1).any() and ((g[:-1] == 1) & (g[1:] == 0)).any(), (int(r), "the twin never left comfort noise")


# ---- 1. the padded layout equals the rates call ---------------------------------------------------------------------------

def _padded_case(B, serial, streams=None):
    T, ms = 40, 64
    ids = _ids(B, ms, B + 9)
    rates = _rates(B)
    pk, sz = _case_packets(T, B, B)
    pad = np.arange(B, dtype=np.int32) * ROW
    a, u = _ctx(ms, streams=streams), _ctx(ms, streams=streams)
    try:
        if serial:
            a.set_serial(True)
        cn = np.zeros((T, B), np.int32)
        for t in range(T):
            got = _streams_dev(a, ids, pk[t], sz[t], rates)
            want = _decode_rates(u, ids, pk[t], sz[t], rates)
            _check_packed(got, want, rates, pad, f"hop {t}")   # (samples past rate / 50 of a row are "outside the rows")
            cn[t] = want[3]
        _cn_and_back(cn, rates)
        assert a.rates_errors() == 0 and a.decode_lossy_errors() == 0
        _same_state(a, u, ids, "after the last hop")
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B,serial,streams", stream_cases([(37, False), (37, True), (5, False)], plain=(37, False)))
def test_padded_layout_equals_the_rates_call(B, serial, streams):
    _padded_case(B, serial, streams)


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_decode_streams as T
T._padded_case(37, False)
print("child ok")
"""


@pytest.mark.gpu
def test_padded_layout_on_a_split_context():
    """LYRA_HIP_SUBBATCHES=2 (read at context creation, hence a child process): the call is accepted and not split."""
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, HERE], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, LYRA_HIP_SUBBATCHES="2"))
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


# ---- 2. packed rows -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pcm16", ["given", "null", "alternating"])
def test_packed_rows_equal_the_rates_call(pcm16):
    B, T, ms = 12, 30, 64
    ids = _ids(B, ms, 21)
    rates = _rates(B)                      # three rows of every rate
    pk, sz = _case_packets(T, B, 3)
    a, u = _ctx(ms), _ctx(ms)
    try:
        cn = np.zeros((T, B), np.int32)
        for t in range(T):
            off, total = _back_to_back(rates, np.random.default_rng(100 + t).permutation(B))
            with16 = pcm16 == "given" or (pcm16 == "alternating" and t % 2 == 1)
            got = _streams_dev(a, ids, pk[t], sz[t], rates, off, total, with16)
            want = _decode_rates(u, ids, pk[t], sz[t], rates)
            _check_packed(got, want, rates, off, f"hop {t}")
            cn[t] = want[3]
        _cn_and_back(cn, rates)
        assert a.rates_errors() == 0
        _same_state(a, u, ids, "after the last hop")
    finally:
        a.close()
        u.close()


# ---- 3. a stream moves between the calls ----------------------------------------------------------------------------------

@pytest.mark.gpu
def test_streams_move_between_the_two_calls():
    T, ms = 24, 64
    rates = np.repeat(np.array(RATES, np.int32), 6)
    B = rates.size
    ids = _ids(B, ms, 5)
    pk, sz = _packets(np.random.default_rng(8), T, B)
    sz[2:14, ::2] = 0
    sz[14:24, ::2] = 23
    off, total = _back_to_back(rates, np.random.default_rng(6).permutation(B))
    a, u = _ctx(ms), _ctx(ms)
    try:
        for t in range(T):
            want = _decode_rates(u, ids, pk[t], sz[t], rates)
            if t % 2 == 0:
                _check_packed(_streams_dev(a, ids, pk[t], sz[t], rates, off, total, with16=t % 4 == 0), want, rates, off, f"hop {t}")
            else:
                got = _decode_rates(a, ids, pk[t], sz[t], rates)
                assert all(np.array_equal(x, y) for x, y in zip(got, want)), f"hop {t}"
        _same_state(a, u, ids, "after the last hop")
    finally:
        a.close()
        u.close()


# ---- 4. invalid rows ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_invalid_rows_write_nothing_and_keep_their_resampler_slot():
    """Hops 6..9: rows 0..6 are invalid, each for its own reason.  The twin decodes those rows at 16 kHz on those hops (its
    resampler slot is then not touched either) into rows that are not compared."""
    B, T, ms = 12, 20, 64
    ids = _ids(B, ms, 31)
    rates = np.array([8000, 32000, 48000, 8000, 48000, 32000, 8000, 16000, 32000, 48000, 8000, 16000], np.int32)
    pk, sz = _packets(np.random.default_rng(12), T, B)
    sz[:, :7] = 23                                   # the rows under test play throughout
    sz[4:8, :7:2] = 0                                # ... but for a short loss across the window's start
    off, total = _back_to_back(rates, np.arange(B))
    bad_hops = range(6, 10)
    # (row, what is wrong): offsets first, then rates.  Row 2's offset is aligned and inside the buffer, its end 8 samples past
    # it: only the upper bound refuses it (one sample past: test_the_upper_bound_is_n_pcm_samples)
    bad_off = {0: -8, 1: int(off[1]) + 4, 2: total - 960 + 8, 3: total}
    bad_rate = {4: 0, 5: 44100, 6: -1}
    bad_rows = sorted(bad_off) + sorted(bad_rate)
    a, u = _ctx(ms), _ctx(ms)
    try:
        errors = 0
        for t in range(T):
            o, r, r_u = off.copy(), rates.copy(), rates.copy()
            skip = ()
            if t in bad_hops:
                for b, v in bad_off.items():
                    o[b] = v
                for b, v in bad_rate.items():
                    r[b] = v
                r_u[bad_rows] = 16000
                skip = bad_rows
                errors += len(bad_rows)
            got = _streams_dev(a, ids, pk[t], sz[t], r, o, total)
            want = _decode_rates(u, ids, pk[t], sz[t], r_u)
            # d_pcm16 and the flags of every row, the invalid ones included, are the 16 kHz run's; valid rows as without them;
            # the buffer holds FILL wherever no valid row lies -- where the invalid rows would have gone included
            _check_packed(got, want, rates, off, f"hop {t}", skip=skip)
            assert a.rates_errors() == errors, (t, errors)
        # (the hops after the window compared the invalid rows' samples with a twin whose slots never saw the window)
        _same_state(a, u, ids, "after the last hop")
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [8000, 48000, 16000])
def test_the_upper_bound_is_n_pcm_samples(rate):
    """The bound that keeps a row inside the buffer, apart from the alignment rule and from the tensor's own length: the row
    under test is aligned and valid in every other respect, lies last in a tensor two rows longer than the layout, and
    n_pcm_samples is what changes.  One sample short of the row's end: refused and counted, the whole tensor past the other
    rows -- the tail behind n_pcm_samples included -- keeps its fill.  Exactly the row's end: accepted."""
    import lyra_amd
    import torch
    B, ms = 4, 16
    rates = np.array([r for r in RATES if r != rate] + [rate], np.int32)
    ids = np.arange(B, dtype=np.int32)
    off, used = _back_to_back(rates, np.arange(B))
    assert off[B - 1] % 8 == 0 and off[B - 1] + rate // 50 == used
    tensor = used + 2 * ROW
    pk, sz = _packets(np.random.default_rng(rate), 4, B)
    sz[:] = 23
    a, u = _ctx(ms), _ctx(ms)
    try:
        for t, (n_pcm, valid) in enumerate([(used, True), (used - 1, False), (used, True), (tensor, True)]):
            r_u = rates.copy()
            if not valid:
                r_u[B - 1] = 16000
            got = _streams_dev(a, ids, pk[t], sz[t], rates, off, tensor, n_pcm=n_pcm)
            want = _decode_rates(u, ids, pk[t], sz[t], r_u)
            _check_packed(got, want, rates, off, f"hop {t}, n_pcm_samples {n_pcm}", skip=() if valid else (B - 1,))
            assert a.rates_errors() == (0 if t == 0 else 1), t
        _same_state(a, u, ids, "after the last hop")
        # (the Python mirror does not let n_pcm_samples exceed the tensor)
        buf = torch.zeros(tensor, dtype=torch.int16, device=_dev())
        with pytest.raises(lyra_amd.LyraHipError):
            a.decode_streams_dev(_t(ids), _t(pk[0]), _t(sz[0]), _t(rates), buf, _t(off), n_pcm_samples=tensor + 1)
    finally:
        a.close()
        u.close()


# ---- 5. argument checks ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_argument_checks_enqueue_nothing():
    import torch
    B, ms = 5, 16
    ids = np.arange(B, dtype=np.int32)
    rates = np.array([8000, 16000, 32000, 48000, 16000], np.int32)
    pk, sz = _packets(np.random.default_rng(2), 3, B)
    sz[:] = 23
    off, total = _back_to_back(rates, np.arange(B))
    a, u = _ctx(ms), _ctx(ms)
    try:
        _check_packed(_streams_dev(a, ids, pk[0], sz[0], rates, off, total), _decode_rates(u, ids, pk[0], sz[0], rates), rates, off, 0)
        big = ms + 1
        bufs = dict(ids=_t(np.arange(big, dtype=np.int32)), pk=torch.zeros((big, 23), dtype=torch.uint8, device=_dev()),
                    pb=_t(np.full(big, 23, np.int32)), rates=_t(np.full(big, 16000, np.int32)),
                    pcm=torch.full((big * ROW,), FILL, dtype=torch.int16, device=_dev()),
                    off=_t(np.arange(big, dtype=np.int32) * ROW), p16=torch.full((big, 320), FILL, dtype=torch.int16, device=_dev()),
                    dn=torch.full((big,), -3, dtype=torch.int32, device=_dev()),
                    dc=torch.full((big,), -3, dtype=torch.int32, device=_dev()))
        p = {k: v.data_ptr() for k, v in bufs.items()}

        def call(B_=B, n=big * ROW, ctx=a.h, **null):
            g = lambda k: None if k in null else p[k]   # noqa: E731
            return a.L.lyra_hip_decode_streams_dev(ctx, g("ids"), B_, g("pk"), g("pb"), g("rates"), g("pcm"), n, g("off"),
                                                   g("p16"), g("dn"), g("dc"))
        for k in ("ids", "pk", "pb", "rates", "pcm"):
            assert call(**{k: True}) == EINVAL, k
        assert call(B_=0) == EINVAL and call(B_=-1) == EINVAL and call(B_=big) == EINVAL
        assert call(n=-1) == EINVAL
        assert call(ctx=None) == EINVAL
        a.synchronize()
        assert a.rates_errors() == 0 and a.decode_lossy_errors() == 0
        for k in ("pcm", "p16"):
            assert (bufs[k].cpu().numpy() == FILL).all(), k
        assert (bufs["dn"].cpu().numpy() == -3).all() and (bufs["dc"].cpu().numpy() == -3).all()
        # the next valid hop is the twin's
        _check_packed(_streams_dev(a, ids, pk[1], sz[1], rates, off, total), _decode_rates(u, ids, pk[1], sz[1], rates), rates, off, 1)
        _same_state(a, u, np.arange(ms, dtype=np.int32), "after the refusals")
    finally:
        a.close()
        u.close()


# ---- 6. host form ---------------------------------------------------------------------------------------------------------

def _want_host(u, ids, pk_t, sz_t, rates):
    """what end() must hand over: the blocking `_dev` call on the twin, rows packed in batch order"""
    off, total = _back_to_back(rates, np.arange(rates.size))
    _, buf, dn, dc = _streams_dev(u, ids, pk_t, sz_t, rates, off, total)
    return buf, dn, dc


@pytest.mark.gpu
def test_begin_end_equals_the_dev_call():
    import lyra_amd
    import torch
    B, T, ms = 9, 12, 64
    rates = np.array([48000, 8000, 16000, 32000, 8000, 48000, 16000, 32000, 8000], np.int32)
    ids = _ids(B, ms, 40)
    pk, sz = _packets(np.random.default_rng(41), T, B)
    sz[1:9, :4] = 0                       # comfort noise on rows of every rate: both flags take both values
    a, u = _ctx(ms), _ctx(ms)
    samples_begin = a.L.lyra_hip_decode_samples_begin   # (not in the Python mirror: the C call itself)
    samples_begin.restype, samples_begin.argtypes = ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2
    samples_end = a.L.lyra_hip_decode_samples_end
    samples_end.restype, samples_end.argtypes = ctypes.c_int, [ctypes.c_void_p] * 2
    spare = np.setdiff1d(np.arange(ms), ids)[:2].astype(np.int32)
    try:
        want, got = [], []

        def begin(t, how):
            if how == "pinned":   # hipHostMalloc'ed inputs, through torch's pinned tensors
                args = [torch.from_numpy(x.copy()).pin_memory() for x in (pk[t], sz[t], rates)]
                a.decode_streams_begin(*args, stream_ids=ids)
                for x in args:
                    x.fill_(77)               # the caller's arrays are the caller's again
            else:
                args = [pk[t].copy(), sz[t].copy(), rates.copy()]
                a.decode_streams_begin(*args, stream_ids=ids)
                for x in args:
                    x[...] = 77
            want.append(_want_host(u, ids, pk[t], sz[t], rates))

        def end():
            got.append(a.decode_streams_end())

        def refused(fn, *args, **kw):
            n = len(a._pending_stream_decodes)
            with pytest.raises(lyra_amd.LyraHipError):
                fn(*args, **kw)
            assert len(a._pending_stream_decodes) == n

        refused(a.decode_streams_end)                       # nothing in flight
        begin(0, "pageable")
        end()                                               # blocking use
        for t in range(1, T):
            begin(t, "pinned" if t & 1 else "pageable")
            if t == 1:
                continue
            if t == 6:   # two in flight: every refusal leaves them, and the streams, as they are
                refused(a.decode_streams_begin, pk[t], sz[t], rates, stream_ids=ids)                 # a third
                refused(a.decode_begin, np.zeros((2, 23), np.uint8), 184, stream_ids=spare)           # the other pipelines
                assert samples_begin(a.h, spare.ctypes.data, 2, np.zeros((2, 23), np.uint8).ctypes.data,
                                     np.zeros(2, np.int32).ctypes.data, 320, 16000) == EINVAL
                refused(a.export_streams, ids)
                refused(a.import_streams, ids[:1], np.zeros((1, a.stream_blob_bytes()), np.uint8))
            end()
        # one in flight (hop T - 1): the host checks of begin() change nothing
        for bad in (44100, 0, -16000):
            r2 = rates.copy(); r2[B - 1] = bad
            refused(a.decode_streams_begin, pk[0], sz[0], r2, stream_ids=ids)
        for bad in (1, 16, 24, -8):
            s2 = sz[0].copy(); s2[B - 1] = bad
            refused(a.decode_streams_begin, pk[0], s2, rates, stream_ids=ids)
        for bad in ((3, ids[4]), (0, ms), (0, -1)):
            i2 = ids.copy(); i2[bad[0]] = bad[1]
            refused(a.decode_streams_begin, pk[0], sz[0], rates, stream_ids=i2)
        end()
        refused(a.decode_streams_end)
        for t in range(T):
            for x, y, what in zip(got[t], want[t], ("samples", "is_noise", "is_comfort_noise")):
                assert np.array_equal(x, y), (f"hop {t}", what)
        cn = np.stack([w[2] for w in want])
        noise = np.stack([w[1] for w in want])
        assert set(np.unique(cn)) == {0, 1} and set(np.unique(noise)) <= {0, 1}
        assert a.rates_errors() == 0 and a.decode_lossy_errors() == 0
        # the other pipelines in flight refuse this one
        a.decode_begin(np.zeros((2, 23), np.uint8), 184, stream_ids=spare)
        refused(a.decode_streams_begin, pk[0], sz[0], rates, stream_ids=ids)
        a.decode_end()
        assert samples_begin(a.h, spare.ctypes.data, 2, np.zeros((2, 23), np.uint8).ctypes.data, np.zeros(2, np.int32).ctypes.data,
                             320, 16000) == 0
        refused(a.decode_streams_begin, pk[0], sz[0], rates, stream_ids=ids)
        out = np.empty((2, 320), np.int16)
        assert samples_end(a.h, out.ctypes.data) == 0
        _same_state(a, u, ids, "after the refusals")
        # reset_streams drains: a hop in flight is still delivered, and complete
        begin(0, "pageable")
        a.reset(spare)
        end()
        for x, y in zip(got[-1], want[-1]):
            assert np.array_equal(x, y)
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
def test_a_larger_batch_begun_behind_one_in_flight():
    """A hop of 5 rows begun while a hop of 2 rows is in flight, on a context of 8 streams: the scratch grows under a request
    in flight.  Against the blocking `_dev` call on the twin."""
    ms, sizes = 8, (2, 5)
    rates = np.array([48000, 8000, 16000, 32000, 8000], np.int32)
    pk, sz = _packets(np.random.default_rng(43), len(sizes), 5)
    sz[:, :2] = 23
    a, u = _ctx(ms), _ctx(ms)
    try:
        ids = np.arange(5, dtype=np.int32)
        want = [_want_host(u, ids[:B], pk[k][:B], sz[k][:B], rates[:B]) for k, B in enumerate(sizes)]
        for k, B in enumerate(sizes):
            a.decode_streams_begin(pk[k][:B].copy(), sz[k][:B].copy(), rates[:B].copy(), stream_ids=ids[:B])
        got = [a.decode_streams_end(), a.decode_streams_end()]
        for k in range(len(sizes)):
            for x, y, what in zip(got[k], want[k], ("samples", "is_noise", "is_comfort_noise")):
                assert np.array_equal(x, y), (f"request {k}", what)
        assert a.rates_errors() == 0 and a.decode_lossy_errors() == 0
        _same_state(a, u, ids, "after the last request")
    finally:
        a.close()
        u.close()


# ---- 7. the class against the reference model -----------------------------------------------------------------------------

N_STREAMS, T_SESSION = 8, 60
SESSION_RATES = [RATES[s // 2] for s in range(N_STREAMS)]
BITRATE_BITS = {3200: 64, 6000: 120, 9200: 184}


@pytest.fixture(scope="module")
def session_reference(golden_dir, oracle_default):
    """The session's packets (RefLyraEncoder on golden speech, bitrates switching per stream on a script), its loss pattern,
    and what RefLyraDecoder(rate, seed ^ stream) per stream plays: computed once.  -> (packets [T][n][23], lengths [T][n]
    as received, per stream the played samples [T][rate / 50], the comfort-noise reach of each, is_comfort_noise [T][n])."""
    from oracle import lyra_codec_model as M
    n, T = N_STREAMS, T_SESSION
    pcm = _speech(golden_dir, n, T, offset=17)
    rng = np.random.default_rng(78)
    bitrate = np.empty((T, n), np.int32)
    bitrate[:] = [(3200, 6000, 9200)[s % 3] for s in range(n)]
    for _ in range(20):
        bitrate[int(rng.integers(1, T)):, int(rng.integers(0, n))] = int(rng.choice((3200, 6000, 9200)))
    rx = _gilbert(np.random.default_rng(79), T, n)
    rx[:] = 1 - (1 - rx) * (np.arange(n) % 2 == 0)    # (scattered losses on the even streams only ...)
    rx[4:16] = 1
    rx[30:44, 1::2] = 0                               # ... and the long burst on one stream of every rate
    encs = [M.RefLyraEncoder(oracle_default, r, 64, False) for r in SESSION_RATES]
    decs = [M.RefLyraDecoder(oracle_default, r, cng_seed=0x4C797261 ^ s) for s, r in enumerate(SESSION_RATES)]
    reach = [CnReach(r) for r in SESSION_RATES]
    packets = np.zeros((T, n, 23), np.uint8)
    lengths = np.zeros((T, n), np.int32)
    want = [np.zeros((T, r // 50), np.int16) for r in SESSION_RATES]
    cn_reach = [np.zeros((T, r // 50), bool) for r in SESSION_RATES]
    is_cn = np.zeros((T, n), np.int32)
    back = np.zeros(n, int)
    for t in range(T):
        for s, r in enumerate(SESSION_RATES):
            encs[s].bits = BITRATE_BITS[int(bitrate[t, s])]
            p = encs[s].Encode(np.repeat(pcm[t, s], r // 16000) if r >= 16000 else pcm[t, s, ::2])
            if rx[t, s]:
                packets[t, s, :p.size] = p
                lengths[t, s] = p.size
                decs[s].SetEncodedPacket(p)
            was = decs[s].is_comfort_noise()
            want[s][t] = decs[s].DecodeSamples(r // 50)
            cn_reach[s][t] = reach[s](decs[s], r // 50)
            is_cn[t, s] = int(decs[s].is_comfort_noise())
            back[s] += int(was and not decs[s].is_comfort_noise())
    # the session exercised what it is about, on the model's side: every rate saw comfort noise and the fade back, and all
    # three packet sizes occurred
    for r in RATES:
        sel = [s for s in range(n) if SESSION_RATES[s] == r]
        assert is_cn[:, sel].any() and back[sel].sum() > 0, r
    assert set(np.unique(lengths)) == {0, 8, 15, 23}
    return packets, lengths, want, cn_reach, is_cn


def _run_demo(tmp_path, mode, packets, lengths):
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "mixed_decoder_demo")
    assert os.path.exists(demo), "lyra_amd/mixed_decoder_demo not built (__graft_entry__.build())"
    (tmp_path / "rates.txt").write_text("".join(f"{r}\n" for r in SESSION_RATES))
    packets.tofile(tmp_path / "pk.bin")
    lengths.tofile(tmp_path / "len.i32")
    out, flags = tmp_path / f"out{mode}.s16", tmp_path / f"cn{mode}.i32"
    r = subprocess.run([demo, lyra_amd.default_model_dir(), str(tmp_path / "rates.txt"), str(tmp_path / "pk.bin"),
                        str(tmp_path / "len.i32"), str(out), str(flags)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, LYRA_DEMO_PIPELINED=mode))
    assert r.returncode == 0, (mode, r.returncode, r.stderr[-3000:])
    hop = sum(SESSION_RATES) // 50
    return np.fromfile(out, np.int16).reshape(T_SESSION, hop), np.fromfile(flags, np.int32).reshape(T_SESSION, N_STREAMS)


@pytest.mark.gpu
def test_mixed_batch_decoder_equals_the_reference_model(tmp_path, session_reference):
    packets, lengths, want, cn_reach, is_cn = session_reference
    runs = [_run_demo(tmp_path, mode, packets, lengths) for mode in ("0", "1")]
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), "the two demo modes differ"
    pcm, flags = runs[0]
    assert np.array_equal(flags, is_cn), np.argwhere(flags != is_cn)[:8]
    start = np.concatenate([[0], np.cumsum([r // 50 for r in SESSION_RATES])])
    for s, r in enumerate(SESSION_RATES):
        tally = Tally(cn_lsb=1 if r == 16000 else 2)
        for t in range(T_SESSION):
            tally.check(pcm[t, start[s]:start[s + 1]], want[s][t], cn_reach[s][t], f"hop {t}, stream {s} ({r} Hz)")
        tally.report(f"MixedBatchLyraDecoder stream {s}, {r} Hz")
    # the demo's output == decode_streams_begin / _end driven from Python on a context with the default seed, bit for bit
    a = _ctx(N_STREAMS)
    try:
        rates = np.array(SESSION_RATES, np.int32)
        got = []
        a.decode_streams_begin(packets[0], lengths[0], rates)
        for t in range(T_SESSION):
            if t + 1 < T_SESSION:
                a.decode_streams_begin(packets[t + 1], lengths[t + 1], rates)
            got.append(a.decode_streams_end())
        assert np.array_equal(np.stack([g[0] for g in got]), pcm)
        assert np.array_equal(np.stack([g[2] for g in got]), flags)
    finally:
        a.close()
