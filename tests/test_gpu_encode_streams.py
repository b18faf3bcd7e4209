"""Encoders of any sample rate, bitrate and DTX setting in one batch (include/lyra_hip_encode_streams.h):
lyra_hip_encode_streams_dev, its two-deep host form lyra_hip_encode_streams_begin / _end and the C++ class
MixedBatchLyraEncoder (through mixed_encoder_demo).  Expectation of the device calls: lyra_hip_encode_rates_dev on a twin
context fed the same audio, once with dtx = 1 on the flagged rows and once with dtx = 0 on the rest -- packets, packet_bytes
and every byte of the exported stream state.  Expectation of the class: oracle/lyra_codec_model.RefLyraEncoder per stream.

Shapes.  The estimator serves 2 streams per workgroup, the resampler 4 rows, the quantizer 16 rows per tile: B = 37 (19
estimator workgroups, the last with one row; 10 resampler workgroups, the last with one row; 3 quantizer tiles, the last
with 5 rows) and B = 5.  Rows 0..7 of the B = 37 layout pin the pairs (on, off), (off, on), (on, absent), (absent, off) into
estimator workgroups 0..3 on every hop; every other flag is redrawn every hop.  T = 40 hops with every third stream silent
from hop 5 on, as the DTX case of tests/test_gpu_mixed_rate.py: on the CPU, oracle NoiseEstimators at the rows' rates fed
exactly the flagged hops of this audio and these flags decide "noise" and "not noise" at every rate (counts in
_COND_CPU below), so the flagged rows give empty and non-empty packets at every rate.

Stream kind: the contexts here (64 streams) run on the CU-masked streams the library picks up to 1,024 streams, which are
blocking streams with respect to the NULL stream; the case with streams="plain" runs on hipStreamNonBlocking streams, the kind
of a 4,096-stream context (tests/gpu_plumbing.py make_ctx)."""
import os
import subprocess

import numpy as np
import pytest

from gpu_plumbing import _dev, _ids, _t, make_ctx, stream_cases
from row_cases import ROW, SENTINEL, _check_sentinel_rows as _check_rows, _same_state
from signals import RATES, _pcm_rows, _speech

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))

BITS = (64, 120, 184)
T_HOPS = 40
EINVAL = -1
BAD_RATE = 44100
# Flagged hops that the oracle's NoiseEstimators call noise / not noise, per rate (8, 16, 32, 48 kHz), for B = 37, T = 40 and
# the flags of _flags(37, 40, ..., seed 37): computed on the CPU with oracle/lyra_oracle.NoiseEstimator + Resampler, each
# estimator fed only the hops on which its row's flag is set.  The GPU test asserts the condition (both > 0 at every rate)
# on the twin's output, and that the twin decided exactly as the oracle did: a change of the audio or of the flags that is
# not followed by a new CPU confirmation fails there.
_COND_CPU = {"noise": (100, 81, 46, 71), "not_noise": (153, 187, 157, 197)}


def _ctx(max_streams=64, **kw):
    return make_ctx(max_streams, **kw)


def _row_layout(B):
    """-> (rates [B] with BAD_RATE for the absent rows, bits [B], fixed [B]: 1 / 0 = flag pinned on / off, -1 = redrawn)."""
    rates = np.array([RATES[(b // 3) % 4] for b in range(B)], np.int32)
    bits = np.array([BITS[(b + b // 16) % 3] for b in range(B)], np.int32)
    fixed = np.full(B, -1, np.int32)
    if B >= 8:
        fixed[:8] = (1, 0, 0, 1, 1, -1, -1, 0)   # (on, off) (off, on) (on, absent) (absent, off)
        rates[5] = rates[6] = BAD_RATE
    else:   # B = 5: (on, absent) (absent, off) and a workgroup with one row, redrawn
        fixed[:4] = (1, -1, -1, 0)
        rates = np.array([8000, BAD_RATE, BAD_RATE, 48000, 32000], np.int32)
    return rates, bits, fixed


def _flags(B, T, fixed, seed):
    f = (np.random.default_rng(seed).random((T, B)) < 0.75).astype(np.int32)
    f[:, fixed >= 0] = fixed[fixed >= 0]
    return f


def _streams_dev(a, ids, pcm, rates, bits, flags, offsets=None, n_pcm=None):
    """one lyra_hip_encode_streams_dev call -> (packets [B][23] over a sentinel, packet_bytes [B])"""
    import torch
    B = ids.size
    d_pk = torch.full((B, 23), SENTINEL, dtype=torch.uint8, device=_dev())
    d_pb = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    a.encode_streams_dev(_t(ids), pcm if hasattr(pcm, "is_cuda") else _t(pcm), _t(rates), _t(bits), d_pk, d_pb,
                         d_dtx=None if flags is None else _t(flags, np.int32),
                         d_pcm_offsets=None if offsets is None else _t(offsets, np.int32), n_pcm_samples=n_pcm)
    a.synchronize()
    return d_pk.cpu().numpy(), d_pb.cpu().numpy()


def _uniform(u, ids, pcm_t, rates, bits, flags):
    """The twin: encode_rates_dev(dtx=True) on the flagged valid rows, encode_rates_dev(dtx=False) on the other valid rows;
    rows with an invalid rate are omitted (packet_bytes 0) -> (packets [B][23] over the sentinel, packet_bytes [B])."""
    import torch
    B = ids.size
    pk = np.full((B, 23), SENTINEL, np.uint8)
    pb = np.zeros(B, np.int32)
    valid = np.isin(rates, RATES)
    for dtx in (True, False):
        sel = np.flatnonzero(valid & ((flags != 0) == dtx))
        if not sel.size:
            continue
        d_pk = torch.full((sel.size, 23), SENTINEL, dtype=torch.uint8, device=_dev())
        d_pb = torch.full((sel.size,), -7, dtype=torch.int32, device=_dev())
        u.encode_rates_dev(_t(ids[sel]), _t(pcm_t[sel]), _t(rates[sel]), _t(bits[sel]), d_pk, d_pb, dtx=dtx)
        u.synchronize()
        pk[sel], pb[sel] = d_pk.cpu().numpy(), d_pb.cpu().numpy()
    return pk, pb


# ---- 1. per-row DTX equals the uniform calls -----------------------------------------------------------------------------

def _per_row_case(golden_dir, B, sub_batches, serial, streams=None):
    ms = 64
    ids = _ids(B, ms, B + 11)
    rates, bits, fixed = _row_layout(B)
    flags = _flags(B, T_HOPS, fixed, B)
    pcm_a = _pcm_rows(golden_dir, B, T_HOPS, rates, 3, B, 0x1111)
    pcm_u = _pcm_rows(golden_dir, B, T_HOPS, rates, 3, B, 0x2222)   # (a read past the row would differ)
    absent = int((~np.isin(rates, RATES)).sum())
    a, u = _ctx(ms, sub_batches=sub_batches, streams=streams), _ctx(ms, streams=streams)
    try:
        if serial:
            a.set_serial(True)
        a.set_encoder_sample_rate(32000)   # not read
        empty_on, full_on, empty_off = np.zeros(4, int), np.zeros(4, int), 0
        for t in range(T_HOPS):
            got = _streams_dev(a, ids, pcm_a[t], rates, bits, flags[t])
            want = _uniform(u, ids, pcm_u[t], rates, bits, flags[t])
            _check_rows(*got, *want, f"hop {t}")
            for i, r in enumerate(RATES):
                on = (rates == r) & (flags[t] != 0)
                empty_on[i] += int((want[1][on] == 0).sum())
                full_on[i] += int((want[1][on] != 0).sum())
            empty_off += int((want[1][np.isin(rates, RATES) & (flags[t] == 0)] == 0).sum())
        assert a.rates_errors() == absent * T_HOPS and a.encode_mixed_errors() == 0
        _same_state(a, u, ids, "after the last hop")
        print("flagged rows, empty / non-empty packets per rate:", empty_on, full_on, "unflagged rows, empty:", empty_off)
        if B == 37:   # the condition of the comparison, on the twin's output
            assert (empty_on > 0).all() and (full_on > 0).all(), (empty_on, full_on)
            assert tuple(empty_on) == _COND_CPU["noise"] and tuple(full_on) == _COND_CPU["not_noise"], (empty_on, full_on)
        assert empty_off == 0
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B,sub_batches,serial,streams", stream_cases([(37, None, False), (37, 2, False), (37, None, True),
                                                                       (5, None, False)], plain=(37, None, False)))
def test_per_row_dtx_equals_the_uniform_calls(golden_dir, B, sub_batches, serial, streams):
    _per_row_case(golden_dir, B, sub_batches, serial, streams)


# ---- 2. fixed flags -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("flag", ["zeros", "null", "ones"])
def test_fixed_flags_equal_encode_rates_dev(golden_dir, flag):
    B, T, ms = 37, 14, 64
    ids = _ids(B, ms, 3)
    rates = np.array([RATES[(b // 3) % 4] for b in range(B)], np.int32)
    bits = np.array([BITS[b % 3] for b in range(B)], np.int32)
    pcm = _pcm_rows(golden_dir, B, T, rates, 3, 7, 0)
    flags = {"zeros": np.zeros(B, np.int32), "null": None, "ones": np.ones(B, np.int32)}[flag]
    a, u = _ctx(ms), _ctx(ms)
    try:
        for t in range(T):
            got = _streams_dev(a, ids, pcm[t], rates, bits, flags)
            want = _uniform(u, ids, pcm[t], rates, bits, np.full(B, flag == "ones", np.int32))
            _check_rows(*got, *want, f"hop {t}")
        assert a.rates_errors() == 0
        _same_state(a, u, ids, flag)
    finally:
        a.close()
        u.close()


# ---- 3. packed rows -------------------------------------------------------------------------------------------------------

def _pack(pcm_t, rates, order=None):
    """-> (packed int16 [sum rate / 50], offsets [B]); rows laid back to back in `order` (default: row order)"""
    B = rates.size
    order = np.arange(B) if order is None else order
    offsets = np.zeros(B, np.int32)
    parts, pos = [], 0
    for b in order:
        n = int(rates[b]) // 50
        offsets[b] = pos
        parts.append(pcm_t[b, :n])
        pos += n
    return np.concatenate(parts).astype(np.int16), offsets


@pytest.mark.gpu
def test_packed_rows_equal_the_padded_layout(golden_dir):
    import torch
    B, T, ms = 37, 10, 64
    ids = _ids(B, ms, 5)
    rates = np.array([RATES[(b // 3) % 4] for b in range(B)], np.int32)
    bits = np.array([BITS[b % 3] for b in range(B)], np.int32)
    flags = _flags(B, T, np.full(B, -1, np.int32), 9)
    pcm = _pcm_rows(golden_dir, B, T, rates, 3, 2, 0x1111)   # the padded layout: gaps and tail poisoned
    order = np.random.default_rng(4).permutation(B)
    a, u = _ctx(ms), _ctx(ms)
    try:
        for t in range(T):
            packed, offsets = _pack(pcm[t], rates, order if t & 1 else None)
            buf = torch.full((packed.size + 2048,), 0x2222, dtype=torch.int16, device=_dev())   # poisoned behind the rows
            buf[:packed.size] = _t(packed)
            got = _streams_dev(a, ids, buf, rates, bits, flags[t], offsets=offsets, n_pcm=packed.size)
            want = _streams_dev(u, ids, pcm[t], rates, bits, flags[t])
            _check_rows(*got, *want, f"hop {t}")
        assert a.rates_errors() == 0 and u.rates_errors() == 0
        _same_state(a, u, ids, "packed")
    finally:
        a.close()
        u.close()


# ---- 4. invalid rows never fault ------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_invalid_rows_are_absent_and_counted(golden_dir):
    B, T, ms = 5, 12, 64
    ids = _ids(B, ms, 21)
    rates = np.array([8000, 16000, 48000, 32000, 16000], np.int32)
    bits = np.array([64, 120, 184, 64, 120], np.int32)
    flags = np.array([1, 1, 0, 0, 1], np.int32)
    bad_rows, good = np.array([1, 3]), np.array([0, 2, 4])
    pcm = _pcm_rows(golden_dir, B, T, rates, 3, 8, 0)
    a, u = _ctx(ms), _ctx(ms)
    try:
        before = a.export_streams(ids[bad_rows])
        for t in range(T):
            packed, offsets = _pack(pcm[t], rates)
            r = rates.copy()
            for k, b in enumerate(bad_rows):
                kind = (t + 2 * k) % 5
                if kind == 0:
                    r[b] = BAD_RATE
                elif kind == 1:
                    offsets[b] += 4                      # 8 bytes: inside the buffer, not a multiple of 16 bytes
                elif kind == 2:
                    offsets[b] = -8
                elif kind == 3:
                    offsets[b] = packed.size - 8         # starts inside, ends outside
                else:
                    offsets[b] = 2147483640              # far outside (a multiple of 8)
            got_pk, got_pb = _streams_dev(a, ids, packed, r, bits, flags, offsets=offsets)
            p2, o2 = _pack(pcm[t][good], rates[good])
            want_pk, want_pb = _streams_dev(u, ids[good], p2, rates[good], bits[good], flags[good], offsets=o2)
            assert (got_pb[bad_rows] == 0).all() and (got_pk[bad_rows] == SENTINEL).all(), f"hop {t}"
            _check_rows(got_pk[good], got_pb[good], want_pk, want_pb, f"hop {t}")
            assert a.rates_errors() == 2 * (t + 1), f"hop {t}"
        assert u.rates_errors() == 0
        assert np.array_equal(a.export_streams(ids[bad_rows]), before), "an absent row's stream advanced"
        _same_state(a, u, ids[good], "valid rows")
    finally:
        a.close()
        u.close()


# ---- 5. argument checks ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_argument_checks_enqueue_nothing(golden_dir):
    import torch
    B, ms = 5, 16
    ids = np.arange(B, dtype=np.int32)
    rates = np.array([8000, 16000, 32000, 48000, 16000], np.int32)
    bits = np.full(B, 184, np.int32)
    pcm = _pcm_rows(golden_dir, B, 2, rates, 0, 1, 0)
    a = _ctx(ms)
    try:
        _streams_dev(a, ids, pcm[0], rates, bits, np.ones(B, np.int32))
        state = a.export_streams(np.arange(ms, dtype=np.int32))
        big = ms + 1
        bufs = dict(ids=_t(np.arange(big, dtype=np.int32)), pcm=torch.zeros((big, ROW), dtype=torch.int16, device=_dev()),
                    off=_t(np.arange(big, dtype=np.int32) * ROW), rates=_t(np.full(big, 16000, np.int32)),
                    bits=_t(np.full(big, 184, np.int32)), dtx=_t(np.ones(big, np.int32)),
                    pk=torch.zeros((big, 23), dtype=torch.uint8, device=_dev()),
                    pb=torch.zeros(big, dtype=torch.int32, device=_dev()))
        p = {k: v.data_ptr() for k, v in bufs.items()}

        def call(B_=B, n=big * ROW, **null):
            g = lambda k: None if k in null else p[k]   # noqa: E731
            return a.L.lyra_hip_encode_streams_dev(a.h, g("ids"), B_, g("pcm"), n, g("off"), g("rates"), g("bits"), g("dtx"),
                                                   g("pk"), g("pb"))
        for k in ("ids", "pcm", "rates", "bits", "pk", "pb"):
            assert call(**{k: True}) == EINVAL, k
        assert call(B_=0) == EINVAL and call(B_=-1) == EINVAL and call(B_=big) == EINVAL
        assert call(n=-1) == EINVAL
        assert a.L.lyra_hip_encode_streams_dev(None, p["ids"], B, p["pcm"], big * ROW, None, p["rates"], p["bits"], None,
                                               p["pk"], p["pb"]) == EINVAL
        assert a.rates_errors() == 0 and a.encode_mixed_errors() == 0
        assert np.array_equal(a.export_streams(np.arange(ms, dtype=np.int32)), state)
        assert (bufs["pk"].cpu().numpy() == 0).all() and (bufs["pb"].cpu().numpy() == 0).all()
        assert call() == 0 and call(off=True) == 0 and call(dtx=True) == 0   # (the two optional pointers)
        a.synchronize()
    finally:
        a.close()


# ---- 6. host form ---------------------------------------------------------------------------------------------------------

def _want_host(u, ids, pcm_t, rates, bits, flags):
    """what end() must hand over: the `_dev` call on the same rows; bytes behind each packet zero"""
    pk, pb = _streams_dev(u, ids, pcm_t, rates, bits, flags)
    for b in range(pb.size):
        pk[b, pb[b]:] = 0
    return pk, pb


@pytest.mark.gpu
def test_begin_end_equals_the_dev_call(golden_dir):
    import lyra_amd
    import torch
    B, T, ms = 37, 16, 64
    rates, bits, fixed = _row_layout(B)
    rates[[5, 6]] = (32000, 32000)   # (begin() refuses an invalid rate: every row is present here)
    flags = _flags(B, T, fixed, 2)
    # the id list changes between requests in flight; a stream's rate belongs to the stream, so ids move inside rate groups
    base = _ids(B, ms, 40)
    ids_t = [base.copy() for _ in range(T)]
    for t in range(T):
        for r in RATES:
            sel = np.flatnonzero(rates == r)
            ids_t[t][sel] = base[np.random.default_rng(t // 3).permutation(sel)]
    pcm = _pcm_rows(golden_dir, B, T, rates, 3, 4, 0)
    a, u = _ctx(ms), _ctx(ms)
    try:
        want = []
        got = []

        def begin(t, how):
            packed, _ = _pack(pcm[t], rates)
            if how == "pinned":
                buf = torch.from_numpy(packed.copy()).pin_memory()
                a.encode_streams_begin(buf, rates, bits, flags[t], ids_t[t])
                buf.fill_(0x3333)        # the caller's buffer is the caller's again
            else:
                buf = packed.copy()
                a.encode_streams_begin(buf, rates, bits, flags[t], ids_t[t])
                buf[:] = 0x3333
            want.append(_want_host(u, ids_t[t], pcm[t], rates, bits, flags[t]))

        def end():
            got.append(a.encode_streams_end())

        with pytest.raises(lyra_amd.LyraHipError):
            a.encode_streams_end()                      # nothing in flight
        begin(0, "pageable")
        end()                                           # blocking use
        for t in range(1, T):
            begin(t, "pinned" if t & 1 else "pageable")
            if t == 1:
                continue
            if t == 6:   # two in flight: every refusal leaves them, and the streams, as they are
                packed, _ = _pack(pcm[t], rates)
                with pytest.raises(lyra_amd.LyraHipError):
                    a.encode_streams_begin(packed, rates, bits, flags[t], ids_t[t])        # a third
                with pytest.raises(lyra_amd.LyraHipError):
                    a.encode_begin(np.zeros((2, 320), np.int16), 184)                      # the other pipeline
                with pytest.raises(lyra_amd.LyraHipError):
                    a.export_streams(ids_t[t])
                with pytest.raises(lyra_amd.LyraHipError):
                    a.import_streams(ids_t[t][:1], np.zeros((1, a.stream_blob_bytes()), np.uint8))
                assert len(a._pending_stream_encodes) == 2
            end()
        end()
        for t in range(T):
            assert np.array_equal(got[t][1], want[t][1]), f"hop {t}"
            assert np.array_equal(got[t][0], want[t][0]), f"hop {t}"
        assert (np.concatenate([g[1] for g in got]) == 0).any(), "no empty packet was read back"

        # host checks of begin(): nothing enqueued, nothing changed
        packed, _ = _pack(pcm[0], rates)
        ok = (rates, bits, flags[0], ids_t[0])

        def refused(rates_=ok[0], bits_=ok[1], ids_=ok[3]):
            with pytest.raises(lyra_amd.LyraHipError):
                a.encode_streams_begin(packed, rates_, bits_, ok[2], ids_)
            assert not a._pending_stream_encodes
        for bad in (BAD_RATE, 0, -16000):
            r2 = rates.copy(); r2[B - 1] = bad
            refused(rates_=r2)
        for bad in (0, 2, 188, -4, 63):
            b2 = bits.copy(); b2[B - 1] = bad
            refused(bits_=b2)
        i2 = ids_t[0].copy(); i2[3] = i2[4]
        refused(ids_=i2)
        i2 = ids_t[0].copy(); i2[0] = ms
        refused(ids_=i2)
        i2[0] = -1
        refused(ids_=i2)
        with pytest.raises(lyra_amd.LyraHipError):
            a.encode_streams_end()
        # the other pipeline in flight refuses this one
        a.encode_begin(np.zeros((2, 320), np.int16), 184, stream_ids=np.setdiff1d(np.arange(ms), base)[:2].astype(np.int32))
        refused()
        a.encode_end()
        assert a.rates_errors() == 0 and a.encode_mixed_errors() == 0
        _same_state(a, u, base, "after the refusals")
        # ... and a hop after them is still the twin's
        begin(0, "pageable")
        end()
        assert np.array_equal(got[-1][0], want[-1][0]) and np.array_equal(got[-1][1], want[-1][1])
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
def test_a_larger_batch_begun_behind_one_in_flight(golden_dir):
    """Batches of 2, 5 and max_streams = 8 rows, each begun while the one before is in flight: the scratch grows under a request
    in flight, and at 8 rows the last row of every array of the slot borders the next array.  Against the `_dev` call."""
    ms, sizes = 8, (2, 5, 8)
    rates = np.array([48000, 8000, 16000, 32000, 8000, 48000, 16000, 32000], np.int32)
    bits = np.array([184, 64, 120, 184, 64, 120, 184, 64], np.int32)
    flags = np.array([1, 0, 1, 0, 0, 1, 1, 1], np.int32)
    pcm = _pcm_rows(golden_dir, ms, len(sizes), rates, 0, 6, 0)
    a, u = _ctx(ms), _ctx(ms)
    try:
        ids = np.arange(ms, dtype=np.int32)
        want = [_want_host(u, ids[:B], pcm[k][:B], rates[:B], bits[:B], flags[:B]) for k, B in enumerate(sizes)]
        got = []
        for k, B in enumerate(sizes):
            a.encode_streams_begin(_pack(pcm[k][:B], rates[:B])[0], rates[:B], bits[:B], flags[:B], ids[:B])
            if k:
                got.append(a.encode_streams_end())
        got.append(a.encode_streams_end())
        for k in range(len(sizes)):
            assert np.array_equal(got[k][1], want[k][1]) and np.array_equal(got[k][0], want[k][0]), f"request {k}"
        assert a.rates_errors() == 0 and a.encode_mixed_errors() == 0
        _same_state(a, u, ids, "after the last request")
    finally:
        a.close()
        u.close()


# ---- 7. the class against the reference model -----------------------------------------------------------------------------

BITRATE_BITS = {3200: 64, 6000: 120, 9200: 184}


def _session():
    """8 streams = four rates x DTX off / on, 40 hops; bitrates switch per stream on a script -> (params, switches)."""
    params = [(RATES[s // 2], (3200, 6000, 9200)[s % 3], s & 1) for s in range(8)]
    rng = np.random.default_rng(77)
    switches = sorted((int(rng.integers(1, T_HOPS)), int(rng.integers(0, 8)), int(rng.choice((3200, 6000, 9200))))
                      for _ in range(24))
    switches.append((0, 6, 9200))   # before the first hop
    return params, sorted(switches)


@pytest.fixture(scope="module")
def session_reference(golden_dir, oracle_default):
    """The session's audio and what RefLyraEncoder(rate, bits, dtx) per stream makes of it: computed once."""
    from oracle import lyra_codec_model as M
    params, switches = _session()
    pcm = _speech(golden_dir, 8, T_HOPS, offset=9)
    pcm[5:30, [1, 2, 3, 5, 7]] = 0        # the DTX streams (odd) and one stream without DTX fall silent, then speak again
    pcm[12:20, 4] = 0
    rows = [[np.repeat(pcm[t, s], r // 16000) if r >= 16000 else pcm[t, s, ::2] for s, (r, _, _) in enumerate(params)]
            for t in range(T_HOPS)]
    encs = [M.RefLyraEncoder(oracle_default, r, BITRATE_BITS[br], bool(dtx)) for r, br, dtx in params]
    want_pk = np.zeros((T_HOPS, 8, 23), np.uint8)
    want_len = np.zeros((T_HOPS, 8), np.int32)
    for t in range(T_HOPS):
        for hop, s, br in switches:
            if hop == t:
                encs[s].bits = BITRATE_BITS[br]
        for s in range(8):
            p = encs[s].Encode(rows[t][s])
            want_len[t, s] = p.size
            want_pk[t, s, :p.size] = p
    packed = np.concatenate([np.concatenate(rows[t]) for t in range(T_HOPS)]).astype(np.int16)
    return params, switches, packed, want_pk, want_len


@pytest.mark.gpu
def test_mixed_batch_encoder_equals_the_reference_model(tmp_path, session_reference):
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "mixed_encoder_demo")
    assert os.path.exists(demo), "lyra_amd/mixed_encoder_demo not built (__graft_entry__.build())"
    params, switches, packed, want_pk, want_len = session_reference
    (tmp_path / "params.txt").write_text("".join(f"{r} {br} {dtx}\n" for r, br, dtx in params))
    (tmp_path / "switches.txt").write_text("".join(f"{h} {s} {br}\n" for h, s, br in switches))
    packed.tofile(tmp_path / "in.s16")
    runs = []
    for mode in ("0", "1"):
        pk, ln = tmp_path / f"pk{mode}.bin", tmp_path / f"len{mode}.i32"
        r = subprocess.run([demo, lyra_amd.default_model_dir(), str(tmp_path / "params.txt"), str(tmp_path / "switches.txt"),
                            str(tmp_path / "in.s16"), str(pk), str(ln)], capture_output=True, text=True, timeout=120,
                           env=dict(os.environ, LYRA_DEMO_PIPELINED=mode))
        assert r.returncode == 0, (mode, r.returncode, r.stderr[-3000:])
        runs.append((np.fromfile(pk, np.uint8).reshape(T_HOPS, 8, 23), np.fromfile(ln, np.int32).reshape(T_HOPS, 8)))
    for mode, (got_pk, got_len) in enumerate(runs):
        assert np.array_equal(got_len, want_len), (mode, np.argwhere(got_len != want_len)[:8])
        assert np.array_equal(got_pk, want_pk), (mode, np.argwhere((got_pk != want_pk).any(axis=2))[:8])
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    # the session exercised what it is about: empty packets only from DTX streams, at every rate; all three sizes per stream class
    dtx = np.array([p[2] for p in params], bool)
    assert (want_len[:, dtx] == 0).any(axis=0).all() and not (want_len[:, ~dtx] == 0).any()
    assert set(np.unique(want_len)) == {0, 8, 15, 23}
