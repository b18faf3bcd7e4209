"""The two-deep pipelined host-buffer calls (include/lyra_hip.h "Pipelined host-buffer calls"; BatchLyraEncoder::EncodeAsync /
WaitEncoded, BatchLyraDecoder::DecodeSamplesAsync / WaitDecoded) on the GPU: same kernels in the same order per stream, so
every packet and every decoded sample must equal what the blocking calls give -- over scripted sessions with packet loss,
DTX, odd request sizes and all four sample rates -- and the C ABI's begin / end pair must equal lyra_hip_encode."""
import ctypes as C
import os

import numpy as np
import pytest

from sessions import _run_session, _session

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("rate,bitrate,dtx", [(16000, 9200, False), (48000, 6000, True), (8000, 3200, False), (32000, 9200, True)])
def test_pipelined_twins_equal_the_blocking_twins(tmp_path, golden_dir, rate, bitrate, dtx):
    pcm, script = _session(golden_dir, rate, bitrate)
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    pa, la, oa = _run_session(tmp_path / "a", None, rate, bitrate, dtx, pcm, script)
    pb, lb, ob = _run_session(tmp_path / "b", None, rate, bitrate, dtx, pcm, script, pipelined=True)
    assert np.array_equal(la, lb) and np.array_equal(pa, pb), "packets differ between the blocking and the pipelined session"
    assert oa.size == ob.size and np.array_equal(oa, ob), "decoded samples differ between the blocking and the pipelined session"


@pytest.mark.parametrize("sub_batches", [1, 2])
def test_c_abi_encode_begin_end_equals_encode_and_enforces_two_in_flight(sub_batches):
    """sub_batches = 2: the context splits a batch over two extractor / quantizer stream pairs (LYRA_HIP_SUBBATCHES); the
    pipelined call orders its upload in front of, and its download behind, every chunk."""
    import lyra_amd
    from lyra_amd import codec
    L = codec._load()
    vp = C.c_void_p
    B, T, bits = 300, 7, 184
    rng = np.random.Generator(np.random.PCG64(31))
    pcm = rng.integers(-20000, 20000, size=(T, B, 320)).astype(np.int16)
    ids = np.arange(B, dtype=np.int32)[::-1].copy()
    a = lyra_amd.LyraHip(max_streams=512)
    b = lyra_amd.LyraHip(max_streams=512, sub_batches=sub_batches)
    try:
        want = [a.encode(pcm[t], bits, ids) for t in range(T)]
        p = lambda x: x.ctypes.data_as(vp)
        h = b.h if hasattr(b, "h") else b.ctx
        got = []
        out = np.empty((B, 23), np.uint8)
        lens = np.empty(B, np.int32)
        assert L.lyra_hip_encode_end(h, p(out), p(lens)) != 0                     # nothing in flight
        assert L.lyra_hip_encode_begin(h, p(ids), B, p(pcm[0]), 16000, bits, 0) == 0
        for t in range(T):
            if t + 1 < T:
                assert L.lyra_hip_encode_begin(h, p(ids), B, p(pcm[t + 1]), 16000, bits, 0) == 0
                if t == 0:
                    assert L.lyra_hip_encode_begin(h, p(ids), B, p(pcm[t + 1]), 16000, bits, 0) != 0   # a third one is refused
            assert L.lyra_hip_encode_end(h, p(out), p(lens)) == 0
            assert (lens == 23).all()
            got.append(out.copy())
        for t in range(T):
            assert np.array_equal(got[t], want[t]), f"hop {t}"
        # ... and the Python mirror of the pair (lyra_amd/codec.py), at 48 kHz with DTX, against the blocking calls
        a.reset(); b.reset()
        a.set_encoder_sample_rate(48000)
        p48 = rng.integers(-20000, 20000, size=(4, B, 960)).astype(np.int16)
        p48[:, :7] //= 2000          # a few streams are noise: DTX sends empty packets for them
        b.encode_begin(p48[0], bits, ids, sample_rate_hz=48000, dtx=True)
        for t in range(4):
            if t + 1 < 4:
                b.encode_begin(p48[t + 1], bits, ids, sample_rate_hz=48000, dtx=True)
            pk, lens = b.encode_end()
            p16 = a.resample(p48[t], 48000, 16000, ids, side="encoder")
            want_pk, want_len = a.encode_dtx(p16, bits, ids)
            assert np.array_equal(lens, want_len) and np.array_equal(pk, want_pk), f"48 kHz DTX hop {t}"
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("sub_batches", [1, 2])
def test_c_abi_decode_begin_end_equals_decode(sub_batches):
    """lyra_hip_decode_begin / _end (through the Python mirror), two deep, against lyra_hip_decode on a second context: the
    same PCM hop for hop, state carried; a third begin is refused, an end without a begin too."""
    import lyra_amd
    B, T, bits = 700, 8, 120
    rng = np.random.Generator(np.random.PCG64(77))
    pcm = rng.integers(-20000, 20000, size=(T, B, 320)).astype(np.int16)
    ids = np.arange(B, dtype=np.int32)
    enc = lyra_amd.LyraHip(max_streams=1024)
    a = lyra_amd.LyraHip(max_streams=1024)
    b = lyra_amd.LyraHip(max_streams=1024, sub_batches=sub_batches)
    try:
        packets = [enc.encode(pcm[t], bits, ids) for t in range(T)]
        want = [a.decode(packets[t], bits, ids) for t in range(T)]
        with pytest.raises(Exception):
            b._pending_decodes = [B]
            b.decode_end()
        b._pending_decodes = []
        b.decode_begin(packets[0], bits, ids)
        for t in range(T):
            if t + 1 < T:
                b.decode_begin(packets[t + 1], bits, ids)
                if t == 0:
                    with pytest.raises(Exception):
                        b.decode_begin(packets[t + 1], bits, ids)     # a third call in flight is refused
            got = b.decode_end()
            assert np.array_equal(got, want[t]), f"hop {t}"
    finally:
        enc.close(); a.close(); b.close()


@pytest.mark.parametrize("sub_batches", [1, 2])
def test_pipelined_calls_with_stream_ids_that_change_every_hop(sub_batches):
    """Every hop lists the streams in another order (and the small id / packet buffers of a slot are rewritten while the
    previous call's kernels run): a call that read a slot's ids or packets from before its own upload would mix streams up.
    Encode and decode, two deep, against the blocking calls given the same orders."""
    import lyra_amd
    B, T, bits = 700, 8, 120
    rng = np.random.Generator(np.random.PCG64(5))
    pcm = rng.integers(-20000, 20000, size=(T, B, 320)).astype(np.int16)
    orders = [rng.permutation(B).astype(np.int32) for _ in range(T)]
    a = lyra_amd.LyraHip(max_streams=1024)
    b = lyra_amd.LyraHip(max_streams=1024, sub_batches=sub_batches)
    try:
        want_pk = [a.encode(pcm[t][orders[t]], bits, orders[t]) for t in range(T)]
        want_pcm = [a.decode(want_pk[t], bits, orders[t]) for t in range(T)]
        got_pk = []
        b.encode_begin(pcm[0][orders[0]], bits, orders[0])
        for t in range(T):
            if t + 1 < T:
                b.encode_begin(pcm[t + 1][orders[t + 1]], bits, orders[t + 1])
            got_pk.append(b.encode_end()[0])
        for t in range(T):
            assert np.array_equal(got_pk[t], want_pk[t]), f"packets of hop {t}"
        got_pcm = []
        b.decode_begin(want_pk[0], bits, orders[0])
        for t in range(T):
            if t + 1 < T:
                b.decode_begin(want_pk[t + 1], bits, orders[t + 1])
            got_pcm.append(b.decode_end())
        for t in range(T):
            assert np.array_equal(got_pcm[t], want_pcm[t]), f"PCM of hop {t}"
    finally:
        a.close(); b.close()


def test_a_larger_batch_begun_behind_one_in_flight():
    """Batches of 2, 5 and max_streams = 8 rows, each begun while the one before is in flight: the scratch grows under a request
    in flight, and at 8 rows the last row of every array of a slot borders the next array.  Encode (48 kHz, so the slot's
    external-rate and 16 kHz rows are both in use) and decode, against the blocking calls on a second context."""
    import lyra_amd
    ms, bits, sizes = 8, 184, (2, 5, 8)
    rng = np.random.Generator(np.random.PCG64(11))
    p48 = [rng.integers(-20000, 20000, size=(B, 960)).astype(np.int16) for B in sizes]
    a, b = lyra_amd.LyraHip(max_streams=ms), lyra_amd.LyraHip(max_streams=ms)
    try:
        ids = [np.arange(B, dtype=np.int32) for B in sizes]
        want_pk = [a.encode(a.resample(p48[k], 48000, 16000, ids[k], side="encoder"), bits, ids[k]) for k in range(3)]
        want_pcm = [a.decode(want_pk[k], bits, ids[k]) for k in range(3)]
        got_pk, got_pcm = [], []
        for k in range(3):
            b.encode_begin(p48[k], bits, ids[k], sample_rate_hz=48000)
            if k:
                got_pk.append(b.encode_end())
        got_pk.append(b.encode_end())
        for k in range(3):
            b.decode_begin(want_pk[k], bits, ids[k])
            if k:
                got_pcm.append(b.decode_end())
        got_pcm.append(b.decode_end())
        for k in range(3):
            assert (got_pk[k][1] == bits // 8).all() and np.array_equal(got_pk[k][0], want_pk[k]), f"packets of request {k}"
            assert np.array_equal(got_pcm[k], want_pcm[k]), f"PCM of request {k}"
    finally:
        a.close(); b.close()


def test_twin_fetch_with_a_larger_batch_begun_behind_one_in_flight():
    """lyra_hip_twin_fetch_begin / _end (the C calls: only the C++ classes drive them otherwise) on a fresh context: requests
    of 2, 5 and max_streams = 8 decoded hops at 48 kHz, each assembled and begun while the one before is in flight, so the
    twin's row buffers grow under a request in flight.  Against lyra_hip_twin_fetch on a second context."""
    import lyra_amd

    class Slice(C.Structure):
        _fields_ = [(n, C.c_int32) for n in ("id", "gan_off", "gen_n", "cng_off", "cng_n", "fade", "fade_dir", "out_off",
                                             "noise_row")]
    vp, ci = C.c_void_p, C.c_int
    rate, calls = 48000, [(2, 320), (5, 320), (8, 160)]
    a, u = lyra_amd.LyraHip(max_streams=8), lyra_amd.LyraHip(max_streams=8)
    try:
        for L in (a.L, u.L):
            L.lyra_hip_twin_decode.argtypes = [vp, vp, ci, vp, ci]
            L.lyra_hip_twin_assemble.argtypes = [vp, vp, ci, ci]
            L.lyra_hip_twin_fetch.argtypes = [vp, ci, ci, ci, vp]
            L.lyra_hip_twin_fetch_begin.argtypes = [vp, ci, ci, ci]
            L.lyra_hip_twin_fetch_end.argtypes = [vp, vp]

        packets = np.random.Generator(np.random.PCG64(3)).integers(0, 256, size=(len(calls), 8, 23)).astype(np.uint8)

        def assemble(ctx, k, B, n):
            ids = np.arange(B, dtype=np.int32)
            assert ctx.L.lyra_hip_twin_decode(ctx.h, ids.ctypes.data, B, packets[k].ctypes.data, 184) == 0, ctx.last_error()
            sl = (Slice * B)(*[Slice(b, 0, n, 0, 0, 0, 1, 0, -1) for b in range(B)])
            assert ctx.L.lyra_hip_twin_assemble(ctx.h, C.addressof(sl), B, n) == 0, ctx.last_error()

        want = [np.zeros((B, 3 * n), np.int16) for B, n in calls]
        got = [np.full((B, 3 * n), 0x3333, np.int16) for B, n in calls]
        for k, (B, n) in enumerate(calls):
            assemble(u, k, B, n)
            assert u.L.lyra_hip_twin_fetch(u.h, B, n, rate, want[k].ctypes.data) == 0, u.last_error()
        assert a.L.lyra_hip_twin_fetch_end(a.h, got[0].ctypes.data) != 0          # nothing in flight
        for k, (B, n) in enumerate(calls):
            assemble(a, k, B, n)
            assert a.L.lyra_hip_twin_fetch_begin(a.h, B, n, rate) == 0, a.last_error()
            if k:
                assert a.L.lyra_hip_twin_fetch_end(a.h, got[k - 1].ctypes.data) == 0, a.last_error()
        assert a.L.lyra_hip_twin_fetch_end(a.h, got[-1].ctypes.data) == 0, a.last_error()
        for k in range(len(calls)):
            assert want[k].any(), f"request {k}: the blocking twin delivered silence"
            assert np.array_equal(got[k], want[k]), f"request {k}"
    finally:
        a.close(); u.close()
