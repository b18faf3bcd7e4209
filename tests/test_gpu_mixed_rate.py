"""Per-stream sample rates on the device path: lyra_hip_encode_rates_dev, lyra_hip_decode_lossy_rates_dev and
LYRA_HIP_STEP_MIXED_RATE.  Expectation: the existing uniform calls (encode_mixed_dev after set_encoder_sample_rate,
decode_lossy_mixed_dev) on a second context fed the same audio, one call per rate on that rate's id subset -- bit for bit,
packets and every decoder output; run_steps against the single calls."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_plumbing import _dev, _ids, _t, make_ctx as _ctx
from receiver_models import LossyModel
from row_cases import ROW, SENTINEL, _check_sentinel_rows as _check_rows, _decode_rates, _draw_bits, _rates
from signals import RATES, _gilbert, _pcm_rows, _random_packets as _packets

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))


def _encode_uniform(u, ids, pcm_t, rates, bits, dtx):
    """encode_mixed_dev once per rate on that rate's id subset -> (packets [B][23], packet_bytes [B]); rows of other rates: 0."""
    import torch
    B = ids.size
    pk = np.zeros((B, 23), np.uint8)
    pb = np.zeros(B, np.int32)
    for r in RATES:
        sel = np.flatnonzero(rates == r)
        if not sel.size:
            continue
        if dtx:
            u.set_encoder_sample_rate(r)
        d_pk = torch.zeros((sel.size, 23), dtype=torch.uint8, device=_dev())
        d_pb = torch.full((sel.size,), -7, dtype=torch.int32, device=_dev())
        u.encode_mixed_dev(_t(ids[sel]), _t(pcm_t[sel, :r // 50]), r, _t(bits[sel]), d_pk, d_pb, dtx=dtx)
        u.synchronize()
        pk[sel], pb[sel] = d_pk.cpu().numpy(), d_pb.cpu().numpy()
    return pk, pb


def _encode_rates(a, ids, pcm_t, rates, bits, dtx):
    import torch
    B = ids.size
    d_pk = torch.full((B, 23), SENTINEL, dtype=torch.uint8, device=_dev())
    d_pb = torch.full((B,), -7, dtype=torch.int32, device=_dev())
    a.encode_rates_dev(_t(ids), _t(pcm_t), _t(rates), _t(bits), d_pk, d_pb, dtx=dtx)
    a.synchronize()
    return d_pk.cpu().numpy(), d_pb.cpu().numpy()


def _encode_case(golden_dir, B, dtx, serial):
    T = 8 if B > 64 else 40
    ms = 4096 if B > 64 else 64
    ids = _ids(B, ms, B + 5)
    rates = _rates(B) if B > 1 else np.array([48000], np.int32)
    pcm_a = _pcm_rows(golden_dir, B, T, rates, 3 if dtx else 0, B, 0x1111)
    pcm_u = _pcm_rows(golden_dir, B, T, rates, 3 if dtx else 0, B, 0x2222)   # (a read past the row would differ)
    rng = np.random.default_rng(B + dtx)
    a, u = _ctx(ms), _ctx(ms)
    try:
        if serial:
            a.set_serial(True)
        a.set_encoder_sample_rate(32000)   # not read by the per-row call
        empty, full = np.zeros(4, int), np.zeros(4, int)
        for t in range(T):
            bits = _draw_bits(rng, B)
            got_pk, got_pb = _encode_rates(a, ids, pcm_a[t], rates, bits, dtx)
            want_pk, want_pb = _encode_uniform(u, ids, pcm_u[t], rates, bits, dtx)
            _check_rows(got_pk, got_pb, want_pk, want_pb, f"hop {t}")
            if t > 5:
                for i, r in enumerate(RATES):
                    empty[i] += int((want_pb[rates == r] == 0).sum())
                    full[i] += int((want_pb[rates == r] != 0).sum())
        assert a.rates_errors() == 0 and a.encode_mixed_errors() == 0
        print("DTX empty / non-empty packets per rate after hop 5:", empty, full)
        if dtx and B == 17:   # the estimator-per-row path must have decided both ways at every rate
            assert (empty > 0).all() and (full > 0).all(), (empty, full)
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B,dtx,serial", [(4096, False, False), (4096, True, False), (4096, True, True), (4096, False, True),
                                          (17, False, False), (17, True, False), (1, True, False), (1, False, False)])
def test_encode_rates_equals_uniform_calls(golden_dir, B, dtx, serial):
    _encode_case(golden_dir, B, dtx, serial)


def _decode_uniform(u, ids, pk_t, sz_t, rates):
    import torch
    B = ids.size
    out16 = np.zeros((B, 320), np.int16)
    ext = np.zeros((B, ROW), np.int16)
    noise, cn = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for r in RATES:
        sel = np.flatnonzero(rates == r)
        if not sel.size:
            continue
        n = r // 50
        d16 = torch.zeros((sel.size, 320), dtype=torch.int16, device=_dev())
        dx = torch.zeros((sel.size, n), dtype=torch.int16, device=_dev())
        dn = torch.full((sel.size,), -3, dtype=torch.int32, device=_dev())
        dc = torch.full((sel.size,), -3, dtype=torch.int32, device=_dev())
        u.decode_lossy_mixed_dev(_t(ids[sel]), _t(pk_t[sel]), _t(sz_t[sel]), r, d16, dx, dn, dc)
        u.synchronize()
        out16[sel], noise[sel], cn[sel] = d16.cpu().numpy(), dn.cpu().numpy(), dc.cpu().numpy()
        ext[sel, :n] = dx.cpu().numpy() if r != 16000 else d16.cpu().numpy()
    return out16, ext, noise, cn


def _check_decode(got, want, rates, where):
    g16, gx, gn, gc = got
    w16, wx, wn, wc = want
    assert np.array_equal(g16, w16), where
    assert np.array_equal(gc, wc), where
    for b, r in enumerate(rates):
        n = r // 50 if r in RATES else 0
        assert np.array_equal(gx[b, :n], wx[b, :n]), (where, b, r)
        assert (gx[b, n:] == 0x3333).all(), (where, b, r, "samples past rate / 50 were written")
        if r == 16000:
            assert np.array_equal(gx[b, :320], g16[b]), (where, b)
    # is_noise is left alone on ticks without a packet: both calls start from -3 there
    assert np.array_equal(gn, wn), where


def _decode_case(B, serial):
    T = 8 if B > 64 else 40
    ms = 4096 if B > 64 else 64
    ids = _ids(B, ms, B + 9)
    rates = _rates(B) if B > 1 else np.array([8000], np.int32)
    pk, sz = _packets(np.random.default_rng(B), T, B)
    if B > 1:
        sz[2:14, :min(B, 12)] = 0   # >= 5 consecutive losses in every rate group (rows 0..11 cover the four rates) ...
        sz[14:24, :min(B, 12)] = 23  # ... and packets again: the fade back
    a, u = _ctx(ms), _ctx(ms)
    try:
        if serial:
            a.set_serial(True)
        cn = np.zeros((T, B), np.int32)
        for t in range(T):
            got = _decode_rates(a, ids, pk[t], sz[t], rates)
            want = _decode_uniform(u, ids, pk[t], sz[t], rates)
            _check_decode(got, want, rates, f"tick {t}")
            cn[t] = got[3]
        assert a.rates_errors() == 0
        if B >= 17 and T >= 40:   # every rate group went to comfort noise and came back
            for r in RATES:
                g = cn[:, rates == r]
                assert ((g[:-1] == 1) & (g[1:] == 0)).any(), (r, "no fade back from comfort noise")
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B,serial", [(4096, False), (4096, True), (17, False), (1, False)])
def test_decode_lossy_rates_equals_uniform_calls(B, serial):
    _decode_case(B, serial)


_CHILD = """
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_mixed_rate as T
T._encode_case(sys.argv[3], 4096, False, False)
T._encode_case(sys.argv[3], 4096, True, False)
T._decode_case(4096, False)
T._random_sequence(sys.argv[3], 2)
print("child ok")
"""


@pytest.mark.gpu
def test_split_context(golden_dir):
    """LYRA_HIP_SUBBATCHES=2 (read at context creation, hence a child process): the encode and decode comparisons at
    B = 4096 and the random call sequence."""
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, HERE, golden_dir], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, LYRA_HIP_SUBBATCHES="2"))
    assert r.returncode == 0 and "child ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


@pytest.mark.gpu
def test_state_is_interchangeable_with_the_uniform_calls(golden_dir):
    """Hop by hop alternately the per-row call and the uniform call at the streams' rate == the uniform-only session."""
    B, T = 6, 24
    for r in RATES:
        rates = np.full(B, r, np.int32)
        ids = _ids(B, 64, r)
        pcm = _pcm_rows(golden_dir, B, T, rates, 3, r % 97, 0)
        pk, sz = _packets(np.random.default_rng(r), T, B)
        rng = np.random.default_rng(1)
        a, u = _ctx(64), _ctx(64)
        try:
            for t in range(T):
                bits = _draw_bits(rng, B)
                per_row = t % 2 == 0
                got_e = (_encode_rates if per_row else _encode_uniform)(a, ids, pcm[t], rates, bits, True)
                want_e = _encode_uniform(u, ids, pcm[t], rates, bits, True)
                assert np.array_equal(got_e[1], want_e[1]), (r, t)
                for b in range(B):
                    assert np.array_equal(got_e[0][b, :want_e[1][b]], want_e[0][b, :want_e[1][b]]), (r, t, b)
                want_d = _decode_uniform(u, ids, pk[t], sz[t], rates)
                if per_row:
                    _check_decode(_decode_rates(a, ids, pk[t], sz[t], rates), want_d, rates, (r, t))
                else:
                    got_d = _decode_uniform(a, ids, pk[t], sz[t], rates)
                    assert all(np.array_equal(x, y) for x, y in zip(got_d, want_d)), (r, t)
        finally:
            a.close()
            u.close()


@pytest.mark.gpu
def test_against_the_reference_model(golden_dir, oracle_default):
    """16 streams, 4 per rate, 60 hops, DTX on, a long loss burst, bitrates switching at hop 20: packets byte for byte
    against RefLyraEncoder created at each stream's rate; the decoder under test_gpu_lossy_decode.LossyModel's criteria."""
    import torch
    from oracle import lyra_codec_model as M
    B, T = 16, 60
    ids = _ids(B, 64, 13)
    rates = np.repeat(np.array(RATES, np.int32), 4)
    pcm = _pcm_rows(golden_dir, B, T, rates, 3, 9, 0)
    rng = np.random.default_rng(4)
    sched = np.empty((T, B), np.int32)
    sched[:] = rng.choice((64, 120, 184), size=B)
    sched[20:] = rng.choice((64, 120, 184), size=B)
    rx = _gilbert(np.random.default_rng(5), T, B)
    rx[30:44, 1::4] = 0   # the long burst: comfort noise and back, one stream of every rate
    encs = [M.RefLyraEncoder(oracle_default, int(rates[s]), int(sched[0, s]), True) for s in range(B)]
    models = {r: LossyModel(oracle_default, r, ids[rates == r]) for r in RATES}
    a = _ctx(64)
    try:
        dn = torch.zeros(B, dtype=torch.int32, device=_dev())
        for t in range(T):
            pk, pb = _encode_rates(a, ids, pcm[t], rates, sched[t], True)
            for s, enc in enumerate(encs):
                enc.bits = int(sched[t, s])
                want = enc.Encode(pcm[t, s, :rates[s] // 50])
                assert pb[s] == want.size and np.array_equal(pk[s, :want.size], want), (t, s)
            mask = rx[t].astype(bool) & (pb > 0)
            got = _decode_rates(a, ids, pk, pb * mask, rates, dn=dn)
            for r in RATES:
                sel = rates == r
                models[r].tick(t, [pk[s, :pb[s]] for s in np.flatnonzero(sel)], mask[sel],
                               (got[0][sel], got[1][sel, :r // 50], got[2][sel], got[3][sel]))
        for r in RATES:
            assert models[r].saw_cn > 0 and models[r].saw_back > 0, r
            models[r].tally.report(f"{r} Hz")
    finally:
        a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtx", [True, False])
def test_invalid_rates_are_counted_and_leave_the_stream_alone(golden_dir, dtx):
    """Rows with 0 / 44100 / -1: counted exactly, no packet, other rows as in a run without them; fed validly afterwards
    the stream continues like one that skipped the hop.  Decoder: the tick runs, the external-rate row stays unwritten."""
    B, T = 12, 10
    ids = _ids(B, 64, 3)
    rates = _rates(B)
    bad_hop, bad_rows, bad_vals = 4, [1, 6, 10], [0, 44100, -1]
    pcm = _pcm_rows(golden_dir, B, T, rates, 0, 1, 0)
    pk, sz = _packets(np.random.default_rng(8), T, B)
    bits = np.full(B, 184, np.int32)
    a, u = _ctx(64), _ctx(64)
    try:
        for t in range(T):
            r_t = rates.copy()
            if t == bad_hop:
                r_t[bad_rows] = bad_vals
            got_pk, got_pb = _encode_rates(a, ids, pcm[t], r_t, bits, dtx)
            keep = np.ones(B, bool)
            if t == bad_hop:
                keep[bad_rows] = False
            w_pk, w_pb = _encode_uniform(u, ids[keep], pcm[t][keep], rates[keep], bits[keep], dtx)   # the rows skip the hop
            assert np.array_equal(got_pb[keep], w_pb), t
            assert (got_pb[~keep] == 0).all() and (got_pk[~keep] == SENTINEL).all()
            for g, w, n in zip(got_pk[keep], w_pk, w_pb):
                assert np.array_equal(g[:n], w[:n]), t
            r_d = rates.copy()
            if t == T - 1:   # (the decoder's last tick: its resampler of those rows does not run)
                r_d[bad_rows] = bad_vals
            got = _decode_rates(a, ids, pk[t], sz[t], r_d)
            want = _decode_uniform(u, ids, pk[t], sz[t], rates)
            _check_decode(got, want, r_d, f"tick {t}")
        assert a.rates_errors() == 6          # three rows, both sides
        assert a.rates_errors(clear=True) == 6 and a.rates_errors() == 0
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
def test_invalid_then_valid_back_to_back_without_dtx(golden_dir):
    """Without DTX the quantizer's mask is the call's id list: rows invalid on every other hop, 12 hops enqueued without a
    synchronize in between (the quantizer of hop t runs under hop t + 1's resampler), at the full batch so that the
    kernels overlap.  Every hop's packets must be that hop's."""
    import torch
    B, T, ms = 4096, 12, 4096
    ids, rates = _ids(B, ms, 77), _rates(B)
    bad = np.arange(B) % 5 == 2
    pcm = _pcm_rows(golden_dir, B, T, rates, 0, 2, 0)
    bits = np.full(B, 184, np.int32)
    a, u = _ctx(ms), _ctx(ms)
    try:
        d_ids, d_bits = _t(ids), _t(bits)
        r_bad = rates.copy()
        r_bad[bad] = 44100
        d_r = [_t(rates), _t(r_bad)]
        d_pcm = _t(pcm)
        d_pk = [torch.full((B, 23), SENTINEL, dtype=torch.uint8, device=_dev()) for _ in range(T)]
        d_pb = [torch.full((B,), -7, dtype=torch.int32, device=_dev()) for _ in range(T)]
        for t in range(T):
            a.encode_rates_dev(d_ids, d_pcm[t], d_r[t & 1], d_bits, d_pk[t], d_pb[t], dtx=False)
        a.synchronize()
        for t in range(T):
            keep = ~bad if t & 1 else np.ones(B, bool)
            w_pk, w_pb = _encode_uniform(u, ids[keep], pcm[t][keep], rates[keep], bits[keep], False)
            got_pk, got_pb = d_pk[t].cpu().numpy(), d_pb[t].cpu().numpy()
            assert np.array_equal(got_pb[keep], w_pb) and np.array_equal(got_pk[keep], w_pk), t
            assert (got_pb[~keep] == 0).all() and (got_pk[~keep] == SENTINEL).all(), t
        assert a.rates_errors() == int(bad.sum()) * (T // 2)
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
def test_argument_checks(golden_dir):
    import torch
    import lyra_amd
    B = 4
    ids, rates, bits = _ids(B, 8, 0), _rates(B), np.full(B, 64, np.int32)
    pcm = _pcm_rows(golden_dir, B, 2, rates, 0, 0, 0)
    a, u = _ctx(8), _ctx(8)
    try:
        d_pk = torch.zeros((B, 23), dtype=torch.uint8, device=_dev())
        d_pb = torch.zeros(B, dtype=torch.int32, device=_dev())
        L, h = a.L, a.h
        p = lambda x: x.data_ptr()   # noqa: E731
        d_ids, d_pcm, d_r, d_b = _t(ids), _t(pcm[0]), _t(rates), _t(bits)
        d16 = torch.zeros((B, 320), dtype=torch.int16, device=_dev())
        dx = torch.zeros((B, ROW), dtype=torch.int16, device=_dev())
        good_e = [p(d_ids), B, p(d_pcm), p(d_r), p(d_b), 0, p(d_pk), p(d_pb)]
        for i in (0, 2, 3, 4, 6, 7):
            args = list(good_e)
            args[i] = None
            assert L.lyra_hip_encode_rates_dev(h, *args) == -1, i
        for bad_b in (0, 9):
            args = list(good_e)
            args[1] = bad_b
            assert L.lyra_hip_encode_rates_dev(h, *args) == -1, bad_b
        good_d = [p(d_ids), B, p(d_pk), p(d_pb), p(d_r), p(d16), p(dx), None, None]
        for i in (0, 2, 3, 4, 5, 6):
            args = list(good_d)
            args[i] = None
            assert L.lyra_hip_decode_lossy_rates_dev(h, *args) == -1, i
        for bad_b in (0, 9):
            args = list(good_d)
            args[1] = bad_b
            assert L.lyra_hip_decode_lossy_rates_dev(h, *args) == -1, bad_b
        for t in range(2):
            got = _encode_rates(a, ids, pcm[t], rates, bits, False)
            want = _encode_uniform(u, ids, pcm[t], rates, bits, False)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0][:, :8], want[0][:, :8])
        assert isinstance(lyra_amd.MAX_EXT_HOP, int)
    finally:
        a.close()
        u.close()


class _Steps:
    """Buffers of a run_steps session with MIXED_RATE and the call itself."""

    def __init__(self, B, ids, rates, pcm, rx, sched, mixed_bits, dtx):
        import torch
        z = lambda shape, dt, fill=0: torch.full(shape, fill, dtype=dt, device=_dev())   # noqa: E731
        self.pk = [z((B, 23), torch.uint8) for _ in range(2)]
        self.pb = [z((B,), torch.int32) for _ in range(2)]
        self.out = [z((B, 320), torch.int16) for _ in range(2)]
        self.ext = [z((B, ROW), torch.int16, 0x3333) for _ in range(2)]
        self.cn, self.isn = z((B,), torch.int32), z((B,), torch.int32)
        self.d_ids, self.bits = _t(ids), 0 if mixed_bits else int(sched[0, 0])
        self.kw = dict(d_pcm_ring=_t(pcm), d_packets=self.pk, d_pcm_out=self.out, d_packet_bytes=self.pb, d_ext_out=self.ext,
                       dtx=dtx, packet_loss=True, d_received_ring=_t(rx), d_is_comfort_noise=self.cn, d_is_noise=self.isn,
                       d_rates=_t(rates), d_bits_ring=_t(sched) if mixed_bits else None)

    def run(self, ctx, first, n, **over):
        ctx.run_steps_dev(self.d_ids, self.bits, n, first_step=first, **dict(self.kw, **over))

    def check_hop(self, t, want_pk, want_pb, want, rates, last):
        s = t & 1
        assert np.array_equal(self.pb[s].cpu().numpy(), want_pb), t
        pk = self.pk[s].cpu().numpy()
        for b in range(want_pb.size):
            assert np.array_equal(pk[b, :want_pb[b]], want_pk[b, :want_pb[b]]), (t, b)
        assert np.array_equal(self.out[s].cpu().numpy(), want[0]), t
        gx = self.ext[s].cpu().numpy()
        for b, r in enumerate(rates):
            assert np.array_equal(gx[b, :r // 50], want[1][b, :r // 50]), (t, b)
            assert (gx[b, r // 50:] == 0x3333).all(), (t, b, "samples past rate / 50 were written")
        if last:   # (one buffer for every step)
            assert np.array_equal(self.isn.cpu().numpy(), want[2]) and np.array_equal(self.cn.cpu().numpy(), want[3]), t


@pytest.mark.gpu
@pytest.mark.parametrize("mixed_bits,dtx", [(False, False), (True, True), (False, True), (True, False)])
def test_run_steps_mixed_rate_equals_single_calls(golden_dir, mixed_bits, dtx):
    """MIXED_RATE over checkpoints [3, 4, 12, 14] (first_step != 0 from the second call on) against the two single calls
    per hop on a second context: the last two hops of every segment (both buffer sets), every output."""
    import torch
    B, T, ms = 37, 14, 64
    ids, rates = _ids(B, ms, 21), _rates(B)
    pcm = _pcm_rows(golden_dir, B, T, rates, 3 if dtx else 0, 4, 0)
    rng = np.random.default_rng(6)
    sched = np.stack([_draw_bits(rng, B) for _ in range(T)]) if mixed_bits else np.full((T, B), 120, np.int32)
    rx = _gilbert(np.random.default_rng(2), T, B)
    a, u = _ctx(ms), _ctx(ms)
    try:
        S = _Steps(B, ids, rates, pcm, rx, sched, mixed_bits, dtx)
        dn = torch.zeros(B, dtype=torch.int32, device=_dev())
        wants, done = {}, 0
        for upto in (3, 4, 12, 14):
            S.run(a, done, upto - done)
            a.synchronize()
            for t in range(done, upto):
                w_pk, w_pb = _encode_rates(u, ids, pcm[t], rates, sched[t], dtx)
                wants[t] = (w_pk, w_pb, _decode_rates(u, ids, w_pk, w_pb * rx[t], rates, dn=dn))
            for t in (upto - 2, upto - 1):
                S.check_hop(t, *wants[t], rates, last=t == upto - 1)
            done = upto
        assert a.rates_errors() == 0
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
def test_run_steps_mixed_rate_rejections(golden_dir):
    """external_rate != 0, d_rates == NULL and d_features through a raw lyra_hip_steps_rates; DECODE without PACKET_LOSS and
    missing d_packet_bytes through the wrapper, which refuses an explicit external_rate itself.  A valid call follows."""
    import torch
    from lyra_amd import LyraHipError, codec
    B, T = 8, 3
    ids, rates = _ids(B, 16, 1), _rates(B)
    pcm = _pcm_rows(golden_dir, B, T, rates, 0, 4, 0)
    sched, rx = np.full((T, B), 64, np.int32), np.ones((T, B), np.uint8)
    a, u = _ctx(16), _ctx(16)
    try:
        S = _Steps(B, ids, rates, pcm, rx, sched, False, False)
        with pytest.raises(LyraHipError):
            S.run(a, 0, 1, packet_loss=False, d_received_ring=None)
        with pytest.raises(LyraHipError):
            S.run(a, 0, 1, d_packet_bytes=None)
        with pytest.raises(ValueError):
            S.run(a, 0, 1, external_rate=48000)

        def raw(**over):
            R = codec.StepsDescRates()
            st = R.steps
            st.d_stream_ids, st.B, st.num_bits, st.n_steps, st.ring = S.d_ids.data_ptr(), B, 64, 1, T
            st.flags = codec.STEP_ENCODE | codec.STEP_DECODE | codec.STEP_PACKET_LOSS | codec.STEP_MIXED_RATE
            st.d_pcm_ring = S.kw["d_pcm_ring"].data_ptr()
            for i in range(2):
                st.d_packets[i], st.d_packet_bytes[i] = S.pk[i].data_ptr(), S.pb[i].data_ptr()
                st.d_pcm_out[i], st.d_ext_out[i] = S.out[i].data_ptr(), S.ext[i].data_ptr()
            R.d_rates = S.kw["d_rates"].data_ptr()
            for k, v in over.items():
                setattr(R if k == "d_rates" else st, k, v)
            return a.L.lyra_hip_run_steps_dev(a.h, ctypes.byref(R.steps))

        feats = torch.zeros((B, 64), dtype=torch.float32, device=_dev())
        assert raw(external_rate=48000) == -1
        assert raw(external_rate=16000) == -1
        assert raw(d_rates=None) == -1
        assert raw(d_features=feats.data_ptr(), n_features=1) == -1
        a.synchronize()
        assert S.pb[0].sum().item() == 0   # nothing was enqueued
        assert raw() == 0
        a.synchronize()
        w_pk, w_pb = _encode_rates(u, ids, pcm[0], rates, sched[0], False)
        S.check_hop(0, w_pk, w_pb, _decode_rates(u, ids, w_pk, w_pb, rates), rates, last=False)
    finally:
        a.close()
        u.close()


def _random_sequence(golden_dir, seed):
    """A seeded random sequence over 36 hops on context A -- per hop the per-row calls, or the uniform calls per rate group,
    or a run_steps segment with MIXED_RATE; synchronize and set_serial at random -- against a strictly serial replay with
    the per-row calls on context B: every hop's packets and decoder outputs."""
    import torch
    B, T, ms = 29, 36, 64
    rng = np.random.default_rng(seed)
    ids, rates = _ids(B, ms, 40 + seed), _rates(B)
    pcm = _pcm_rows(golden_dir, B, T, rates, 3, seed, 0)
    sched = np.stack([_draw_bits(rng, B) for _ in range(T)])
    rx = _gilbert(np.random.default_rng(seed + 1), T, B)
    a, u = _ctx(ms), _ctx(ms)
    try:
        u.set_serial(True)
        S = _Steps(B, ids, rates, pcm, rx, sched, True, True)
        dn = torch.zeros(B, dtype=torch.int32, device=_dev())
        wants = []
        for t in range(T):
            w_pk, w_pb = _encode_rates(u, ids, pcm[t], rates, sched[t], True)
            wants.append((w_pk, w_pb, _decode_rates(u, ids, w_pk, w_pb * rx[t], rates, dn=dn)))
        t, serial, log = 0, False, []
        while t < T:
            if rng.random() < 0.2:
                serial = not serial
                a.set_serial(serial)
                log.append(f"serial={serial}")
            op = rng.choice(["rates", "uniform", "steps"])
            log.append(f"{t}:{op}")
            if op == "steps":
                n = int(min(T - t, rng.integers(1, 5)))
                S.run(a, t, n)
                a.synchronize()
                for k in range(max(t, t + n - 2), t + n):
                    S.check_hop(k, *wants[k], rates, last=False)
                assert np.array_equal(S.cn.cpu().numpy(), wants[t + n - 1][2][3]), (log, "is_comfort_noise")
                t += n
                continue
            enc = _encode_rates if op == "rates" else _encode_uniform
            if rng.random() < 0.5:
                a.synchronize()
            g_pk, g_pb = enc(a, ids, pcm[t], rates, sched[t], True)
            w_pk, w_pb, want = wants[t]
            assert np.array_equal(g_pb, w_pb), log
            for b in range(B):
                assert np.array_equal(g_pk[b, :w_pb[b]], w_pk[b, :w_pb[b]]), (log, b)
            if op == "rates":
                got = _decode_rates(a, ids, w_pk, w_pb * rx[t], rates)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3]), log
                for b, r in enumerate(rates):
                    assert np.array_equal(got[1][b, :r // 50], want[1][b, :r // 50]), (log, b)
            else:
                got = _decode_uniform(a, ids, w_pk, w_pb * rx[t], rates)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[3]), log
                for b, r in enumerate(rates):
                    assert np.array_equal(got[1][b, :r // 50], want[1][b, :r // 50]), (log, b)
            t += 1
        assert a.rates_errors() == 0
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_call_sequences(golden_dir, seed):
    _random_sequence(golden_dir, seed)
