"""Per-stream bitrates on the device path: lyra_hip_encode_mixed_dev, lyra_hip_decode_lossy_mixed_dev and
LYRA_HIP_STEP_MIXED_BITRATE.  Expectations: the existing one-bitrate calls on the same streams, split by bit count over
disjoint id lists on a second context (bit for bit, packets and every decoder output); the reference models
(oracle/lyra_codec_model.py: RefLyraEncoder with its bitrate changed between hops as set_bitrate does, RefLyraDecoder fed
packets of changing sizes, held to the criteria of test_gpu_lossy_decode.py); run_steps against the single calls."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_plumbing import _dev, _ids, _same, _t, make_ctx as _ctx
from receiver_models import LossyModel
from row_cases import SENTINEL, _check_sentinel_rows as _check_rows, _draw_bits
from signals import _gilbert, _patterns, _speech

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))

SIZES = (8, 15, 23)                       # the codec's packet sizes: 64 / 120 / 184 bits


def _pcm(golden_dir, B, T, rate, silent_every=0, seed=0):
    """[T][B][rate / 50] int16: speech (signals._speech), every silent_every-th stream silent from hop 5 on
    (DTX), at other rates each sample repeated (any int16 input is a valid hop for the encoder's resampler)."""
    pcm = _speech(golden_dir, B, T, offset=seed)
    if silent_every:
        pcm[5:, ::silent_every] = 0
    return np.repeat(pcm, rate // 16000, axis=2) if rate > 16000 else pcm


def _encode_uniform(ctx, d_ids, d_pcm, rate, bits, dtx):
    """encode_ext_dev once per bit count on that count's id subset -> (packets [B][23] zero-padded, packet_bytes [B])."""
    import torch
    import lyra_amd
    B = bits.size
    pk = np.zeros((B, 23), np.uint8)
    pb = np.zeros(B, np.int32)
    outs = []
    for v in np.unique(bits):
        sel = np.flatnonzero(bits == v)
        s = torch.from_numpy(sel).to(_dev())
        n = lyra_amd.packet_size(int(v))
        d_pk = torch.zeros((sel.size, n), dtype=torch.uint8, device=_dev())
        d_pb = torch.full((sel.size,), -7, dtype=torch.int32, device=_dev())
        ctx.encode_ext_dev(d_ids[s].contiguous(), d_pcm[s].contiguous(), rate, int(v), d_pk, d_pb if dtx else None, dtx=dtx)
        outs.append((sel, n, d_pk, d_pb))
    ctx.synchronize()
    for sel, n, d_pk, d_pb in outs:
        pk[sel, :n] = d_pk.cpu().numpy()
        pb[sel] = d_pb.cpu().numpy() if dtx else n
    return pk, pb


# ---- encoder -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("B,rate,dtx", [(4096, 16000, False), (4096, 48000, True), (17, 16000, True), (17, 48000, False),
                                        (1, 48000, True), (1, 16000, False)])
def test_encode_mixed_equals_uniform_calls(golden_dir, B, rate, dtx):
    """Every row's packet and packet_bytes equal encode_ext_dev's at that row's bit count (one call per bit count on a
    second context fed the same audio); bytes past each row's size keep the sentinel.  Bits change every hop."""
    import torch
    T = 8 if B > 64 else 40
    ms = 4096 if B > 64 else 64
    ids = _ids(B, ms, B + rate)
    pcm = _pcm(golden_dir, B, T, rate, silent_every=3 if dtx else 0, seed=B)
    rng = np.random.default_rng(rate + B + dtx)
    a, u = _ctx(ms), _ctx(ms)
    try:
        if dtx:
            a.set_encoder_sample_rate(rate)
            u.set_encoder_sample_rate(rate)
        d_ids = _t(ids)
        saw_noise = 0
        for t in range(T):
            bits = _draw_bits(rng, B)
            d_pcm = _t(pcm[t])
            d_pk = torch.full((B, 23), SENTINEL, dtype=torch.uint8, device=_dev())
            d_pb = torch.full((B,), -7, dtype=torch.int32, device=_dev())
            a.encode_mixed_dev(d_ids, d_pcm, rate, _t(bits), d_pk, d_pb, dtx=dtx)
            want_pk, want_pb = _encode_uniform(u, d_ids, d_pcm, rate, bits, dtx)
            a.synchronize()
            _check_rows(d_pk.cpu().numpy(), d_pb.cpu().numpy(), want_pk, want_pb, f"hop {t}")
            saw_noise += int((want_pb == 0).sum())
        assert a.encode_mixed_errors() == 0
        if dtx and T >= 40:
            assert saw_noise > 0
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
def test_encode_mixed_vs_reference_model(golden_dir, oracle_default):
    """16 streams over 40 hops whose bitrates change mid-session (RefLyraEncoder.bits assigned before each hop, as
    LyraEncoder::set_bitrate does): packets equal, byte for byte."""
    import torch
    from oracle import lyra_codec_model as M
    B, T = 16, 40
    ids = _ids(B, 64, 11)
    pcm = _pcm(golden_dir, B, T, 16000, seed=7)
    rng = np.random.default_rng(3)
    sched = np.empty((T, B), np.int32)
    sched[:] = rng.choice((64, 120, 184), size=B)
    sched[20:] = rng.choice((64, 120, 184), size=B)          # every stream may switch at hop 20 ...
    sched[25:, ::4] = 64                                      # ... some again at 25 and 33
    sched[33:, 1::4] = 184
    encs = [M.RefLyraEncoder(oracle_default, 16000, int(sched[0, s]), False) for s in range(B)]
    a = _ctx(64)
    try:
        d_ids = _t(ids)
        for t in range(T):
            d_pk = torch.full((B, 23), SENTINEL, dtype=torch.uint8, device=_dev())
            d_pb = torch.zeros(B, dtype=torch.int32, device=_dev())
            a.encode_mixed_dev(d_ids, _t(pcm[t]), 16000, _t(sched[t]), d_pk, d_pb)
            a.synchronize()
            pk, pb = d_pk.cpu().numpy(), d_pb.cpu().numpy()
            for s, enc in enumerate(encs):
                enc.bits = int(sched[t, s])
                want = enc.Encode(pcm[t, s])
                assert pb[s] == want.size and np.array_equal(pk[s, :want.size], want), (t, s)
    finally:
        a.close()


# ---- decoder -------------------------------------------------------------------------------------------------------------

def _mixed_run(ctx, ids, packets, sizes, rate, fill):
    """decode_lossy_mixed_dev per tick: packets [T][B][23] (bytes past sizes[t][b] set to `fill`) -> outputs per tick."""
    import torch
    T, B = sizes.shape
    n_ext = rate // 50
    d_ids = _t(np.asarray(ids, np.int32))
    out = []
    for t in range(T):
        pk = packets[t].copy()
        for s in SIZES + (0,):
            pk[sizes[t] == s, s:] = fill
        o16 = torch.empty((B, 320), dtype=torch.int16, device=_dev())
        oext = torch.empty((B, n_ext), dtype=torch.int16, device=_dev())
        isn = torch.empty(B, dtype=torch.int32, device=_dev())
        icn = torch.empty(B, dtype=torch.int32, device=_dev())
        ctx.decode_lossy_mixed_dev(d_ids, _t(pk), _t(sizes[t]), rate, o16, oext if rate != 16000 else None, isn, icn)
        ctx.synchronize()
        out.append((o16.cpu().numpy(), (oext if rate != 16000 else o16).cpu().numpy(), isn.cpu().numpy(), icn.cpu().numpy()))
    return out


def _uniform_run(ctx, ids, packets, sizes, group, rate):
    """decode_lossy_dev once per packet size on disjoint id lists; a row without a packet goes with group[t][b]."""
    import torch
    T, B = sizes.shape
    n_ext = rate // 50
    d_ids = _t(np.asarray(ids, np.int32))
    out = []
    for t in range(T):
        o16, oext = np.zeros((B, 320), np.int16), np.zeros((B, n_ext), np.int16)
        isn, icn = np.zeros(B, np.int32), np.zeros(B, np.int32)
        calls = []
        for g, s in enumerate(SIZES):
            sel = np.flatnonzero((sizes[t] == s) | ((sizes[t] == 0) & (group[t] == g)))
            if sel.size == 0:
                continue
            n = sel.size
            d = [torch.empty((n, 320), dtype=torch.int16, device=_dev()), torch.empty((n, n_ext), dtype=torch.int16, device=_dev()),
                 torch.empty(n, dtype=torch.int32, device=_dev()), torch.empty(n, dtype=torch.int32, device=_dev())]
            ctx.decode_lossy_dev(d_ids[torch.from_numpy(sel).to(_dev())].contiguous(), _t(packets[t][sel, :s]), _t(sizes[t][sel]),
                                 s * 8 if s != 23 else 184, rate, d[0], d[1] if rate != 16000 else None, d[2], d[3])
            calls.append((sel, d))
        ctx.synchronize()
        for sel, d in calls:
            o16[sel] = d[0].cpu().numpy()
            oext[sel] = (d[1] if rate != 16000 else d[0]).cpu().numpy()
            isn[sel] = d[2].cpu().numpy()
            icn[sel] = d[3].cpu().numpy()
        out.append((o16, oext, isn, icn))
    return out


@pytest.mark.gpu
def test_decode_mixed_equals_uniform_calls():
    """4096 streams, 40 ticks at 48 kHz: per-row sizes from {0, 8, 15, 23} changing every tick, Gilbert loss bursts into
    comfort noise and back.  decode_lossy_mixed_dev (bytes past each size zero, and again 0xFF) equals decode_lossy_dev called
    per bitrate on disjoint id lists, every output, bit for bit."""
    B, T, rate = 4096, 40, 48000
    rng = np.random.default_rng(17)
    ids = _ids(B, 4096, 5)
    packets = rng.integers(0, 256, size=(T, B, 23), dtype=np.uint8)
    rx = _gilbert(rng, T, B)
    sizes = (rng.choice(SIZES, size=(T, B)) * rx).astype(np.int32)
    group = rng.integers(0, 3, size=(T, B))
    m, f, u = _ctx(4096), _ctx(4096), _ctx(4096)
    try:
        want = _uniform_run(u, ids, packets, sizes, group, rate)
        got = _mixed_run(m, ids, packets, sizes, rate, 0)
        got_ff = _mixed_run(f, ids, packets, sizes, rate, 0xFF)
        for t in range(T):
            _same(got[t], want[t], f"tick {t}")
            _same(got_ff[t], want[t], f"tick {t}, 0xFF fill")
        assert want[12][3][:16].all() and (want[20][3][:16] == 0).sum() >= 8   # rows 0..15: comfort noise, and back
        assert m.decode_lossy_errors() == 0 and f.decode_lossy_errors() == 0
    finally:
        for c in (m, f, u):
            c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [64, 120, 184])
def test_decode_mixed_uniform_rows_equal_existing_call(bits):
    """Every row at one bitrate: decode_lossy_mixed_dev on rows restrided to 23 bytes == decode_lossy_dev."""
    B, T, rate = 263, 20, 16000
    s = (bits + 7) // 8
    rng = np.random.default_rng(bits)
    ids = _ids(B, 512, bits)
    packets = rng.integers(0, 256, size=(T, B, 23), dtype=np.uint8)
    sizes = (_gilbert(rng, T, B, p_loss=0.2) * s).astype(np.int32)
    m, u = _ctx(512), _ctx(512)
    try:
        want = _uniform_run(u, ids, packets, sizes, np.full((T, B), SIZES.index(s)), rate)
        got = _mixed_run(m, ids, packets, sizes, rate, 0x5A)
        for t in range(T):
            _same(got[t], want[t], f"tick {t}")
    finally:
        m.close()
        u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [16000, 32000])
def test_decode_mixed_vs_reference_model(golden_dir, oracle_default, rate):
    """Six streams whose packets change size every few ticks, through the loss patterns of test_gpu_lossy_decode.py, against
    RefLyraDecoder with SetEncodedPacket(packet[:size]) on received ticks: generative samples exact, comfort-noise samples
    within 1 LSB, flags exact (LossyModel)."""
    from oracle import lyra_codec_model as M
    B, T = 6, 36
    ids = [21, 4, 9, 50, 0, 33]
    pcm = _pcm(golden_dir, B, T, 16000, seed=rate)
    mask = np.concatenate([_patterns(T), _patterns(T)[:, 2:4]], axis=1)
    sched = np.array([[(64, 120, 184)[(t // (3 + s) + s) % 3] for s in range(B)] for t in range(T)], np.int32)
    encs = [M.RefLyraEncoder(oracle_default, 16000, int(sched[0, s]), False) for s in range(B)]
    pk_list = []
    for t in range(T):
        row = []
        for s, enc in enumerate(encs):
            enc.bits = int(sched[t, s])
            row.append(enc.Encode(pcm[t, s]))
        pk_list.append(row)
    packets = np.zeros((T, B, 23), np.uint8)
    sizes = np.zeros((T, B), np.int32)
    for t in range(T):
        for s in range(B):
            packets[t, s, :pk_list[t][s].size] = pk_list[t][s]
            sizes[t, s] = pk_list[t][s].size if mask[t, s] else 0
    model = LossyModel(oracle_default, rate, ids)
    ctx = _ctx(64)
    try:
        for t in range(T):
            got = _mixed_run(ctx, ids, packets[t:t + 1], sizes[t:t + 1], rate, 0xEE)[0]
            model.tick(t, pk_list[t], mask[t], got)
        model.check_estimates(ctx, "end")
    finally:
        ctx.close()
    model.tally.report(f"mixed-bitrate lossy sessions {rate} Hz")
    assert model.saw_cn and model.saw_mix and model.saw_back


# ---- invalid values and arguments ----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_invalid_values_are_counted_once_and_change_nothing_else(golden_dir):
    """Encoder bits 0, 63, 188, -4 and decoder sizes 5, 24, -1: each counted exactly once; those rows get packet_bytes 0 /
    are treated as lost, every other row is what the uniform calls give, and the encoder state of an invalid row advances
    (its next hop, valid again, equals the uniform path that encoded it)."""
    import torch
    B, rate = 64, 16000
    ids = _ids(B, 64, 1)
    pcm = _pcm(golden_dir, B, 3, rate, seed=5)
    bad = {3: 0, 10: 63, 41: 188, 63: -4}
    a, u = _ctx(64), _ctx(64)
    try:
        d_ids = _t(ids)
        for t in range(3):
            bits = np.full(B, 120, np.int32)
            bits[::2] = 64
            ubits = bits.copy()
            if t == 1:
                for r, v in bad.items():
                    bits[r] = v
            d_pk = torch.full((B, 23), SENTINEL, dtype=torch.uint8, device=_dev())
            d_pb = torch.full((B,), -7, dtype=torch.int32, device=_dev())
            a.encode_mixed_dev(d_ids, _t(pcm[t]), rate, _t(bits), d_pk, d_pb)
            want_pk, want_pb = _encode_uniform(u, d_ids, _t(pcm[t]), rate, ubits, False)
            a.synchronize()
            if t == 1:
                for r in bad:
                    want_pb[r] = 0
            _check_rows(d_pk.cpu().numpy(), d_pb.cpu().numpy(), want_pk, want_pb, f"hop {t}")
        assert a.encode_mixed_errors(clear=True) == len(bad)
        assert a.encode_mixed_errors() == 0
        # decoder: invalid sizes are lost rows, counted once each
        rng = np.random.default_rng(2)
        packets = rng.integers(0, 256, size=(4, B, 23), dtype=np.uint8)
        sizes = rng.choice(SIZES, size=(4, B)).astype(np.int32)
        sizes[2:, 7] = 0
        ref_sizes = sizes.copy()
        for r, v in {5: 5, 20: 24, 30: -1}.items():
            sizes[1, r] = v
            ref_sizes[1, r] = 0
        a.reset()
        a.decode_lossy_errors(clear=True)
        got = _mixed_run(a, ids, packets, sizes, rate, 0)
        b = _ctx(64)
        try:
            want = _mixed_run(b, ids, packets, ref_sizes, rate, 0)
        finally:
            b.close()
        for t in range(4):
            _same(got[t], want[t], f"tick {t}")
        assert a.decode_lossy_errors() == 3
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
def test_host_side_argument_checks():
    import ctypes
    import torch
    import lyra_amd
    from lyra_amd import codec
    B = 32
    a = _ctx(64)
    try:
        L, h = a.L, a.h
        d_ids = torch.arange(B, dtype=torch.int32, device=_dev())
        pcm = torch.zeros((B, 320), dtype=torch.int16, device=_dev())
        bits = torch.full((B,), 64, dtype=torch.int32, device=_dev())
        pk = torch.zeros((B, 23), dtype=torch.uint8, device=_dev())
        pb = torch.zeros(B, dtype=torch.int32, device=_dev())
        o = torch.zeros((B, 320), dtype=torch.int16, device=_dev())
        P = lambda t: t.data_ptr()
        enc = L.lyra_hip_encode_mixed_dev
        assert enc(h, P(d_ids), 0, P(pcm), 16000, P(bits), 0, P(pk), P(pb)) == -1
        assert enc(h, P(d_ids), 65, P(pcm), 16000, P(bits), 0, P(pk), P(pb)) == -1
        assert enc(h, P(d_ids), B, P(pcm), 44100, P(bits), 0, P(pk), P(pb)) == -1
        assert enc(h, P(d_ids), B, P(pcm), 16000, None, 0, P(pk), P(pb)) == -1
        assert enc(h, P(d_ids), B, P(pcm), 16000, P(bits), 0, P(pk), None) == -1
        assert enc(h, P(d_ids), B, P(pcm), 16000, P(bits), 0, None, P(pb)) == -1
        assert enc(h, None, B, P(pcm), 16000, P(bits), 0, P(pk), P(pb)) == -1
        assert enc(h, P(d_ids), B, P(pcm), 48000, P(bits), 1, P(pk), P(pb)) == -1   # DTX estimator set up for 16 kHz
        dec = L.lyra_hip_decode_lossy_mixed_dev
        assert dec(h, P(d_ids), 0, P(pk), P(pb), 16000, P(o), None, None, None) == -1
        assert dec(h, P(d_ids), B, P(pk), P(pb), 22050, P(o), None, None, None) == -1
        assert dec(h, P(d_ids), B, P(pk), None, 16000, P(o), None, None, None) == -1
        assert dec(h, P(d_ids), B, None, P(pb), 16000, P(o), None, None, None) == -1
        assert dec(h, P(d_ids), B, P(pk), P(pb), 48000, P(o), None, None, None) == -1   # no external-rate output
        assert dec(h, P(d_ids), B, P(pk), P(pb), 16000, None, None, None, None) == -1
        ring = torch.full((2, B), 64, dtype=torch.int32, device=_dev())
        ring_pcm = torch.zeros((2, B, 320), dtype=torch.int16, device=_dev())
        two = lambda: [torch.zeros((B, 23), dtype=torch.uint8, device=_dev()) for _ in range(2)]
        pbs = [torch.zeros(B, dtype=torch.int32, device=_dev()) for _ in range(2)]
        outs = [torch.zeros((B, 320), dtype=torch.int16, device=_dev()) for _ in range(2)]
        with pytest.raises(lyra_amd.LyraHipError):   # num_bits != 0
            a.run_steps_dev(d_ids, 64, 1, d_pcm_ring=ring_pcm, d_packets=two(), d_packet_bytes=pbs, d_pcm_out=outs,
                            packet_loss=True, d_bits_ring=ring)
        with pytest.raises(lyra_amd.LyraHipError):   # DECODE without PACKET_LOSS
            a.run_steps_dev(d_ids, 0, 1, d_pcm_ring=ring_pcm, d_packets=two(), d_packet_bytes=pbs, d_pcm_out=outs,
                            d_bits_ring=ring)
        with pytest.raises(lyra_amd.LyraHipError):   # ENCODE without packet_bytes
            a.run_steps_dev(d_ids, 0, 1, d_pcm_ring=ring_pcm, d_packets=two(), d_pcm_out=outs, decode=False, d_bits_ring=ring)
        torch.cuda.synchronize()
        S = codec.StepsDesc()                        # the flag without a ring
        S.d_stream_ids, S.B, S.num_bits, S.n_steps, S.flags = P(d_ids), B, 0, 1, codec.STEP_MIXED_BITRATE | codec.STEP_ENCODE
        S.ring, S.d_pcm_ring = 2, P(ring_pcm)
        for i in range(2):
            S.d_packets[i], S.d_packet_bytes[i] = P(pk), P(pbs[i])
        assert L.lyra_hip_run_steps_dev(h, ctypes.byref(S)) == -1
        S.d_bits_ring, S.n_bits_ring = P(ring), 0
        assert L.lyra_hip_run_steps_dev(h, ctypes.byref(S)) == -1
        S.n_bits_ring = 2
        assert L.lyra_hip_run_steps_dev(h, ctypes.byref(S)) == 0
        a.synchronize()
        assert (pbs[0].cpu().numpy() == 8).all()
    finally:
        a.close()


# ---- run_steps -----------------------------------------------------------------------------------------------------------

def steps_vs_single(golden_dir, rate, dtx, decode_only, serial=False, max_streams=256):
    """run_steps with a bits ring that changes every step (two calls, the second continuing) against encode_mixed_dev +
    decode_lossy_mixed_dev hop by hop on a second context; decode-only reads a packet ring with sizes from the bits ring.
    Returns the number of comfort-noise flags seen."""
    import torch
    import lyra_amd
    B, T = 200, 14
    n_ext = rate // 50
    rng = np.random.default_rng(rate + dtx + 2 * decode_only)
    ids = _ids(B, max_streams, rate)
    choice = (64, 120, 184) if decode_only else (64, 120, 184, 100)   # (decode-only: 100 bits -> 13 bytes, an invalid size)
    bits_ring = np.stack([rng.choice(choice, size=B) for _ in range(5)]).astype(np.int32)
    rx = _gilbert(rng, T, B, p_loss=0.15)
    pcm = _pcm(golden_dir, B, T, rate, silent_every=4 if dtx else 0, seed=3)
    pk_ring = rng.integers(0, 256, size=(3, B, 23), dtype=np.uint8)
    s, r = _ctx(max_streams), _ctx(max_streams)
    try:
        if serial:
            s.set_serial(True)
            r.set_serial(True)
        if dtx:
            s.set_encoder_sample_rate(rate)
            r.set_encoder_sample_rate(rate)
        d_ids = _t(ids)
        mk = lambda shape, dt: [torch.zeros(shape, dtype=dt, device=_dev()) for _ in range(2)]
        pk, pb, o16, oext = mk((B, 23), torch.uint8), mk(B, torch.int32), mk((B, 320), torch.int16), mk((B, n_ext), torch.int16)
        isn, icn = torch.zeros(B, dtype=torch.int32, device=_dev()), torch.zeros(B, dtype=torch.int32, device=_dev())
        d_bits, d_rx, d_pcm, d_pkr = _t(bits_ring), _t(rx), _t(pcm), _t(pk_ring)
        # single calls
        want = []
        for t in range(T):
            k = t & 1
            bits = bits_ring[t % 5]
            if decode_only:
                nb = np.array([lyra_amd.packet_size(int(v)) for v in bits], np.int32)
                pkt = d_pkr[t % 3]
            else:
                r.encode_mixed_dev(d_ids, d_pcm[t], rate, d_bits[t % 5], pk[k], pb[k], dtx=dtx)
                r.synchronize()
                nb = pb[k].cpu().numpy()
                pkt = pk[k]
            r.decode_lossy_mixed_dev(d_ids, pkt, _t(nb * rx[t]), rate, o16[k], oext[k] if rate != 16000 else None,
                                     isn, icn)
            r.synchronize()
            want.append((o16[k].cpu().numpy().copy(), oext[k].cpu().numpy().copy(), isn.cpu().numpy().copy(),
                         icn.cpu().numpy().copy(), None if decode_only else (pk[k].cpu().numpy().copy(), nb.copy())))
        # run_steps in two calls
        for a, b in ((0, 6), (6, T)):
            kw = dict(d_pcm_out=o16, d_received_ring=d_rx, d_is_noise=isn, d_is_comfort_noise=icn, external_rate=rate,
                      d_ext_out=oext if rate != 16000 else None, packet_loss=True, d_bits_ring=d_bits)
            if decode_only:
                s.run_steps_dev(d_ids, 0, b - a, first_step=a, d_packet_ring=d_pkr, encode=False, **kw)
            else:
                for i in range(2):
                    pk[i].fill_(SENTINEL)
                s.run_steps_dev(d_ids, 0, b - a, first_step=a, d_pcm_ring=d_pcm, d_packets=pk, d_packet_bytes=pb, dtx=dtx, **kw)
            s.synchronize()
            for t in (b - 2, b - 1):
                k = t & 1
                w = want[t]
                assert np.array_equal(o16[k].cpu().numpy(), w[0]), t
                if rate != 16000:
                    assert np.array_equal(oext[k].cpu().numpy(), w[1]), t
                if w[4] is not None:
                    got_pb = pb[k].cpu().numpy()
                    assert np.array_equal(got_pb, w[4][1]), t
                    got_pk = pk[k].cpu().numpy()
                    for row in range(B):
                        assert np.array_equal(got_pk[row, :got_pb[row]], w[4][0][row, :got_pb[row]]), (t, row)
            assert np.array_equal(isn.cpu().numpy(), want[b - 1][2]), b
            assert np.array_equal(icn.cpu().numpy(), want[b - 1][3]), b
        assert s.encode_mixed_errors() == 0 == r.encode_mixed_errors()
        # 100 bits make 13-byte packets, a size the decoder counts as invalid: run_steps counts every one (as it counts DTX
        # sizes with PACKET_LOSS), the single calls only those of received rows (the caller zeroed the others)
        bad = [w[4][1] == 13 for w in want] if not decode_only else [np.zeros(B, bool)] * T
        assert s.decode_lossy_errors() == sum(int(x.sum()) for x in bad) > 0 or decode_only
        assert r.decode_lossy_errors() == sum(int((x & (rx[t] != 0)).sum()) for t, x in enumerate(bad))
        return int(sum(w[3].sum() for w in want))
    finally:
        s.close()
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rate,dtx", [(16000, False), (16000, True), (32000, False), (32000, True)])
def test_run_steps_mixed_equals_single_calls(golden_dir, rate, dtx):
    assert steps_vs_single(golden_dir, rate, dtx, decode_only=False) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [16000, 48000])
def test_run_steps_mixed_decode_only(golden_dir, rate):
    assert steps_vs_single(golden_dir, rate, False, decode_only=True) > 0


@pytest.mark.gpu
def test_run_steps_mixed_serial(golden_dir):
    assert steps_vs_single(golden_dir, 16000, True, decode_only=False, serial=True) > 0


_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import test_gpu_mixed_bitrate as m
m.steps_vs_single(sys.argv[3], 16000, False, decode_only=False, max_streams=512)
m.steps_vs_single(sys.argv[3], 32000, True, decode_only=False, max_streams=512)
print("child ok")
'''


@pytest.mark.gpu
def test_run_steps_mixed_split_context(golden_dir):
    """LYRA_HIP_SUBBATCHES=2 (read at context creation, hence a child process): the mixed calls are not split and give the
    single calls' results."""
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, HERE, golden_dir], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, LYRA_HIP_SUBBATCHES="2"))
    assert r.returncode == 0 and "child ok" in r.stdout, r.stderr[-3000:]
