"""lyra_hip_decode_lossy_dev / LYRA_HIP_STEP_PACKET_LOSS: LyraDecoder's packet-loss concealment, comfort noise and
cross-fades (lyra_decoder.cc:172-373) on the device path, for hop-synchronous receivers.  Expectations: the per-stream
reference model oracle/lyra_codec_model.py (RefLyraDecoder, DecodeSamples(rate / 50) per tick, SetEncodedPacket only on
ticks with a packet), BatchLyraDecoder through lyra_amd/decoder_demo (bit for bit), the existing device path when every
packet arrives (bit for bit), and run_steps against the single calls (bit for bit)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BYTES = {64: 8, 120: 15, 184: 23}
SEED = 0x4C797261   # the context's default comfort-noise seed; stream `id` draws from SEED ^ id


def _speech(golden_dir, n, T, offset=0):
    sp = np.load(os.path.join(golden_dir, "sample_wavs.npz"))["sample1_16kHz"].astype(np.int16)
    out = np.empty((T, n, 320), np.int16)
    for s in range(n):
        start = (offset + 2357 * s) % (sp.size - T * 320)
        out[:, s] = sp[start:start + T * 320].reshape(T, 320)
    return out


def _patterns(T):
    """[T][4] 0/1: loss from the first hop then bursts; single losses; bursts of 3; a 12-hop run (pure comfort noise),
    then 5 lost (recovery in the middle of the fade to comfort noise), then 7 lost (recovery inside the fade back)."""
    m = np.ones((T, 4), np.uint8)
    m[:3, 0] = 0; m[9:11, 0] = 0; m[20:24, 0] = 0
    m[4::6, 1] = 0
    for a in (2, 11, 20, 29):
        m[a:a + 3, 2] = 0
    m[1:13, 3] = 0; m[15:20, 3] = 0; m[21:28, 3] = 0
    return m


def _ctx(max_streams=256):
    import lyra_amd
    return lyra_amd.LyraHip(device=0, max_streams=max_streams)


def _lossy_run(ctx, ids, packets, mask, bits, rate):
    """decode_lossy_dev tick by tick; packets [T][B][bytes] uint8, mask [T][B] -> (pcm16, ext, is_noise, is_cn) per tick."""
    import torch
    dev = torch.device("cuda", 0)
    T, B = mask.shape
    n_ext = rate // 50
    d_ids = torch.from_numpy(np.asarray(ids, np.int32)).to(dev)
    pk = [torch.empty((B, BYTES[bits]), dtype=torch.uint8, device=dev) for _ in range(2)]
    nb = [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2)]
    o16 = [torch.empty((B, 320), dtype=torch.int16, device=dev) for _ in range(2)]
    oext = [torch.empty((B, n_ext), dtype=torch.int16, device=dev) for _ in range(2)]
    isn = [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2)]
    icn = [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2)]
    res = []
    for t in range(T):
        k = t & 1
        pk[k].copy_(torch.from_numpy(np.ascontiguousarray(packets[t])))
        nb[k].copy_(torch.from_numpy((mask[t].astype(np.int32) * BYTES[bits])))
        ctx.decode_lossy_dev(d_ids, pk[k], nb[k], bits, rate, o16[k], oext[k] if rate != 16000 else None, isn[k], icn[k])
        ctx.synchronize()
        res.append((o16[k].cpu().numpy().copy(), (oext[k] if rate != 16000 else o16[k]).cpu().numpy().copy(),
                    isn[k].cpu().numpy().copy(), icn[k].cpu().numpy().copy()))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("rate,bits", [(8000, 184), (16000, 64), (32000, 120), (48000, 184)])
def test_lossy_sessions_vs_reference_model(golden_dir, oracle_default, rate, bits):
    from oracle import lyra_codec_model as M
    T, ids = 36, [5, 17, 2, 40]
    pcm = _speech(golden_dir, 4, T)
    mask = _patterns(T)
    encs = [M.RefLyraEncoder(oracle_default, 16000, bits, False) for _ in ids]
    packets = np.stack([np.stack([encs[s].Encode(pcm[t, s]) for s in range(4)]) for t in range(T)])
    ctx = _ctx()
    try:
        got = _lossy_run(ctx, ids, packets, mask, bits, rate)
    finally:
        ctx.close()
    decs = [M.RefLyraDecoder(oracle_default, rate, cng_seed=SEED ^ i) for i in ids]
    worst = n_exact = n_total = 0
    saw_cn = saw_mix = False
    for t in range(T):
        for s in range(4):
            if mask[t, s]:
                decs[s].SetEncodedPacket(packets[t, s])
            want = decs[s].DecodeSamples(rate // 50)
            d = np.abs(got[t][1][s].astype(int) - want.astype(int))
            worst = max(worst, int(d.max()))
            n_exact += int((d == 0).sum()); n_total += d.size
            assert got[t][3][s] == int(decs[s].is_comfort_noise()), (t, s)
            saw_cn = saw_cn or decs[s].is_comfort_noise()
            saw_mix = saw_mix or decs[s].fade == 320
    assert worst <= 2, worst
    assert n_exact / n_total > 0.97, n_exact / n_total
    assert saw_cn and saw_mix


@pytest.mark.gpu
def test_lossy_bit_identical_to_batch_decoder(tmp_path, golden_dir):
    """192 streams, bursty random loss, one hop-sized DecodeSamples per tick through BatchLyraDecoder (decoder_demo) --
    against decode_lossy_dev on the same packets in two calls per tick with scattered ids (B = 101 and 91)."""
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "decoder_demo")
    assert os.path.exists(demo), "lyra_amd/decoder_demo not built (__graft_entry__.build())"
    rate, bitrate, bits, n, T = 48000, 6000, 120, 192, 30
    hop = rate // 50
    rng = np.random.default_rng(11)
    sp = _speech(golden_dir, n, T)
    up = np.repeat(sp, 3, axis=2)   # any 48 kHz input will do: the packets come back from the demo
    mask = np.ones((T, n), np.uint8)
    state = np.zeros(n, bool)
    for t in range(T):            # two-state chain: ~20 % loss in bursts
        state = np.where(state, rng.random(n) < 0.6, rng.random(n) < 0.12)
        mask[t] = ~state
    mask[5:15, 7] = 0             # one stream all the way into comfort noise
    pin, sc = tmp_path / "in.s16", tmp_path / "script.txt"
    pk, ln, pout = tmp_path / "pk.bin", tmp_path / "len.i32", tmp_path / "out.s16"
    up.astype(np.int16).tofile(pin)
    sc.write_text("\n".join("".join(map(str, mask[t])) + f" {hop}" for t in range(T)) + "\n")
    r = subprocess.run([demo, lyra_amd.default_model_dir(), str(sc), str(pin), str(rate), str(bitrate), "0", str(n), str(pk),
                        str(ln), str(pout)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, LYRA_DEMO_PIPELINED="0"))
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    packets = np.fromfile(pk, np.uint8).reshape(T, n, BYTES[bits])
    want = np.fromfile(pout, np.int16).reshape(T, n, hop)
    perm = rng.permutation(n)
    groups = [np.sort(perm[:101])[::-1].copy(), perm[101:]]
    ctx = _ctx()
    try:
        import torch
        dev = torch.device("cuda", 0)
        d_ids = [torch.from_numpy(g.astype(np.int32)).to(dev) for g in groups]
        outs = [[torch.empty((len(g), hop), dtype=torch.int16, device=dev) for _ in range(2)] for g in groups]
        o16 = [[torch.empty((len(g), 320), dtype=torch.int16, device=dev) for _ in range(2)] for g in groups]
        for t in range(T):
            for gi, g in enumerate(groups):
                d_pk = torch.from_numpy(np.ascontiguousarray(packets[t][g])).to(dev)
                d_nb = torch.from_numpy(mask[t][g].astype(np.int32) * BYTES[bits]).to(dev)
                ctx.decode_lossy_dev(d_ids[gi], d_pk, d_nb, bits, rate, o16[gi][t & 1], outs[gi][t & 1])
                ctx.synchronize()
                got = outs[gi][t & 1].cpu().numpy()
                assert np.array_equal(got, want[t][g]), (t, gi, int(np.abs(got.astype(int) - want[t][g]).max()))
    finally:
        ctx.close()


def _steps_inputs(golden_dir, B, T, bits, seed):
    from oracle import lyra_codec_model as M, lyra_oracle
    o = lyra_oracle.Oracle(mode="xnnpack")
    pcm = _speech(golden_dir, B, T)
    rng = np.random.default_rng(seed)
    encs = [M.RefLyraEncoder(o, 16000, bits, False) for _ in range(B)]
    packets = np.stack([np.stack([encs[s].Encode(pcm[t, s]) for s in range(B)]) for t in range(T)])
    mask = (rng.random((T, B)) > 0.25).astype(np.uint8)
    mask[3:14, 1] = 0
    return packets, mask


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [16000, 32000])
def test_run_steps_packet_loss_equals_single_calls(golden_dir, rate):
    """Decode-only run_steps with PACKET_LOSS over 40 hops, as two calls (the second continuing at first_step 17) and as
    40 one-step calls, against 40 decode_lossy_dev calls: 16 kHz PCM, external-rate PCM, is_noise, is_comfort_noise."""
    import torch
    dev = torch.device("cuda", 0)
    B, T, bits = 6, 40, 120
    ids = np.array([9, 3, 30, 1, 22, 14], np.int32)
    packets, mask = _steps_inputs(golden_dir, B, T, bits, rate)
    ctx = _ctx()
    try:
        ref = _lossy_run(ctx, ids, packets, mask, bits, rate)
        n_ext = rate // 50
        d_ids = torch.from_numpy(ids).to(dev)
        d_ring = torch.from_numpy(np.ascontiguousarray(packets)).to(dev)
        d_rx = torch.from_numpy(np.ascontiguousarray(mask)).to(dev)
        o16 = [torch.empty((B, 320), dtype=torch.int16, device=dev) for _ in range(2)]
        oext = [torch.empty((B, n_ext), dtype=torch.int16, device=dev) for _ in range(2)]
        isn = torch.empty(B, dtype=torch.int32, device=dev)
        icn = torch.empty(B, dtype=torch.int32, device=dev)
        for cuts in ([0, 17, T], list(range(T + 1))):
            ctx.reset()
            for a, b in zip(cuts[:-1], cuts[1:]):
                ctx.run_steps_dev(d_ids, bits, b - a, first_step=a, d_pcm_out=o16,
                                  d_packet_ring=d_ring, d_received_ring=d_rx, d_is_noise=isn, d_is_comfort_noise=icn,
                                  external_rate=rate, d_ext_out=oext if rate != 16000 else None, encode=False,
                                  packet_loss=True, decoder_noise=True)
                ctx.synchronize()
                for t in (b - 2, b - 1):
                    if t < a:
                        continue
                    k = t & 1
                    assert np.array_equal(o16[k].cpu().numpy(), ref[t][0]), (cuts[:3], t)
                    if rate != 16000:
                        assert np.array_equal(oext[k].cpu().numpy(), ref[t][1]), (cuts[:3], t)
                assert np.array_equal(isn.cpu().numpy(), ref[b - 1][2]), (cuts[:3], b)
                assert np.array_equal(icn.cpu().numpy(), ref[b - 1][3]), (cuts[:3], b)
        assert any(r[3].any() for r in ref)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_run_steps_encode_dtx_packet_loss(golden_dir, oracle_default):
    """ENCODE | DTX | DECODE | PACKET_LOSS on partly silent input against encode_dtx_dev + decode_lossy_dev per hop (bit for
    bit) and the reference models (LyraEncoder with DTX; LyraDecoder seeing only non-empty, received packets); the receiver
    reaches comfort noise in the silences."""
    import torch
    from oracle import lyra_codec_model as M
    dev = torch.device("cuda", 0)
    B, T, bits = 4, 60, 64
    ids = np.array([2, 11, 6, 0], np.int32)
    pcm = _speech(golden_dir, B, T)
    pcm[12:44, 1] = 0
    pcm[20:50, 3] = 0
    rng = np.random.default_rng(5)
    rx = (rng.random((T, B)) > 0.1).astype(np.uint8)
    d_ids = torch.from_numpy(ids).to(dev)
    d_pcm = torch.from_numpy(pcm).to(dev)
    d_rx = torch.from_numpy(rx).to(dev)
    mk = lambda shape, dt: [torch.zeros(shape, dtype=dt, device=dev) for _ in range(2)]
    # single calls, hop by hop
    ctx = _ctx()
    try:
        pk, nb, o16, isn, icn = mk((B, 8), torch.uint8), mk(B, torch.int32), mk((B, 320), torch.int16), mk(B, torch.int32), mk(B, torch.int32)
        ref, lens = [], []
        for t in range(T):
            k = t & 1
            ctx.encode_dtx_dev(d_ids, d_pcm[t], bits, pk[k], nb[k])
            eff = nb[k] * d_rx[t].to(torch.int32)
            ctx.decode_lossy_dev(d_ids, pk[k], eff, bits, 16000, o16[k], None, isn[k], icn[k])
            ctx.synchronize()
            ref.append((o16[k].cpu().numpy().copy(), isn[k].cpu().numpy().copy(), icn[k].cpu().numpy().copy()))
            lens.append((nb[k].cpu().numpy().copy(), pk[k].cpu().numpy().copy()))
        ctx.reset()
        s16, snb, spk, sisn, sicn = mk((B, 320), torch.int16), mk(B, torch.int32), mk((B, 8), torch.uint8), mk(B, torch.int32), mk(B, torch.int32)
        for a, b in ((0, 23), (23, T)):
            ctx.run_steps_dev(d_ids, bits, b - a, first_step=a, d_pcm_ring=d_pcm, d_packets=spk, d_pcm_out=s16,
                              d_packet_bytes=snb, d_received_ring=d_rx, d_is_noise=sisn[0], d_is_comfort_noise=sicn[0],
                              dtx=True, packet_loss=True)
            ctx.synchronize()
            for t in (b - 2, b - 1):
                assert np.array_equal(s16[t & 1].cpu().numpy(), ref[t][0]), t
            assert np.array_equal(sisn[0].cpu().numpy(), ref[b - 1][1])
            assert np.array_equal(sicn[0].cpu().numpy(), ref[b - 1][2])
    finally:
        ctx.close()
    encs = [M.RefLyraEncoder(oracle_default, 16000, bits, True) for _ in ids]
    decs = [M.RefLyraDecoder(oracle_default, 16000, cng_seed=SEED ^ int(i)) for i in ids]
    worst = n_exact = n_total = 0
    saw_cn = False
    for t in range(T):
        for s in range(B):
            p = encs[s].Encode(pcm[t, s])
            assert lens[t][0][s] == p.size, (t, s)
            if p.size:
                assert np.array_equal(lens[t][1][s], p), (t, s)
                if rx[t, s]:
                    decs[s].SetEncodedPacket(p)
            want = decs[s].DecodeSamples(320)
            d = np.abs(ref[t][0][s].astype(int) - want.astype(int))
            worst = max(worst, int(d.max()))
            n_exact += int((d == 0).sum()); n_total += d.size
            assert ref[t][2][s] == int(decs[s].is_comfort_noise()), (t, s)
            saw_cn = saw_cn or (decs[s].is_comfort_noise() and s in (1, 3))
    assert worst <= 2 and n_exact / n_total > 0.97, (worst, n_exact / n_total)
    assert saw_cn


@pytest.mark.gpu
def test_all_received_equals_existing_path(golden_dir):
    """Every packet received: decode_lossy_dev == decode_dev + noise_receive_dev(DECODER) + resample_dev(DECODER), bit for
    bit, and is_comfort_noise stays 0."""
    import torch
    dev = torch.device("cuda", 0)
    B, T, bits, rate = 37, 12, 184, 48000
    ids = np.arange(3, 3 + 2 * B, 2).astype(np.int32)
    packets, _ = _steps_inputs(golden_dir, B, T, bits, 1)
    mask = np.ones((T, B), np.uint8)
    a, b = _ctx(), _ctx()
    try:
        got = _lossy_run(a, ids, packets, mask, bits, rate)
        d_ids = torch.from_numpy(ids).to(dev)
        o16 = torch.empty((B, 320), dtype=torch.int16, device=dev)
        oext = torch.empty((B, 960), dtype=torch.int16, device=dev)
        isn = torch.empty(B, dtype=torch.int32, device=dev)
        for t in range(T):
            b.decode_dev(d_ids, torch.from_numpy(np.ascontiguousarray(packets[t])).to(dev), bits, o16)
            b.noise_receive_dev(d_ids, o16, isn, side="decoder")
            b.resample_dev(d_ids, o16, 16000, rate, oext, side="decoder")
            b.synchronize()
            assert np.array_equal(o16.cpu().numpy(), got[t][0]), t
            assert np.array_equal(oext.cpu().numpy(), got[t][1]), t
            assert np.array_equal(isn.cpu().numpy(), got[t][2]), t
            assert not got[t][3].any()
    finally:
        a.close(); b.close()


_CHILD = r'''
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import torch, lyra_amd
packets = np.load(sys.argv[2]); mask = np.load(sys.argv[3])
T, B, nb = packets.shape
ctx = lyra_amd.LyraHip(device=0, max_streams=256)
dev = torch.device("cuda", 0)
d_ids = torch.arange(B, dtype=torch.int32, device=dev).flip(0).contiguous()
outs = []
for t in range(T):
    o = torch.empty((B, 320), dtype=torch.int16, device=dev)
    # a split decode_dev on other streams between the ticks: the lossy call is ordered against its chunks
    ctx.decode_lossy_dev(d_ids, torch.from_numpy(packets[t]).to(dev), torch.from_numpy(mask[t].astype(np.int32) * nb).to(dev),
                         nb * 8, 16000, o)
    ctx.decode_dev(d_ids + B, torch.from_numpy(packets[t]).to(dev), nb * 8, torch.empty((B, 320), dtype=torch.int16, device=dev))
    ctx.synchronize()
    outs.append(o.cpu().numpy())
np.save(sys.argv[4], np.stack(outs))
ctx.close()
'''


@pytest.mark.gpu
def test_lossy_reset_split_serial_and_errors(tmp_path, golden_dir):
    import torch
    import lyra_amd
    dev = torch.device("cuda", 0)
    B, T, bits = 128, 16, 64
    packets, mask = _steps_inputs(golden_dir, B, T, bits, 3)
    packets = packets[:, :, :8].copy()
    mask[2:12, :5] = 0
    ids = np.arange(B)[::-1].astype(np.int32)
    # reset_streams restores the initial control state: a context driven into comfort noise and reset == a fresh context
    a = _ctx()
    try:
        first = _lossy_run(a, ids, packets, mask, bits, 16000)
        assert first[11][3][:5].all()                        # rows 0..4 lost ticks 2..11: comfort noise
        a.reset(ids[:64].tolist())
        a.reset(ids[64:].tolist())
        again = _lossy_run(a, ids, packets, mask, bits, 16000)
        for t in range(T):
            assert np.array_equal(again[t][0], first[t][0]) and np.array_equal(again[t][3], first[t][3]), t
        # serial mode: the same results
        a.reset()
        a.set_serial(True)
        ser = _lossy_run(a, ids, packets, mask, bits, 16000)
        a.set_serial(False)
        for t in range(T):
            assert np.array_equal(ser[t][0], first[t][0]), t
        # invalid arguments
        d_ids = torch.from_numpy(ids).to(dev)
        d_pk = torch.from_numpy(packets[0]).to(dev)
        d_nb = torch.full((B,), 8, dtype=torch.int32, device=dev)
        o = torch.empty((B, 320), dtype=torch.int16, device=dev)
        L, h = a.L, a.h
        assert L.lyra_hip_decode_lossy_dev(h, d_ids.data_ptr(), B, d_pk.data_ptr(), d_nb.data_ptr(), 63, 16000, o.data_ptr(),
                                           None, None, None) == -1
        assert L.lyra_hip_decode_lossy_dev(h, d_ids.data_ptr(), B, d_pk.data_ptr(), d_nb.data_ptr(), 64, 44100, o.data_ptr(),
                                           None, None, None) == -1
        assert L.lyra_hip_decode_lossy_dev(h, d_ids.data_ptr(), B, d_pk.data_ptr(), None, 64, 16000, o.data_ptr(),
                                           None, None, None) == -1
        assert L.lyra_hip_decode_lossy_dev(h, d_ids.data_ptr(), B, d_pk.data_ptr(), d_nb.data_ptr(), 64, 48000, o.data_ptr(),
                                           None, None, None) == -1
        assert L.lyra_hip_decode_lossy_dev(h, d_ids.data_ptr(), 0, d_pk.data_ptr(), d_nb.data_ptr(), 64, 16000, o.data_ptr(),
                                           None, None, None) == -1
        with pytest.raises(lyra_amd.codec.LyraHipError):   # PACKET_LOSS needs packets, not features
            a.run_steps_dev(d_ids, bits, 1, d_pcm_out=[o, o], d_features=torch.zeros((B, 64), device=dev), encode=False,
                            packet_loss=True)
        # a packet_bytes value that is neither 0 nor the packet size: not received, counted, no fault
        a.decode_lossy_errors(clear=True)
        d_nb[3] = 5
        a.decode_lossy_dev(d_ids, d_pk, d_nb, bits, 16000, o)
        assert a.decode_lossy_errors() == 1
    finally:
        a.close()
    # LYRA_HIP_SUBBATCHES=2 (child process: the switch is read at context creation): same results as unsplit
    np.save(tmp_path / "pk.npy", packets); np.save(tmp_path / "mask.npy", mask)
    outs = {}
    for split in ("1", "2"):
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(tmp_path / "pk.npy"), str(tmp_path / "mask.npy"),
                            str(tmp_path / f"out{split}.npy")], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, LYRA_HIP_SUBBATCHES=split))
        assert r.returncode == 0, r.stderr[-3000:]
        outs[split] = np.load(tmp_path / f"out{split}.npy")
    assert np.array_equal(outs["1"], outs["2"])
