"""lyra_hip_decode_lossy_dev / LYRA_HIP_STEP_PACKET_LOSS: LyraDecoder's packet-loss concealment, comfort noise and
cross-fades (lyra_decoder.cc:172-373) on the device path, for hop-synchronous receivers.  Expectations: the per-stream
reference model oracle/lyra_codec_model.py (RefLyraDecoder, DecodeSamples(rate / 50) per tick, SetEncodedPacket only on
ticks with a packet) sample for sample -- exact where only the generative model speaks, within 1 LSB where comfort noise
goes in (Tally, LossyModel; also used by the BatchLyraDecoder tests), is_noise and the decoder-side estimate included --
up to full batches; BatchLyraDecoder through lyra_amd/decoder_demo (bit for bit), the existing device path when every
packet arrives (bit for bit), and run_steps against the single calls (bit for bit).

Stream kind: the contexts here (64 to 512 streams) run on the CU-masked streams the library picks up to 1,024 streams, which
are blocking streams with respect to the NULL stream; the case with streams="plain" runs on hipStreamNonBlocking streams, the
kind of a 4,096-stream context (tests/gpu_plumbing.py make_ctx)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from gpu_plumbing import make_ctx, stream_cases
from receiver_models import BYTES, CnReach, LossyModel, _full_batch_mask, _lossy_check, _lossy_run, cn_flags
from signals import _patterns, _speech

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _ctx(max_streams=256, streams=None):
    return make_ctx(max_streams, streams=streams)


@pytest.mark.parametrize("rate", [8000, 32000, 48000])
def test_cn_reach_covers_the_resampler(golden_dir, oracle_default, rate):
    """CPU: CnReach is sound.  A model decoder through loss, comfort noise and both fades, played out in odd request
    sizes; its internal stream resampled again with every comfort-noise sample replaced by +-12000 (the far end of the filter
    counts too): the played samples that change must all be flagged, and most flagged ones change."""
    from oracle import lyra_codec_model as M, lyra_oracle
    T = 30
    pcm = _speech(golden_dir, 1, T)[:, 0]
    enc = M.RefLyraEncoder(oracle_default, 16000, 120, False)
    dec = M.RefLyraDecoder(oracle_default, rate, cng_seed=3)
    reach, rs = CnReach(rate), lyra_oracle.Resampler(16000, rate)
    hop = rate // 50
    out, flags, moved = [], [], []
    for t in range(T):
        p = enc.Encode(pcm[t])
        if not 4 <= t < 13 and t != 16:
            dec.SetEncodedPacket(p)
        for k in ([hop] if t % 3 == 0 else [hop // 3 + 1, hop - hop // 3 - 1] if t % 3 == 1 else [1, hop - 1]):
            out.append(dec.DecodeSamples(k))
            flags.append(reach(dec, k))
            x = np.where(cn_flags(dec), np.where(dec.last_internal < 0, 12000, -12000), dec.last_internal)
            moved.append(rs.Resample(x.astype(np.int16)))
    out, flags = np.concatenate(out), np.concatenate(flags)
    moved = np.concatenate(moved)[:out.size]
    changed = moved != out
    assert flags.sum() > 1000 and not (changed & ~flags).any()
    assert changed[flags].mean() > 0.9, changed[flags].mean()


@pytest.mark.gpu
@pytest.mark.parametrize("rate,bits", [(8000, 184), (16000, 64), (32000, 120), (48000, 184)])
def test_lossy_sessions_vs_reference_model(golden_dir, oracle_default, rate, bits):
    from oracle import lyra_codec_model as M
    T, ids = 36, [5, 17, 2, 40]
    pcm = _speech(golden_dir, 4, T)
    mask = _patterns(T)
    encs = [M.RefLyraEncoder(oracle_default, 16000, bits, False) for _ in ids]
    packets = np.stack([np.stack([encs[s].Encode(pcm[t, s]) for s in range(4)]) for t in range(T)])
    model = LossyModel(oracle_default, rate, ids)
    ctx = _ctx()
    try:
        _lossy_check(ctx, model, ids, packets, mask, bits)
    finally:
        ctx.close()
    model.tally.report(f"lossy sessions {rate} Hz")
    assert model.tally.exact_fraction() > 0.97
    assert model.saw_cn and model.saw_mix and model.saw_back


def _lossy_full_batch(golden_dir, oracle, rate, bits, B, T, mask, max_streams, seed, streams=None):
    from oracle import lyra_codec_model as M
    rng = np.random.default_rng(seed)
    ids = rng.choice(max_streams - 1, B - 1, replace=False).tolist() + [max_streams - 1]
    ids = np.array(ids, np.int32)[rng.permutation(B)]
    pcm = _speech(golden_dir, B, T, offset=int(rng.integers(0, 20000)))
    encs = [M.RefLyraEncoder(oracle, 16000, bits, False) for _ in range(B)]
    packets = np.stack([np.stack([encs[s].Encode(pcm[t, s]) for s in range(B)]) for t in range(T)])
    model = LossyModel(oracle, rate, ids)
    ctx = _ctx(max_streams, streams)
    try:
        _lossy_check(ctx, model, ids, packets, mask, bits)
        assert ctx.decode_lossy_errors() == 0
    finally:
        ctx.close()
    model.tally.report(f"full batch B={B} {rate} Hz")
    assert model.tally.exact_fraction() > 0.97
    return model


@pytest.mark.gpu
@pytest.mark.parametrize("rate,bits,B,streams", stream_cases([(16000, 120, 263), (8000, 64, 37), (32000, 184, 37), (48000, 120, 37)],
                                                             plain=(48000, 120, 37)))
def test_lossy_full_batch_vs_reference_model(golden_dir, oracle_default, rate, bits, B, streams):
    """Past one workgroup of every kernel of the tick, with scattered ids up to max_streams - 1 and distinct speech per
    stream: lossy_plan_kernel's blocks of 256 rows and their feature zeroing, logmel_masked_kernel's pairs in all four
    received / lost combinations at every tick, lossy_mix_kernel's and resample_kernel's tiles of 4 rows (one all lost),
    cng_kernel's masked rows -- every sample, is_noise and the decoder-side estimate against the reference model."""
    T = 44
    mask = _full_batch_mask(T, B, np.random.default_rng(rate + B))
    for t in range(T):
        pairs = {(int(mask[t, 2 * k]), int(mask[t, 2 * k + 1])) for k in range(B // 2)}
        assert pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}, t
    assert any((mask[t, 4 * j:4 * j + 4] == 0).all() for t in range(T) for j in range(B // 4))
    model = _lossy_full_batch(golden_dir, oracle_default, rate, bits, B, T, mask, 512, rate + B, streams)
    assert model.saw_back >= 2 and model.saw_mix and model.saw_cn


@pytest.mark.gpu
@pytest.mark.parametrize("rate,B", [(48000, 1), (16000, 2)])
def test_lossy_tiny_batch_vs_reference_model(golden_dir, oracle_default, rate, B):
    """B = 1 (a lone row in every kernel's first workgroup) and B = 2 with one row lost while the other is received."""
    T = 36
    m = _patterns(T)[:, 3]
    mask = np.stack([m, 1 - m] if B == 2 else [m], axis=1).astype(np.uint8)
    mask[30:33, :] = 0
    model = _lossy_full_batch(golden_dir, oracle_default, rate, 184, B, T, mask, 64, B)
    assert model.saw_back >= 1 and model.saw_mix and model.saw_cn


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
    # single calls, hop by hop, each against the reference models
    encs = [M.RefLyraEncoder(oracle_default, 16000, bits, True) for _ in ids]
    model = LossyModel(oracle_default, 16000, ids)
    saw_cn = False
    prev_rx = np.ones(B, np.uint8)
    ctx = _ctx()
    try:
        pk, nb, o16, isn, icn = mk((B, 8), torch.uint8), mk(B, torch.int32), mk((B, 320), torch.int16), mk(B, torch.int32), mk(B, torch.int32)
        ref = []
        for t in range(T):
            k = t & 1
            ctx.encode_dtx_dev(d_ids, d_pcm[t], bits, pk[k], nb[k])
            eff = nb[k] * d_rx[t].to(torch.int32)
            ctx.decode_lossy_dev(d_ids, pk[k], eff, bits, 16000, o16[k], None, isn[k], icn[k])
            ctx.synchronize()
            ref.append((o16[k].cpu().numpy().copy(), isn[k].cpu().numpy().copy(), icn[k].cpu().numpy().copy()))
            got_nb, got_pk = nb[k].cpu().numpy(), pk[k].cpu().numpy()
            got_rx = np.zeros(B, np.uint8)
            for s in range(B):
                p = encs[s].Encode(pcm[t, s])
                assert got_nb[s] == p.size, (t, s)
                if p.size:
                    assert np.array_equal(got_pk[s], p), (t, s)
                    got_rx[s] = rx[t, s]
            model.tick(t, got_pk, got_rx, (ref[t][0], ref[t][0], ref[t][1], ref[t][2]))
            if t % 5 == 4 or (got_rx & ~prev_rx).any():
                model.check_estimates(ctx, f"tick {t}")
            prev_rx = got_rx
            saw_cn = saw_cn or any(model.decs[s].is_comfort_noise() for s in (1, 3))
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
        model.check_estimates(ctx, "after run_steps")
    finally:
        ctx.close()
    model.tally.report("run_steps ENCODE | DTX | PACKET_LOSS")
    assert model.tally.exact_fraction() > 0.97
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
