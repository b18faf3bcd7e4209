"""Throughput of the device-resident packet-loss decode (lyra_hip_run_steps_dev with LYRA_HIP_STEP_PACKET_LOSS): one JSON
line per configuration --
  decode-only at 16 kHz and 48 kHz, and ENCODE | DTX | DECODE | PACKET_LOSS at 16 kHz, 4096 streams,
  0 / 5 / 10 / 20 % loss from a seeded two-state Gilbert model per stream (gilbert_model.cc: received -> lost with
  p = loss / (burst * (1 - loss)), lost -> received with 1 / burst; average burst length 2).
Every configuration runs its hops from ONE run_steps call (after a warm-up call) and then verifies itself: the last two
hops of a subset of streams are replayed with oracle/lyra_codec_model.py (RefLyraEncoder with DTX where the encoder runs,
RefLyraDecoder with SetEncodedPacket only on received, non-empty packets) -- PCM within the comfort-noise criterion of
tests/test_batch_codec_semantics.py (2 LSB), is_comfort_noise() exact.
    python tools/lossy_steps_bench.py [--streams 4096] [--hops 200] [--warmup 20] [--out profiles/lossy_steps.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

SEED = 0x4C797261


def gilbert(rng, n_steps, B, loss, burst=2.0):
    """[n_steps][B] uint8, 1 = received (GilbertModel::IsPacketReceived, one chain per stream, starting received)."""
    rx = np.ones((n_steps, B), np.uint8)
    if loss <= 0:
        return rx
    p_lost = loss / (burst * (1.0 - loss))
    p_back = 1.0 / burst
    received = np.ones(B, bool)
    for t in range(n_steps):
        rx[t] = received
        u = rng.random(B)
        received = np.where(received, u >= p_lost, u < p_back)
    return rx


def speech_ring(n_frames, B, rng, silent_every=0):
    sp = np.load(os.path.join(ROOT, "tests", "golden", "sample_wavs.npz"))["sample1_16kHz"].astype(np.int16)
    ring = np.empty((n_frames, B, 320), np.int16)
    starts = rng.integers(0, sp.size - n_frames * 320, B)
    for b in range(B):
        ring[:, b] = sp[starts[b]:starts[b] + n_frames * 320].reshape(n_frames, 320)
    if silent_every:   # every silent_every-th stream is silent in the second half of the ring (DTX sends empty packets)
        ring[n_frames // 2:, ::silent_every] = 0
    return ring


def run(ctx, mode, rate, B, hops, warmup, loss, verify_n, seed):
    import torch
    from oracle import lyra_codec_model as M, lyra_oracle
    dev = torch.device("cuda", 0)
    bits = 120
    nbytes = 15
    rng = np.random.default_rng(seed)
    total = warmup + hops
    ids = np.arange(B, dtype=np.int32)
    d_ids = torch.from_numpy(ids).to(dev)
    rx = gilbert(rng, total, B, loss)
    d_rx = torch.from_numpy(rx).to(dev)
    n_ext = rate // 50
    o16 = [torch.empty((B, 320), dtype=torch.int16, device=dev) for _ in range(2)]
    oext = [torch.empty((B, n_ext), dtype=torch.int16, device=dev) for _ in range(2)] if rate != 16000 else None
    isn = torch.empty(B, dtype=torch.int32, device=dev)
    icn = torch.empty(B, dtype=torch.int32, device=dev)
    ctx.reset()
    kw = dict(d_pcm_out=o16, d_ext_out=oext, external_rate=rate, d_received_ring=d_rx, d_is_noise=isn,
              d_is_comfort_noise=icn, packet_loss=True)
    n_ring = 64
    if mode == "decode":
        pk_ring = rng.integers(0, 256, size=(n_ring, B, nbytes), dtype=np.uint8)
        kw.update(d_packet_ring=torch.from_numpy(pk_ring).to(dev), encode=False)
    else:
        ctx.set_encoder_sample_rate(16000)
        pcm_ring = speech_ring(n_ring, B, rng, silent_every=3)
        kw.update(d_pcm_ring=torch.from_numpy(pcm_ring).to(dev),
                  d_packets=[torch.zeros((B, nbytes), dtype=torch.uint8, device=dev) for _ in range(2)],
                  d_packet_bytes=[torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2)], dtx=True)
    ctx.run_steps_dev(d_ids, bits, warmup, first_step=0, **kw)
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.run_steps_dev(d_ids, bits, hops, first_step=warmup, **kw)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    last = [(o16[t & 1] if oext is None else oext[t & 1]).cpu().numpy() for t in (total - 2, total - 1)]
    cn = icn.cpu().numpy()
    # self-verification: replay a subset of streams from step 0
    o = lyra_oracle.Oracle(mode="xnnpack")
    sub = np.unique(np.concatenate([[0, 1, 2, B - 1], rng.choice(B, max(0, verify_n - 4), replace=False)]))
    worst, ok_cn = 0, True
    for b in sub:
        dec = M.RefLyraDecoder(o, rate, cng_seed=SEED ^ int(ids[b]))
        enc = M.RefLyraEncoder(o, 16000, bits, True) if mode != "decode" else None
        for t in range(total):
            p = pk_ring[t % n_ring, b] if enc is None else enc.Encode(pcm_ring[t % n_ring, b])
            if p.size and rx[t, b]:
                dec.SetEncodedPacket(p)
            want = dec.DecodeSamples(rate // 50)
            if t >= total - 2:
                worst = max(worst, int(np.abs(last[t - (total - 2)][b].astype(int) - want.astype(int)).max()))
        ok_cn = ok_cn and int(cn[b]) == int(dec.is_comfort_noise())
    flags = "DECODE|PACKET_LOSS" if mode == "decode" else "ENCODE|DTX|DECODE|PACKET_LOSS"
    return {"tool": "lossy_steps_bench", "flags": flags, "streams": B, "external_rate": rate, "num_bits": bits,
            "loss": loss, "burst": 2.0, "hops": hops, "warmup": warmup, "ms_per_hop": round(dt * 1e3 / hops, 4),
            "frames_per_s": round(B * hops / dt), "comfort_noise_streams_at_end": int(cn.sum()),
            "received_fraction": round(float(rx[warmup:].mean()), 4), "verified_streams": int(sub.size),
            "max_lsb_diff": worst, "verified": bool(worst <= 2 and ok_cn)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--hops", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--verify", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import lyra_amd
    ctx = lyra_amd.LyraHip(device=0, max_streams=a.streams)
    lines = []
    try:
        for mode, rate in (("decode", 16000), ("decode", 48000), ("encode", 16000)):
            for i, loss in enumerate((0.0, 0.05, 0.10, 0.20)):
                r = run(ctx, mode, rate, a.streams, a.hops, a.warmup, loss, a.verify, seed=1000 + i)
                print(json.dumps(r), flush=True)
                lines.append(r)
    finally:
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    return 0 if all(r["verified"] for r in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
