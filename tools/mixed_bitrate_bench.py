"""Throughput of per-stream bitrates on the device path: ENCODE | DECODE | PACKET_LOSS at 16 kHz, 4096 streams, 10 % loss from
a seeded two-state Gilbert model per stream (lossy_steps_bench.gilbert, average burst 2), one JSON line per configuration:
  a  uniform      the existing path, every stream at 184 bits (run_steps, num_bits = 184)
  b  mixed_184    LYRA_HIP_STEP_MIXED_BITRATE, every stream at 184 bits
  c  mixed_thirds LYRA_HIP_STEP_MIXED_BITRATE, stream b at (64, 120, 184)[b % 3]
  d  adaptive     LYRA_HIP_STEP_MIXED_BITRATE, stream b at (64, 120, 184)[(hop // 25 + b) % 3]: every stream switches every 25 hops
  e  workaround   the groups of c as three encode_ext_dev + three decode_lossy_dev calls per hop (C calls, no Python per row)
Each configuration runs its warm-up hops, then `hops` timed hops (host clock around the enqueue and a final synchronise),
`repeat` times in rotation (a b c d e a b c d e ...).  The first repetition verifies itself: a subset of streams is replayed
with oracle/lyra_codec_model.py (RefLyraEncoder with .bits set per hop, RefLyraDecoder with SetEncodedPacket on received hops)
and the last two hops must match within the comfort-noise criterion of tests/test_batch_codec_semantics.py (2 LSB), with
is_comfort_noise() exact.
    python tools/mixed_bitrate_bench.py [--streams 4096] [--hops 200] [--warmup 20] [--repeat 3] [--out profiles/x.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lossy_steps_bench import SEED, gilbert, speech_ring  # noqa: E402

RATES = (64, 120, 184)
CONFIGS = ("uniform", "mixed_184", "mixed_thirds", "adaptive", "workaround")


def schedule(cfg, total, B):
    """[total][B] bit count of every stream at every hop."""
    b = np.arange(B)
    if cfg in ("uniform", "mixed_184"):
        return np.full((total, B), 184, np.int32)
    if cfg in ("mixed_thirds", "workaround"):
        return np.tile(np.array(RATES, np.int32)[b % 3], (total, 1))
    return np.stack([np.array(RATES, np.int32)[(t // 25 + b) % 3] for t in range(total)])


class Setup:
    def __init__(self, ctx, B, hops, warmup, seed):
        import torch
        self.dev = torch.device("cuda", 0)
        self.B, self.hops, self.warmup, self.total = B, hops, warmup, warmup + hops
        rng = np.random.default_rng(seed)
        self.n_ring = 64
        self.pcm_ring = speech_ring(self.n_ring, B, rng)
        self.rx = gilbert(rng, self.total, B, 0.10)
        self.ids = np.arange(B, dtype=np.int32)
        self.d_ids = torch.from_numpy(self.ids).to(self.dev)
        self.d_pcm = torch.from_numpy(self.pcm_ring).to(self.dev)
        self.d_rx = torch.from_numpy(self.rx).to(self.dev)
        torch.cuda.synchronize()


def run_steps_cfg(ctx, S, cfg, first, n, kw, ring):
    if cfg == "uniform":
        ctx.run_steps_dev(S.d_ids, 184, n, first_step=first, **kw)
    else:
        ctx.run_steps_dev(S.d_ids, 0, n, first_step=first, d_bits_ring=ring, **kw)


def time_run_steps(ctx, S, cfg):
    import torch
    dev, B = S.dev, S.B
    sched = schedule(cfg, S.total, B)
    o16 = [torch.empty((B, 320), dtype=torch.int16, device=dev) for _ in range(2)]
    pk = [torch.zeros((B, 23), dtype=torch.uint8, device=dev) for _ in range(2)]   # (184 bits: 23 bytes in both forms)
    pb = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2)]
    icn = torch.empty(B, dtype=torch.int32, device=dev)
    # the bits ring: one row per hop of the adaptive schedule's period (75), else one row
    ring = torch.from_numpy(np.ascontiguousarray(sched[:75] if cfg == "adaptive" else sched[:1])).to(dev)
    torch.cuda.synchronize()
    ctx.reset()
    kw = dict(d_pcm_ring=S.d_pcm, d_packets=pk, d_pcm_out=o16, d_received_ring=S.d_rx, d_is_comfort_noise=icn,
              packet_loss=True)
    if cfg != "uniform":
        kw["d_packet_bytes"] = pb
    run_steps_cfg(ctx, S, cfg, 0, S.warmup, kw, ring)
    ctx.synchronize()
    t0 = time.perf_counter()
    run_steps_cfg(ctx, S, cfg, S.warmup, S.hops, kw, ring)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    last = [o16[t & 1].cpu().numpy() for t in (S.total - 2, S.total - 1)]
    return dt, last, icn.cpu().numpy(), sched


def time_workaround(ctx, S):
    """Three encode_ext_dev + three decode_lossy_dev per hop on the groups of mixed_thirds, straight through the C ABI."""
    import torch
    dev, B = S.dev, S.B
    sched = schedule("workaround", S.total, B)
    L, h = ctx.L, ctx.h
    groups = []
    for g, bits in enumerate(RATES):
        sel = np.flatnonzero(np.arange(B) % 3 == g)
        n, nb = sel.size, (bits + 7) // 8
        d = dict(sel=sel, bits=bits, n=n,
                 ids=torch.from_numpy(S.ids[sel]).to(dev),
                 pcm=torch.from_numpy(np.ascontiguousarray(S.pcm_ring[:, sel])).to(dev),
                 sizes=torch.from_numpy(np.ascontiguousarray(S.rx[:, sel].astype(np.int32) * nb)).to(dev),
                 pk=[torch.zeros((n, nb), dtype=torch.uint8, device=dev) for _ in range(2)],
                 o16=[torch.empty((n, 320), dtype=torch.int16, device=dev) for _ in range(2)],
                 icn=torch.empty(n, dtype=torch.int32, device=dev))
        groups.append(d)
    torch.cuda.synchronize()
    ctx.reset()

    def hops(a, b):
        for t in range(a, b):
            k = t & 1
            for d in groups:
                rc = L.lyra_hip_encode_ext_dev(h, d["ids"].data_ptr(), d["n"], d["pcm"][t % S.n_ring].data_ptr(), 16000,
                                               d["bits"], 0, d["pk"][k].data_ptr(), None)
                assert rc == 0, ctx.last_error()
            for d in groups:
                rc = L.lyra_hip_decode_lossy_dev(h, d["ids"].data_ptr(), d["n"], d["pk"][k].data_ptr(), d["sizes"][t].data_ptr(),
                                                 d["bits"], 16000, d["o16"][k].data_ptr(), None, None, d["icn"].data_ptr())
                assert rc == 0, ctx.last_error()

    hops(0, S.warmup)
    ctx.synchronize()
    t0 = time.perf_counter()
    hops(S.warmup, S.total)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    last = [np.zeros((B, 320), np.int16) for _ in range(2)]
    icn = np.zeros(B, np.int32)
    for d in groups:
        for i, t in enumerate((S.total - 2, S.total - 1)):
            last[i][d["sel"]] = d["o16"][t & 1].cpu().numpy()
        icn[d["sel"]] = d["icn"].cpu().numpy()
    return dt, last, icn, sched


def verify(S, last, icn, sched, n, rng):
    from oracle import lyra_codec_model as M, lyra_oracle
    o = lyra_oracle.Oracle(mode="xnnpack")
    sub = np.unique(np.concatenate([[0, 1, 2, S.B - 1], rng.choice(S.B, max(0, n - 4), replace=False)]))
    worst, ok_cn = 0, True
    for b in sub:
        enc = M.RefLyraEncoder(o, 16000, int(sched[0, b]), False)
        dec = M.RefLyraDecoder(o, 16000, cng_seed=SEED ^ int(S.ids[b]))
        for t in range(S.total):
            enc.bits = int(sched[t, b])
            p = enc.Encode(S.pcm_ring[t % S.n_ring, b])
            if S.rx[t, b]:
                dec.SetEncodedPacket(p)
            want = dec.DecodeSamples(320)
            if t >= S.total - 2:
                worst = max(worst, int(np.abs(last[t - (S.total - 2)][b].astype(int) - want.astype(int)).max()))
        ok_cn = ok_cn and int(icn[b]) == int(dec.is_comfort_noise())
    return int(sub.size), worst, bool(worst <= 2 and ok_cn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--hops", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--verify", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import lyra_amd
    ctx = lyra_amd.LyraHip(device=0, max_streams=a.streams)
    ctx.torch_order = False   # the timed loops order themselves (synchronise before and after)
    S = Setup(ctx, a.streams, a.hops, a.warmup, seed=2026)
    res = {c: [] for c in CONFIGS}
    checks = {}
    rng = np.random.default_rng(7)
    try:
        for rep in range(a.repeat):
            for cfg in CONFIGS:
                dt, last, icn, sched = time_workaround(ctx, S) if cfg == "workaround" else time_run_steps(ctx, S, cfg)
                res[cfg].append(S.B * S.hops / dt)
                if rep == 0:
                    checks[cfg] = verify(S, last, icn, sched, a.verify, rng)
                    checks[cfg] += (int(icn.sum()),)
    finally:
        ctx.close()
    lines = []
    for cfg in CONFIGS:
        f = sorted(res[cfg])
        n_ver, worst, ok, cn_end = checks[cfg]
        r = {"tool": "mixed_bitrate_bench", "config": cfg, "flags": "ENCODE|DECODE|PACKET_LOSS" +
             ("|MIXED_BITRATE" if cfg not in ("uniform", "workaround") else ""),
             "calls_per_hop": "6 single calls" if cfg == "workaround" else "run_steps", "streams": S.B, "external_rate": 16000,
             "loss": 0.10, "burst": 2.0, "hops": S.hops, "warmup": S.warmup, "repeat": a.repeat,
             "frames_per_s_median": round(float(np.median(f))), "frames_per_s_min": round(f[0]), "frames_per_s_max": round(f[-1]),
             "comfort_noise_streams_at_end": cn_end, "received_fraction": round(float(S.rx[S.warmup:].mean()), 4),
             "verified_streams": n_ver, "max_lsb_diff": worst, "verified": ok}
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        with open(a.out, "a") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")
    return 0 if all(r["verified"] for r in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
