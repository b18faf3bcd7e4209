"""Throughput of per-stream sample rates on the device path: ENCODE | DECODE | PACKET_LOSS, 184 bits, 4096 streams, 10 % loss
from a seeded two-state Gilbert model per stream (lossy_steps_bench.gilbert, average burst 2), one JSON line per configuration:
  uniform_16k / uniform_48k   the existing path (run_steps, external_rate 0 / 48000)
  rates_all16 / rates_all48   LYRA_HIP_STEP_MIXED_RATE, every row at one rate
  rates_quarters              LYRA_HIP_STEP_MIXED_RATE, stream b at (8000, 16000, 32000, 48000)[b % 4]
  workaround                  the groups of rates_quarters as four encode_mixed_dev + four decode_lossy_mixed_dev calls per hop
                              (C calls, no Python per row)
Each configuration runs its warm-up hops, then `hops` timed hops (host clock around the enqueue and a final synchronise),
`repeat` times in rotation.  The first repetition verifies itself: a subset of streams is replayed with
oracle/lyra_codec_model.py (RefLyraEncoder / RefLyraDecoder created at the stream's rate) and the last two external-rate hops
must match within the comfort-noise criterion of tests/test_batch_codec_semantics.py (2 LSB), is_comfort_noise() exact.
    python tools/mixed_rate_bench.py [--streams 4096] [--hops 200] [--warmup 20] [--repeat 3] [--out profiles/x.jsonl]"""
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

QUARTERS = (8000, 16000, 32000, 48000)
CONFIGS = ("uniform_16k", "uniform_48k", "rates_all16", "rates_all48", "rates_quarters", "workaround")
BITS, ROW = 184, 960


def rates_of(cfg, B):
    if cfg in ("uniform_16k", "rates_all16"):
        return np.full(B, 16000, np.int32)
    if cfg in ("uniform_48k", "rates_all48"):
        return np.full(B, 48000, np.int32)
    return np.array(QUARTERS, np.int32)[np.arange(B) % 4]


def at_rate(pcm16, rate):
    """[..., 320] at 16 kHz -> [..., rate / 50]: samples repeated / every second one (any int16 input is a valid hop)."""
    return np.repeat(pcm16, rate // 16000, axis=-1) if rate >= 16000 else np.ascontiguousarray(pcm16[..., ::2])


class Setup:
    def __init__(self, B, hops, warmup, seed):
        import torch
        self.dev = torch.device("cuda", 0)
        self.B, self.hops, self.warmup, self.total = B, hops, warmup, warmup + hops
        rng = np.random.default_rng(seed)
        self.n_ring = 32
        self.pcm16 = speech_ring(self.n_ring, B, rng)
        self.rx = gilbert(rng, self.total, B, 0.10)
        self.ids = np.arange(B, dtype=np.int32)
        self.d_ids = torch.from_numpy(self.ids).to(self.dev)
        self.d_rx = torch.from_numpy(self.rx).to(self.dev)


def time_run_steps(ctx, S, cfg):
    import torch
    dev, B = S.dev, S.B
    rates = rates_of(cfg, B)
    per_row = cfg.startswith("rates_")
    n_ext = ROW if per_row else int(rates[0]) // 50
    ring = np.zeros((S.n_ring, B, n_ext), np.int16)
    for r in np.unique(rates):
        sel = np.flatnonzero(rates == r)
        ring[:, sel, :r // 50] = at_rate(S.pcm16[:, sel], int(r))
    d_ring = torch.from_numpy(ring).to(dev)
    o16 = [torch.empty((B, 320), dtype=torch.int16, device=dev) for _ in range(2)]
    ext = [torch.zeros((B, n_ext), dtype=torch.int16, device=dev) for _ in range(2)]
    pk = [torch.zeros((B, 23), dtype=torch.uint8, device=dev) for _ in range(2)]
    pb = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2)]
    icn = torch.empty(B, dtype=torch.int32, device=dev)
    kw = dict(d_pcm_ring=d_ring, d_packets=pk, d_pcm_out=o16, d_received_ring=S.d_rx, d_is_comfort_noise=icn, packet_loss=True)
    if per_row:
        kw.update(d_rates=torch.from_numpy(rates).to(dev), d_packet_bytes=pb, d_ext_out=ext)
    elif rates[0] != 16000:
        kw.update(external_rate=int(rates[0]), d_ext_out=ext)
    torch.cuda.synchronize()
    ctx.reset()
    ctx.run_steps_dev(S.d_ids, BITS, S.warmup, first_step=0, **kw)
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.run_steps_dev(S.d_ids, BITS, S.hops, first_step=S.warmup, **kw)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    src = ext if (per_row or rates[0] != 16000) else o16
    last = [src[t & 1].cpu().numpy() for t in (S.total - 2, S.total - 1)]
    return dt, last, icn.cpu().numpy(), rates


def time_workaround(ctx, S):
    import torch
    dev, B = S.dev, S.B
    rates = rates_of("workaround", B)
    L, h = ctx.L, ctx.h
    groups = []
    for r in QUARTERS:
        sel = np.flatnonzero(rates == r)
        n = sel.size
        groups.append(dict(sel=sel, rate=r, n=n, ids=torch.from_numpy(S.ids[sel]).to(dev),
                           pcm=torch.from_numpy(at_rate(S.pcm16[:, sel], r)).to(dev),
                           bits=torch.full((n,), BITS, dtype=torch.int32, device=dev),
                           sizes=torch.from_numpy(np.ascontiguousarray(S.rx[:, sel].astype(np.int32) * 23)).to(dev),
                           pk=[torch.zeros((n, 23), dtype=torch.uint8, device=dev) for _ in range(2)],
                           pb=[torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2)],
                           o16=[torch.empty((n, 320), dtype=torch.int16, device=dev) for _ in range(2)],
                           ext=[torch.empty((n, r // 50), dtype=torch.int16, device=dev) for _ in range(2)],
                           icn=torch.empty(n, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    ctx.reset()

    def hops(a, b):
        for t in range(a, b):
            k = t & 1
            for d in groups:
                rc = L.lyra_hip_encode_mixed_dev(h, d["ids"].data_ptr(), d["n"], d["pcm"][t % S.n_ring].data_ptr(), d["rate"],
                                                 d["bits"].data_ptr(), 0, d["pk"][k].data_ptr(), d["pb"][k].data_ptr())
                assert rc == 0, ctx.last_error()
            for d in groups:
                rc = L.lyra_hip_decode_lossy_mixed_dev(h, d["ids"].data_ptr(), d["n"], d["pk"][k].data_ptr(),
                                                       d["sizes"][t].data_ptr(), d["rate"], d["o16"][k].data_ptr(),
                                                       d["ext"][k].data_ptr(), None, d["icn"].data_ptr())
                assert rc == 0, ctx.last_error()

    hops(0, S.warmup)
    ctx.synchronize()
    t0 = time.perf_counter()
    hops(S.warmup, S.total)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    last = [np.zeros((B, ROW), np.int16) for _ in range(2)]
    icn = np.zeros(B, np.int32)
    for d in groups:
        for i, t in enumerate((S.total - 2, S.total - 1)):
            last[i][d["sel"], :d["rate"] // 50] = (d["ext"] if d["rate"] != 16000 else d["o16"])[t & 1].cpu().numpy()
        icn[d["sel"]] = d["icn"].cpu().numpy()
    return dt, last, icn, rates


def verify(S, last, icn, rates, n, rng):
    from oracle import lyra_codec_model as M, lyra_oracle
    o = lyra_oracle.Oracle(mode="xnnpack")
    sub = np.unique(np.concatenate([[0, 1, 2, 3], rng.choice(S.B, max(0, n - 4), replace=False)]))
    worst, ok_cn = 0, True
    for b in sub:
        r = int(rates[b])
        enc = M.RefLyraEncoder(o, r, BITS, False)
        dec = M.RefLyraDecoder(o, r, cng_seed=SEED ^ int(S.ids[b]))
        for t in range(S.total):
            p = enc.Encode(at_rate(S.pcm16[t % S.n_ring, b], r))
            if S.rx[t, b]:
                dec.SetEncodedPacket(p)
            want = dec.DecodeSamples(r // 50)
            if t >= S.total - 2:
                got = last[t - (S.total - 2)][b, :r // 50]
                worst = max(worst, int(np.abs(got.astype(int) - want.astype(int)).max()))
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
    ap.add_argument("--configs", default=",".join(CONFIGS), help="comma-separated subset, e.g. for a kernel trace of one")
    a = ap.parse_args()
    import lyra_amd
    ctx = lyra_amd.LyraHip(device=0, max_streams=a.streams)
    ctx.torch_order = False   # the timed loops order themselves (synchronise before and after)
    S = Setup(a.streams, a.hops, a.warmup, seed=2026)
    configs = tuple(a.configs.split(","))
    assert all(c in CONFIGS for c in configs), configs
    res = {c: [] for c in configs}
    checks = {}
    rng = np.random.default_rng(7)
    try:
        for rep in range(a.repeat):
            for cfg in configs:
                dt, last, icn, rates = time_workaround(ctx, S) if cfg == "workaround" else time_run_steps(ctx, S, cfg)
                res[cfg].append(S.B * S.hops / dt)
                if rep == 0:
                    checks[cfg] = (0, 0, True, int(icn.sum())) if a.verify == 0 else verify(S, last, icn, rates, a.verify, rng) + (int(icn.sum()),)
    finally:
        ctx.close()
    lines = []
    for cfg in configs:
        n_ver, worst, ok, cn_end = checks[cfg]
        r = {"tool": "mixed_rate_bench", "config": cfg, "flags": "ENCODE|DECODE|PACKET_LOSS" +
             ("|MIXED_RATE" if cfg.startswith("rates_") else ""),
             "calls_per_hop": "8 single calls" if cfg == "workaround" else "run_steps", "streams": S.B, "num_bits": BITS,
             "loss": 0.10, "burst": 2.0, "hops": S.hops, "warmup": S.warmup, "repeat": a.repeat,
             "frames_per_s": [round(x) for x in res[cfg]], "frames_per_s_median": round(float(np.median(res[cfg]))),
             "comfort_noise_streams_at_end": cn_end, "verified_streams": n_ver, "max_lsb_diff": worst, "verified": ok}
        print(json.dumps(r), flush=True)
        lines.append(r)
    faster = True
    if "rates_quarters" in res and "workaround" in res:
        faster = all(q > w for q, w in zip(res["rates_quarters"], res["workaround"]))
        print(json.dumps({"tool": "mixed_rate_bench", "rates_quarters_faster_than_workaround_in_every_repeat": faster}), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")
    return 0 if faster and all(r["verified"] for r in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
