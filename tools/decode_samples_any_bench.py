"""Throughput of lyra_hip_decode_samples_any_dev (DecodeSamples(n) for any n of up to four hops on the device): one JSON line
per configuration, appended to --out --
  "480":   4096 streams, 48 kHz, 480 frames per call, a packet every second call, Gilbert loss at 10 %: the new call against
           lyra_hip_decode_samples_dev on the same packets on a second context, the two ALTERNATING window by window in one
           run -- the old call is the baseline for what the splice kernel and the per-row totals cost;
  "class": AnySizeDeviceLyraDecoder against BatchLyraDecoder on host buffers, blocking and pipelined, on one script, driven
           and timed by lyra_amd/device_decoder_demo --bench-any: 48 kHz with callbacks of 128 and of 1024 frames, 16 kHz
           with 1024 frames, 10 % Gilbert loss.
Every shape is warmed up first; `reps` windows per configuration, median and min..max as decoded hops (20 ms) per second.
    python tools/decode_samples_any_bench.py [--streams 4096] [--hops 100] [--reps 5] [--out profiles/decode_samples_any.jsonl]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    import torch
    import lyra_amd
    from lossy_steps_bench import gilbert
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--hops", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_samples_any.jsonl"))
    a = ap.parse_args()
    B, dev = a.streams, torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    ring = 16    # distinct packet sets; the packets are random codes (the decoder's work does not depend on them)
    d_pk = torch.from_numpy(rng.integers(0, 256, (ring, B, 23), dtype=np.uint8)).to(dev)
    size = np.array([8, 15, 23], np.int32)[np.arange(B) % 3]
    d_ids = torch.arange(B, dtype=torch.int32, device=dev)
    d_none = torch.zeros(B, dtype=torch.int32, device=dev)
    rate, loss = 48000, 0.10
    lines = []
    new, old = lyra_amd.LyraHip(device=0, max_streams=B), lyra_amd.LyraHip(device=0, max_streams=B)
    try:
        out = [torch.zeros((B, 480), dtype=torch.int16, device=dev) for _ in range(2)]
        rx = gilbert(rng, a.hops, B, loss)
        d_nb = [torch.from_numpy(rx[t].astype(np.int32) * size).to(dev) for t in range(a.hops)]

        def window(call):
            for t in range(a.hops):
                call(d_ids, d_pk[t % ring], d_nb[t], 480, rate, out[0])
                call(d_ids, d_pk[t % ring], d_none, 480, rate, out[1])

        windows = {"any": (new.decode_samples_any_dev, new), "one_hop_call": (old.decode_samples_dev, old)}
        times = {k: [] for k in windows}
        for rep in range(a.reps + 1):          # rep 0 warms every shape up and is not counted
            for name, (call, ctx) in windows.items():
                ctx.synchronize()
                t0 = time.perf_counter()
                window(call)
                ctx.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
        line = {"bench": "decode_samples_any", "streams": B, "rate": rate, "frames": 480, "loss": loss, "hops": a.hops,
                "reps": a.reps}
        for name, ts in times.items():
            f = sorted(B * a.hops / t for t in ts)
            line[name] = {"frames_per_s_median": round(f[len(f) // 2]), "min": round(f[0]), "max": round(f[-1])}
        line["errors"] = int(new.decode_samples_errors()) + int(old.decode_samples_errors())
        print(json.dumps(line), flush=True)
        lines.append(line)
    finally:
        new.close()
        old.close()
    demo = os.path.join(ROOT, "lyra_amd", "device_decoder_demo")
    for rate, cb in ((48000, 128), (48000, 1024), (16000, 1024)):
        r = subprocess.run([demo, "--bench-any", lyra_amd.default_model_dir(), str(rate), str(B), str(a.hops), "10", str(a.reps),
                            str(cb)], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"device_decoder_demo --bench-any failed ({r.returncode}): {r.stderr[-2000:]}")
        line = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(line), flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
