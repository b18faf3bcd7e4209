"""Throughput of lyra_hip_decode_samples_dev (LyraDecoder's loss state machine for any request size, on the device): one
JSON line per configuration, appended to --out --
  4096 streams, 16 and 48 kHz, Gilbert loss with burst 2 at 0 % and 10 % (one chain per stream, tools/lossy_steps_bench.py),
  "hop":  n = one hop, against lyra_hip_decode_lossy_mixed_dev on the same packets on a second context -- the same device
          work plus the larger plan kernel; the two calls ALTERNATE, window by window, in one run;
  "10ms": n = 10 ms, a packet every second call (two calls per hop of audio).
Every shape is warmed up first; a timed window is `hops` hops of calls enqueued back to back and ends in a synchronise;
`reps` windows per configuration, median and min..max spread reported as decoded hops (stream-frames of 20 ms) per second.
    python tools/decode_samples_bench.py [--streams 4096] [--hops 100] [--reps 7] [--out profiles/decode_samples.jsonl]"""
import argparse
import json
import os
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_samples.jsonl"))
    a = ap.parse_args()
    B, dev = a.streams, torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    ring = 16    # distinct packet sets; the packets are random codes (the decoder's work does not depend on them)
    d_pk = torch.from_numpy(rng.integers(0, 256, (ring, B, 23), dtype=np.uint8)).to(dev)
    size = np.array([8, 15, 23], np.int32)[np.arange(B) % 3]
    d_ids = torch.arange(B, dtype=torch.int32, device=dev)
    d_none = torch.zeros(B, dtype=torch.int32, device=dev)
    new, old = lyra_amd.LyraHip(device=0, max_streams=B), lyra_amd.LyraHip(device=0, max_streams=B)
    lines = []
    try:
        for rate in (16000, 48000):
            hop = rate // 50
            o16 = [torch.zeros((B, 320), dtype=torch.int16, device=dev) for _ in range(2)]
            oh = [torch.zeros((B, hop), dtype=torch.int16, device=dev) for _ in range(2)]
            o10 = [torch.zeros((B, hop // 2), dtype=torch.int16, device=dev) for _ in range(2)]
            for loss in (0.0, 0.10):
                rx = gilbert(rng, a.hops, B, loss)
                d_nb = [torch.from_numpy(rx[t].astype(np.int32) * size).to(dev) for t in range(a.hops)]

                def w_new_hop():
                    for t in range(a.hops):
                        new.decode_samples_dev(d_ids, d_pk[t % ring], d_nb[t], hop, rate, oh[t & 1])

                def w_old_hop():
                    for t in range(a.hops):
                        old.decode_lossy_mixed_dev(d_ids, d_pk[t % ring], d_nb[t], rate, o16[t & 1],
                                                   oh[t & 1] if rate != 16000 else None)

                def w_new_10ms():
                    for t in range(a.hops):
                        new.decode_samples_dev(d_ids, d_pk[t % ring], d_nb[t], hop // 2, rate, o10[0])
                        new.decode_samples_dev(d_ids, d_pk[t % ring], d_none, hop // 2, rate, o10[1])

                windows = {"hop_new": (w_new_hop, new), "hop_lossy_mixed": (w_old_hop, old), "10ms_new": (w_new_10ms, new)}
                times = {k: [] for k in windows}
                for rep in range(a.reps + 1):          # rep 0 warms every shape up and is not counted
                    for name, (fn, ctx) in windows.items():
                        ctx.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        ctx.synchronize()
                        if rep:
                            times[name].append(time.perf_counter() - t0)
                line = {"bench": "decode_samples", "streams": B, "rate": rate, "loss": loss, "hops": a.hops, "reps": a.reps}
                for name, ts in times.items():
                    f = sorted(B * a.hops / t for t in ts)
                    line[name] = {"frames_per_s_median": round(f[len(f) // 2]), "min": round(f[0]), "max": round(f[-1])}
                line["errors"] = int(new.decode_samples_errors())
                print(json.dumps(line), flush=True)
                lines.append(line)
    finally:
        new.close()
        old.close()
    # (a) the public C++ classes on host buffers, 10 ms requests: BatchLyraDecoder against DeviceLyraDecoder, blocking and
    # pipelined, all four driven and timed by lyra_amd/device_decoder_demo --bench in one process per configuration
    import subprocess
    demo = os.path.join(ROOT, "lyra_amd", "device_decoder_demo")
    for rate in (16000, 48000):
        for loss in (0, 10):
            r = subprocess.run([demo, "--bench", lyra_amd.default_model_dir(), str(rate), str(B), str(a.hops), str(loss),
                                str(a.reps)], capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"device_decoder_demo --bench failed ({r.returncode}): {r.stderr[-2000:]}")
            line = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
