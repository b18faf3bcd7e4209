#!/usr/bin/env python3
"""Time lyra_hip_export_streams_dev / lyra_hip_import_streams_dev against a device-to-device copy of the same bytes.
   python tools/stream_state_bench.py [--out profiles/stream_state.jsonl]
For 4096 streams and for 1: export, import and the copy alternate in one run, each timed around the call on an otherwise
idle context (the calls drain the context themselves); median of 5 with min..max, GB/s counting the blob bytes once read
and once written, and the ratio to the copy.  The copy is the yardstick because the kernels move the same bytes, in 12
strided pieces per row."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import lyra_amd
    dev = torch.device("cuda", 0)
    ctx = lyra_amd.LyraHip(device=0, max_streams=4096)
    nbytes = ctx.stream_blob_bytes()
    lines = []
    for B in (4096, 1):
        ids = torch.arange(B, dtype=torch.int32, device=dev)
        blobs = torch.zeros((B, nbytes), dtype=torch.uint8, device=dev)
        other = torch.zeros_like(blobs)
        ctx.export_streams_dev(ids, blobs)      # warm-up: allocations, code objects
        ctx.import_streams_dev(ids, blobs)
        other.copy_(blobs)
        torch.cuda.synchronize()
        t = {"export": [], "import": [], "copy": []}
        for _ in range(args.reps):
            for name, fn in (("export", lambda: ctx.export_streams_dev(ids, blobs)),
                             ("import", lambda: ctx.import_streams_dev(ids, blobs)),
                             ("copy", lambda: (other.copy_(blobs), torch.cuda.synchronize()))):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                t[name].append(time.perf_counter() - t0)
        assert ctx.import_errors() == 0
        rec = {"streams": B, "bytes": B * nbytes}
        for name, v in t.items():
            v = sorted(v)
            med = v[len(v) // 2]
            rec[name] = {"ms_median": med * 1e3, "ms_min": v[0] * 1e3, "ms_max": v[-1] * 1e3, "GBps": 2 * B * nbytes / med / 1e9}
        for name in ("export", "import"):
            rec[name]["ratio_to_copy"] = rec["copy"]["ms_median"] / rec[name]["ms_median"]
        lines.append(json.dumps(rec))
        print(lines[-1])
    ctx.close()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
