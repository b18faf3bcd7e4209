#!/usr/bin/env python3
"""Time MixedBatchLyraDecoder against what the classes before it offer, through lyra_amd/mixed_decoder_demo --bench.
   python tools/mixed_decoder_bench.py [--out profiles/mixed_decoders.jsonl] [--streams 4096] [--hops 1000] [--windows 5]
Every comparison is ONE run of the demo with the engines' windows alternating: host buffers, two hops deep, random 15-byte
packets under Gilbert loss (10 %, mean burst 2), the same packets and losses per stream for every engine.
  single_rate_16k / single_rate_48k   like for like: every stream at that rate.  MixedBatchLyraDecoder ("mixed") against ONE
                BatchLyraDecoder ("batch") and ONE DeviceLyraDecoder ("device", pipelined, requests of one hop) at that rate --
                the guard against the per-stream path costing the uniform user something.
  mixed         a quarter of the streams at each rate: one MixedBatchLyraDecoder against four BatchLyraDecoder objects of
                streams / 4, each with its own context, driven round robin in one process (GPU_MAX_HW_QUEUES as the machine
                sets it).  The four objects are then timed once more in a process of their own ("batch_alone"), without the
                mixed engine's context beside them.  Several contexts in one process are known to run anomalously slowly
                (profiles/mixed_encoders.jsonl, cause not profiled): that figure is reported as such, not as a gain.
Per engine: the median of the windows with min..max, in frames (stream-hops) per second; whether two spreads overlap is
stated, nothing is judged against a threshold.  Every line is appended to --out."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RATES = (8000, 16000, 32000, 48000)


def table(kind, n):
    return [RATES[s % 4] for s in range(n)] if kind == "mixed" else [kind] * n


def run(demo, model_dir, rates, hops, windows, engines):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rates.txt")
        with open(path, "w") as f:
            f.write("".join(f"{r}\n" for r in rates))
        out = subprocess.run([demo, "--bench", model_dir, path, str(hops), str(windows), engines], check=True,
                             capture_output=True, text=True).stdout
    return [json.loads(line) for line in out.splitlines() if line.startswith("{")]


def spread(rows, engine, alone=False):
    v = sorted(r["frames_per_s"] for r in rows if r["engine"] == engine and bool(r.get("alone")) == alone)
    if not v:
        return None
    return {"median_Mfps": v[len(v) // 2] / 1e6, "min_Mfps": v[0] / 1e6, "max_Mfps": v[-1] / 1e6, "windows": len(v)}


def summary(name, rows, engines):
    rec = {"comparison": name}
    for engine in engines:
        rec[engine] = spread(rows, engine)
    a = rec["mixed"]
    for engine in engines[1:]:
        b = rec[engine]
        rec[f"spreads_overlap_mixed_{engine}"] = a["min_Mfps"] <= b["max_Mfps"] and b["min_Mfps"] <= a["max_Mfps"]
        rec[f"median_ratio_mixed_to_{engine}"] = a["median_Mfps"] / b["median_Mfps"]
    alone = spread(rows, "batch", alone=True)
    if alone:
        rec["batch_alone"] = alone
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--hops", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "mixed_decoder_demo")
    model_dir = lyra_amd.default_model_dir()
    lines = []
    for name, kind, engines in (("single_rate_16k", 16000, ("mixed", "batch", "device")),
                                ("single_rate_48k", 48000, ("mixed", "batch", "device")),
                                ("mixed", "mixed", ("mixed", "batch"))):
        hops = args.hops   # (the same window length in every comparison)
        rows = run(demo, model_dir, table(kind, args.streams), hops, args.windows, ",".join(engines))
        if name == "mixed":
            rows += [dict(r, alone=True) for r in run(demo, model_dir, table(kind, args.streams), hops, args.windows, "batch")]
        for r in rows:
            r["comparison"] = name
        rows.append(summary(name, rows, engines))
        for r in rows:
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
        if args.out:   # (appended comparison by comparison: a run that is cut short keeps what it measured)
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
            lines = []


if __name__ == "__main__":
    main()
