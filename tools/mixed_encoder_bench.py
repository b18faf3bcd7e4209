#!/usr/bin/env python3
"""Time MixedBatchLyraEncoder against what the classes before it offer, through lyra_amd/mixed_encoder_demo --bench.
   python tools/mixed_encoder_bench.py [--out profiles/mixed_encoders.jsonl] [--streams 4096] [--hops 1000] [--windows 5]
Two comparisons, each in ONE run of the demo with the two engines' windows alternating, two hops deep, host buffers in and
packets out, the same per-stream audio for both engines:
  mixed         an eighth of the streams in each (sample rate, DTX) class, a third at each bitrate:
                one MixedBatchLyraEncoder ("mixed") against one BatchLyraEncoder per class ("classes": eight objects of
                streams / 8, each with its own context, driven round robin in one process; GPU_MAX_HW_QUEUES as the machine
                sets it).  A BatchLyraEncoder has one bitrate: the eight objects run at 6000 bps, the middle one.
                The eight objects are then timed once more in a process of their own ("classes_alone", after the
                alternated run), without the mixed engine's context beside them.
  single-class  every stream with the same settings: MixedBatchLyraEncoder against ONE BatchLyraEncoder at those settings --
                the guard against the per-stream path costing the uniform user something.
Per engine: the median of the windows with min..max, in frames (stream-hops) per second; whether the two spreads overlap is
stated, nothing is judged against a threshold.  Every line is appended to --out."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RATES = (8000, 16000, 32000, 48000)
BITRATES = (6000, 9200, 3200)   # (stream 0 of every class at 6000: what the "classes" engine runs its objects at)


def table(kind, n):
    if kind == "mixed":
        return [(RATES[(s % 8) // 2], BITRATES[(s // 8) % 3], s & 1) for s in range(n)]
    rate, bitrate, dtx = kind
    return [(rate, bitrate, dtx)] * n


def run(demo, model_dir, params, hops, windows, only=None):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "params.txt")
        with open(path, "w") as f:
            f.write("".join(f"{r} {b} {x}\n" for r, b, x in params))
        out = subprocess.run([demo, "--bench", model_dir, path, str(hops), str(windows)] + ([only] if only else []), check=True, capture_output=True,
                             text=True).stdout
    return [json.loads(line) for line in out.splitlines() if line.startswith("{")]


def summary(name, rows):
    rec = {"comparison": name}
    for engine in ("mixed", "classes"):
        v = sorted(r["frames_per_s"] for r in rows if r["engine"] == engine and not r.get("alone"))
        rec[engine] = {"median_Mfps": v[len(v) // 2] / 1e6, "min_Mfps": v[0] / 1e6, "max_Mfps": v[-1] / 1e6, "windows": len(v)}
    a, b = rec["mixed"], rec["classes"]
    rec["spreads_overlap"] = a["min_Mfps"] <= b["max_Mfps"] and b["min_Mfps"] <= a["max_Mfps"]
    rec["median_ratio_mixed_to_classes"] = a["median_Mfps"] / b["median_Mfps"]
    v = sorted(r["frames_per_s"] for r in rows if r.get("alone"))
    if v:
        rec["classes_alone"] = {"median_Mfps": v[len(v) // 2] / 1e6, "min_Mfps": v[0] / 1e6, "max_Mfps": v[-1] / 1e6, "windows": len(v)}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--hops", type=int, default=1000)
    ap.add_argument("--hops-mixed", type=int, default=400, help="hops per window of the `mixed` comparison")
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "mixed_encoder_demo")
    lines = []
    for name, kind in (("mixed", "mixed"), ("single_class_16k_9200", (16000, 9200, 0)),
                       ("single_class_48k_6000_dtx", (48000, 6000, 1))):
        hops = args.hops_mixed if name == "mixed" else args.hops
        rows = run(demo, lyra_amd.default_model_dir(), table(kind, args.streams), hops, args.windows)
        if name == "mixed":
            alone = run(demo, lyra_amd.default_model_dir(), table(kind, args.streams), hops, args.windows, "classes")
            rows += [dict(r, alone=True) for r in alone]
        for r in rows:
            r["comparison"] = name
        rows.append(summary(name, rows))
        for r in rows:
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
