"""Throughput of lyra_hip_decode_samples_streams_dev (DecodeSamples(n) with a sample rate and a request size per stream in one
device call): JSON lines appended to --out.  4096 streams, a packet per stream and hop under Gilbert loss at 10 %.
  "mixed": a quarter of the streams at each of 8 / 16 / 32 / 48 kHz under callbacks of 160 / 256 / 441 / 1024 frames.  Per hop
           the classes whose next callback fits into the playout time make a round of callbacks, until none is due.
           (a) "one_call":  one lyra_hip_decode_samples_streams_dev call per round for ALL streams (rows that are not due ask for 0
               samples and only hand their packet over);
           (b) "per_class": the same work as one lyra_hip_decode_samples_any_dev call per (rate, size) class that is due, on a
               batch of a quarter of the streams, plus a 0-sample call for a class that has packets and no callback in the hop.
           The two ALTERNATE window by window on contexts of their own.
  "uniform": (c) like for like: every stream at 48 kHz / 480 frames, a packet every second call, through the new call (dense
           offsets, max_hops 1) and through lyra_hip_decode_samples_any_dev, alternating; the ratio new / uniform is reported.
Every shape is warmed up first; `reps` windows per form, median and min..max as decoded hops (20 ms of one stream) per second.
    python tools/decode_samples_streams_bench.py [--streams 4096] [--hops 100] [--reps 5] [--out profiles/decode_samples_streams.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

RATES, CALLBACKS = (8000, 16000, 32000, 48000), (160, 256, 441, 1024)


def rounds(n, rate):
    return (-(-n * 16000 // rate) + 319) // 320


def schedule(hops):
    """-> [(hop, first round of the hop, due[4])]: the rounds of callbacks of the session; a hop without a callback still has
    one round (nobody due) in which the packets are handed over"""
    played, out = [0] * 4, []
    for t in range(hops):
        first = True
        while True:
            due = tuple(played[c] + CALLBACKS[c] <= (t + 1) * (RATES[c] // 50) for c in range(4))
            if not any(due) and not first:
                break
            out.append((t, first, due))
            for c in range(4):
                played[c] += CALLBACKS[c] if due[c] else 0
            first = False
            if not any(due):
                break
    return out


def stats(B, hops, ts):
    f = sorted(B * hops / t for t in ts)
    return {"frames_per_s_median": round(f[len(f) // 2]), "min": round(f[0]), "max": round(f[-1])}


def timed(windows, reps):
    """windows: name -> (callable, context); alternated, rep 0 warms every shape up and is not counted"""
    times = {k: [] for k in windows}
    for rep in range(reps + 1):
        for name, (run, ctx) in windows.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            run()
            ctx.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    return times


def main():
    import torch
    import lyra_amd
    from lossy_steps_bench import gilbert
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--hops", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_samples_streams.jsonl"))
    a = ap.parse_args()
    B, dev = a.streams - a.streams % 4, torch.device("cuda", 0)
    Q = B // 4
    rng = np.random.default_rng(3)
    ring, loss = 16, 0.10    # distinct packet sets; the packets are random codes (the decoder's work does not depend on them)
    pk = rng.integers(0, 256, (ring, B, 23), dtype=np.uint8)
    size = np.array([8, 15, 23], np.int32)[np.arange(B) % 3]
    rx = gilbert(rng, a.hops, B, loss)
    nb = rx.astype(np.int32) * size                       # [hops][B]
    cls = np.arange(B) % 4                                # stream b decodes at RATES[b % 4]
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_ids, d_none = torch.arange(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    d_pk, d_nb = t_(pk), t_(nb)
    d_rates = t_(np.array(RATES, np.int32)[cls])
    sched = schedule(a.hops)
    lines = []
    # ---- (a) against (b) -------------------------------------------------------------------------------------------------
    one, per = lyra_amd.LyraHip(device=0, max_streams=B), lyra_amd.LyraHip(device=0, max_streams=B)
    try:
        shape = {}    # due pattern -> (sizes, offsets, max_hops, samples) of the one call
        for due in {d for _, _, d in sched}:
            n = np.where(np.array(due)[cls], np.array(CALLBACKS, np.int32)[cls], 0).astype(np.int32)
            offs = np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int32)
            shape[due] = (t_(n), t_(offs), max([1] + [rounds(CALLBACKS[c], RATES[c]) for c in range(4) if due[c]]), int(n.sum()))
        out = [torch.zeros(max(1, max(s[3] for s in shape.values())), dtype=torch.int16, device=dev) for _ in range(2)]
        c_ids = [t_(np.flatnonzero(cls == c).astype(np.int32)) for c in range(4)]
        c_pk = [t_(pk[:, cls == c]) for c in range(4)]
        c_nb = [t_(nb[:, cls == c]) for c in range(4)]
        c_none = torch.zeros(Q, dtype=torch.int32, device=dev)
        c_out = [[torch.zeros((Q, CALLBACKS[c]), dtype=torch.int16, device=dev) for _ in range(2)] for c in range(4)]

        def one_call():
            for k, (t, first, due) in enumerate(sched):
                n, offs, hops, total = shape[due]
                one.decode_samples_streams_dev(d_ids, d_pk[t % ring], d_nb[t] if first else d_none, d_rates, n, hops, out[k & 1],
                                               offs, n_pcm_samples=total)

        def per_class():
            for k, (t, first, due) in enumerate(sched):
                for c in range(4):
                    if due[c]:
                        per.decode_samples_any_dev(c_ids[c], c_pk[c][t % ring], c_nb[c][t] if first else c_none, CALLBACKS[c],
                                                   RATES[c], c_out[c][k & 1])
                    elif first:
                        per.decode_samples_any_dev(c_ids[c], c_pk[c][t % ring], c_nb[c][t], 0, RATES[c], None)

        times = timed({"one_call": (one_call, one), "per_class": (per_class, per)}, a.reps)
        line = {"bench": "decode_samples_streams", "case": "mixed", "streams": B, "rates": list(RATES), "callbacks": list(CALLBACKS),
                "loss": loss, "hops": a.hops, "reps": a.reps, "rounds_of_callbacks": len(sched),
                "uniform_calls_per_session": sum(sum(d) + (first and sum(not x for x in d)) for _, first, d in sched)}
        for name, ts in times.items():
            line[name] = stats(B, a.hops, ts)
        line["one_call_over_per_class"] = round(line["one_call"]["frames_per_s_median"] / line["per_class"]["frames_per_s_median"], 3)
        line["errors"] = {"one_call": int(one.decode_samples_errors()), "per_class": int(per.decode_samples_errors()),
                          "rates": int(one.rates_errors())}
        print(json.dumps(line), flush=True)
        lines.append(line)
    finally:
        one.close()
        per.close()
    # ---- (c) like for like -----------------------------------------------------------------------------------------------
    new, old = lyra_amd.LyraHip(device=0, max_streams=B), lyra_amd.LyraHip(device=0, max_streams=B)
    try:
        rate, n = 48000, 480
        out = [torch.zeros((B, n), dtype=torch.int16, device=dev) for _ in range(2)]
        r48 = torch.full((B,), rate, dtype=torch.int32, device=dev)
        n48 = torch.full((B,), n, dtype=torch.int32, device=dev)
        dense = t_((np.arange(B) * n).astype(np.int32))

        def streams_call():
            for t in range(a.hops):
                new.decode_samples_streams_dev(d_ids, d_pk[t % ring], d_nb[t], r48, n48, 1, out[0], dense)
                new.decode_samples_streams_dev(d_ids, d_pk[t % ring], d_none, r48, n48, 1, out[1], dense)

        def uniform_call():
            for t in range(a.hops):
                old.decode_samples_any_dev(d_ids, d_pk[t % ring], d_nb[t], n, rate, out[0])
                old.decode_samples_any_dev(d_ids, d_pk[t % ring], d_none, n, rate, out[1])

        times = timed({"streams_call": (streams_call, new), "uniform_call": (uniform_call, old)}, a.reps)
        line = {"bench": "decode_samples_streams", "case": "uniform", "streams": B, "rate": rate, "frames": n, "loss": loss,
                "hops": a.hops, "reps": a.reps}
        for name, ts in times.items():
            line[name] = stats(B, a.hops, ts)
        line["streams_over_uniform"] = round(line["streams_call"]["frames_per_s_median"] / line["uniform_call"]["frames_per_s_median"], 3)
        line["errors"] = int(new.decode_samples_errors()) + int(old.decode_samples_errors()) + int(new.rates_errors())
        print(json.dumps(line), flush=True)
        lines.append(line)
    finally:
        new.close()
        old.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
