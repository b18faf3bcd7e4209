"""Throughput of the conference bridge (include/lyra_hip_bridge.h): JSON lines appended to --out.  4096 participants, a packet per
participant and tick (speech encoded at 6 kb/s) under Gilbert loss at 10 %, outgoing 6 kb/s with DTX on every other stream.
  (a) "tick_dev":   one lyra_hip_bridge_tick_dev per tick, as a C caller issues it (without the binding's stream brackets:
                    torch_order = False) -- with rooms of 4, rooms of 16 and ONE room of all participants (one wavefront sums
                    4096 rows: the kernel's worst case);
  (b) "python_mix": what a Python caller could do before: decode_lossy_mixed_dev, torch index_add_ / gather / clamp on the caller's
                    stream (bracketed by lyra_hip_stream_wait / lyra_hip_wait_for_stream, which the binding does around every
                    `_dev` call), encode_streams_dev;
  (c) "begin_end":  lyra_hip_bridge_begin / _end two deep from host arrays, against "host_three_calls": the blocking host path --
                    decode_streams_begin / _end, a numpy mix, encode_streams_begin / _end;
  (d) "run_steps":  the ceiling: the same batch through lyra_hip_run_steps_dev with independent encode (DTX) and lossy decode legs
                    and no mix.
Forms of one comparison ALTERNATE window by window on contexts of their own; every shape is warmed up first; `reps` windows per
form, median and min..max in ticks x streams per second.  (a) and (c) are verified against (b) on a prefix of ticks: outgoing
packets and sizes bit for bit ((d) computes something else and is not).  "mix_kernel_us": the mix alone, device events around
back-to-back lyra_hip_bridge_mix_dev calls (memset + kernel), per layout.
--max-speakers N runs the loudest-N leg INSTEAD (include/lyra_hip_speakers.h), per layout, three forms alternating in one run:
  "speakers_tick_dev": one lyra_hip_speakers_tick_dev per tick (torch_order = False, as (a));
  "tick_dev":          (a), the full mix, on the same packets;
  "python_select":     the same selection in torch between the two existing calls: levels, topk per room over the keys
                       (level << 15 | 32767 - position, so that ties fall as the kernel's), index_add_, gather, clamp.
speakers_tick_dev is verified against python_select on the prefix, packets and sizes bit for bit.  "select_kernels_us": the
three kernels alone around back-to-back lyra_hip_speakers_mix_dev calls; "empty_share": the share of empty outgoing packets
(what DTX did not have to send) over one further pass of --hops ticks, of all streams and of the streams with DTX on.
--max-speakers N --shared runs the shared-encoder leg INSTEAD (include/lyra_hip_shared_bridge.h), per layout, two forms
alternating in one run on the same packets:
  "shared_tick_dev":   one lyra_hip_shared_tick_dev per tick: E = rooms x (1 + N) encoder rows (120 bits, DTX on every other
                       row, encoder ids 0 .. E - 1), the slot table on the device, the fan-out;
  "speakers_tick_dev": the loudest-N tick, one encoder chain per participant.
On the prefix shared_tick_dev is held to the loudest-N tick's levels and speaker flags (the same selection), to "a speaker
holds one slot, nobody else does", and to a numpy fan-out of its own encoder packets, bit for bit.  "shared_kernels_us": levels,
selection, slot update and the E mixes around back-to-back lyra_hip_shared_mix_dev calls; "distinct_packets_per_tick": how many
different non-empty packets a tick sends, against the streams it sends them to.  --layout L runs one layout only: give this
leg a process per layout -- with all three in one process the later layouts measured about 40 % slower in both forms (DESIGN.md
4.4, "Shared encoders"; cause not found).
--recording runs the recorded-meeting leg INSTEAD (include/lyra_hip_bridge_spans.h): meetings of 8 participants in one room, 10 %
Gilbert loss, DTX on every other row, of 9,000 ticks (3 minutes) and 180,000 ticks (1 hour), on 4,096 lanes:
  "spans_dev": ONE lyra_hip_spans_bridge_dev call for the whole meeting, median of --reps with min..max (streams reset in front of
               every call, outside the timed window), in seconds and as a multiple of real time;
  "tick_dev":  the same ticks through lyra_hip_bridge_tick_dev (lyra_hip_speakers_tick_dev with --max-speakers N), 8 rows each,
               torch_order = False.  The 3-minute meeting runs whole; of the hour the first 2,000 ticks are timed and the time
               SCALED to 180,000 ("scaled_from_ticks" says so).
"equal": outgoing packets and sizes of both forms bit for bit over the ticks the tick form ran.  "pass": the mix pass alone
(lyra_hip_spans_bridge_mix_dev on the meeting's decoded hops), device events around it on the encode-side stream, and its share
of the call.  No threshold is fixed in advance: "verdict" says faster, SLOWER or inside the spreads as the other legs do.
--recording --churn TICKS runs the meeting WITH A SCHEDULE instead (include/lyra_hip_spans_meeting.h): 3 minutes (9,000 ticks) of
32 participants in 4 rooms on 4,096 lanes, 10 % Gilbert loss, DTX on every other row, and on average one membership event in
TICKS ticks (a participant leaves, comes back or moves rooms).  In one process, alternating, median of --reps with min..max:
  "meeting_dev":           ONE lyra_hip_spans_meeting_dev call;
  "cut_spans_bridge_dev":  the same meeting as consecutive lyra_hip_spans_bridge_dev calls cut at every event, the method without
                           a schedule -- where absent participants are rows in no room, decoded and encoded on every tick,
                           because that is all that call can express;
  "tick_dev_present_rows": the tick form with the present participants as rows.
The first and the last must give the same outgoing packets and sizes bit for bit: asserted.  "pass": the schedule-driven mix pass
alone, device events around it; "epochs" / "entries": the planner's counts.  A second line, "meeting_constant", is the
like-for-like row: nobody comes or goes, the meeting call against one lyra_hip_spans_bridge_dev call in the same run.
    python tools/bridge_bench.py [--streams 4096] [--hops 200] [--reps 5] [--max-speakers N [--shared] [--layout L]]
                                 [--recording [--max-speakers N] [--lanes 4096] [--churn TICKS]] [--out profiles/bridge.jsonl]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def stats(B, hops, ts):
    f = sorted(B * hops / t for t in ts)
    return {"ticks_x_streams_per_s_median": round(f[len(f) // 2]), "min": round(f[0]), "max": round(f[-1])}


def timed(windows, reps):
    """windows: name -> (callable, context); alternated, rep 0 warms every shape up and is not counted"""
    import torch
    times = {k: [] for k in windows}
    for rep in range(reps + 1):
        for name, (run, ctx) in windows.items():
            ctx.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            ctx.synchronize()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    return times


def np_mix(x, room_of, first_rows):
    """the mix-minus where every room's rows lie together (first_rows: each room's first row; everybody a source), vectorised"""
    x = x.astype(np.int32)
    s = np.add.reduceat(x, first_rows, axis=0)
    return np.clip(s[room_of] - x, -32768, 32767).astype(np.int16)


def recording(a):
    """the --recording leg (see the module's docstring)"""
    import torch
    import lyra_amd
    from lossy_steps_bench import gilbert, speech_ring
    P, ring, N, dev = 8, 50, a.max_speakers, torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    ids = np.arange(P, dtype=np.int32)
    lanes = np.arange(P, P + a.lanes, dtype=np.int32)
    rooms = np.zeros(P, np.int32)
    dtx = (np.arange(P) % 2).astype(np.int32)
    d_ids, d_dtx = t_(ids), t_(dtx)
    speech = speech_ring(ring, P, rng)
    prep = lyra_amd.LyraHip(device=0, max_streams=P)
    pk = np.zeros((ring, P, 23), np.uint8)
    d15 = torch.zeros((P, 15), dtype=torch.uint8, device=dev)
    for t in range(ring):
        prep.encode_dev(d_ids, t_(speech[t]), 120, d15)
        prep.synchronize()
        pk[t, :, :15] = d15.cpu().numpy()
    prep.close()
    order, start = lyra_amd.codec.bridge_plan(rooms)
    d_order, d_start = t_(order), t_(start)
    lines = []
    for T, tick_ticks in ((9000, 9000), (180000, 2000)):
        rx = gilbert(rng, T, P, 0.10)
        nb = rx.astype(np.int32) * 15                                   # [T][P]
        F = P * T
        spans = [(int(p), int(p) * T, T) for p in ids]                  # participant-major: frame p * T + t
        pk_frames = np.ascontiguousarray(pk[np.arange(T) % ring].transpose(1, 0, 2)).reshape(F, 23)
        nb_frames = np.ascontiguousarray(nb.T).reshape(F)
        bits_frames = np.full(F, 120, np.int32)
        d_pkf = t_(pk_frames)
        cs, ct = (lyra_amd.LyraHip(device=0, max_streams=P + a.lanes) for _ in range(2))
        try:
            cs.torch_order = ct.torch_order = False
            out_s = torch.zeros((F, 23), dtype=torch.uint8, device=dev)
            len_s = torch.zeros(F, dtype=torch.int32, device=dev)
            x_s, mix_s = (torch.zeros((F, 320), dtype=torch.int16, device=dev) for _ in range(2))
            out_t = torch.zeros((tick_ticks, P, 23), dtype=torch.uint8, device=dev)
            len_t = torch.zeros((tick_ticks, P), dtype=torch.int32, device=dev)
            d_pk_ring, d_nb, d_bits = t_(pk), t_(nb[:tick_ticks]), t_(np.full(P, 120, np.int32))
            torch.cuda.synchronize()

            def one_call():
                cs.bridge_spans_dev(spans, rooms, d_pkf, nb_frames, bits_frames, out_s, len_s, x_s, mix_s, lane_ids=lanes, dtx=dtx,
                                    max_speakers=N)

            def ticks(n):
                for t in range(n):
                    if N:
                        ct.speakers_tick_dev(d_ids, d_pk_ring[t % ring], d_nb[t], d_order, d_start, d_bits, out_t[t], len_t[t], N,
                                             None, d_dtx)
                    else:
                        ct.bridge_tick_dev(d_ids, d_pk_ring[t % ring], d_nb[t], d_order, d_start, d_bits, out_t[t], len_t[t],
                                           None, d_dtx)

            def clocked(ctx, run):
                ctx.reset()
                ctx.synchronize()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                ctx.synchronize()
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            ticks(200)                                                   # warm-up of both forms, not counted
            clocked(cs, one_call)
            span_s = sorted(clocked(cs, one_call) for _ in range(a.reps))
            out_t.zero_()
            tick_s = clocked(ct, lambda: ticks(tick_ticks))
            # outgoing packets and sizes, bit for bit, over the ticks the tick form ran (both buffers started as zeros)
            got_len = len_s.view(P, T)[:, :tick_ticks].t()
            got_pk = out_s.view(P, T, 23)[:, :tick_ticks].transpose(0, 1)
            equal = bool(torch.equal(got_len, len_t) and torch.equal(got_pk, out_t))
            # the pass alone: events on the encode-side stream around it
            how = "device events around one lyra_hip_spans_bridge_mix_dev call"
            try:
                st = torch.cuda.ExternalStream(cs.stream_handle(), device=dev)
            except Exception:
                st, how = None, "host clock around one lyra_hip_spans_bridge_mix_dev call and a synchronise"
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            per = []
            for rep in range(a.reps + 1):
                cs.synchronize()
                t0 = time.perf_counter()
                if st is not None:
                    e0.record(st)
                cs.bridge_spans_mix_dev(spans, rooms, x_s, mix_s, N)
                if st is not None:
                    e1.record(st)
                cs.synchronize()
                if rep:
                    per.append(e0.elapsed_time(e1) if st is not None else (time.perf_counter() - t0) * 1e3)
            per.sort()
            med = span_s[len(span_s) // 2]
            tick_whole = tick_s * T / tick_ticks
            line = {"bench": "bridge", "case": "recording", "participants": P, "ticks": T, "minutes": T / 3000.0, "lanes": int(a.lanes),
                    "max_speakers": N, "loss": 0.10, "reps": a.reps,
                    "spans_dev": {"seconds_median": round(med, 4), "min": round(span_s[0], 4), "max": round(span_s[-1], 4),
                                  "times_real_time": round(T * 0.02 / med, 1)},
                    "tick_dev": {"seconds": round(tick_whole, 3), "timed_ticks": tick_ticks,
                                 "scaled_from_ticks": tick_ticks if tick_ticks != T else None,
                                 "times_real_time": round(T * 0.02 / tick_whole, 1)},
                    "tick_dev_over_spans_dev": round(tick_whole / med, 2),
                    "verdict": "faster" if span_s[-1] < tick_whole else "SLOWER" if span_s[0] > tick_whole else "inside the spreads",
                    "equal": equal, "equal_over_ticks": tick_ticks,
                    "pass": {"ms_median": round(per[len(per) // 2], 3), "min": round(per[0], 3), "max": round(per[-1], 3),
                             "share_of_call": round(per[len(per) // 2] / (med * 1e3), 4), "what": how},
                    "errors": {"bridge": int(cs.bridge_errors()), "lossy": int(cs.decode_lossy_errors()),
                               "mixed": int(cs.encode_mixed_errors())}}
            print(json.dumps(line), flush=True)
            lines.append(line)
        finally:
            cs.close()
            ct.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


def draw_churn(rng, P, T, n_rooms, every):
    """a meeting of T ticks whose membership changes on average once in `every` ticks (0: never): a drawn participant leaves,
    comes back (where it is away) or moves to another room -> (present bool [T][P], room int32 [T][P], events)"""
    present, room = np.ones((T, P), bool), np.tile((np.arange(P) % n_rooms).astype(np.int32), (T, 1))
    at = np.sort(rng.choice(np.arange(1, T), T // every, replace=False)) if every else []
    for t in at:
        p = int(rng.integers(0, P))
        if not present[t, p]:
            present[t:, p] = True
        elif rng.random() < 0.5:
            present[t:, p] = False
        else:
            room[t:, p] = (room[t, p] + 1 + rng.integers(0, n_rooms - 1)) % n_rooms
    return present, room, len(at)


def stays_of(present, room):
    """(present, room) tables -> (stays sorted by (participant, first_tick), present ticks per participant)"""
    T, P = present.shape
    stays = []
    for p in range(P):
        key = np.where(present[:, p], room[:, p], -2)
        cuts = np.flatnonzero(np.diff(key)) + 1
        for lo, hi in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [T]])):
            if key[lo] != -2:
                stays.append((p, int(key[lo]), int(lo), int(hi - lo)))
    return stays, present.sum(axis=0)


def churn(a):
    """the --recording --churn leg (see the module's docstring)"""
    import torch
    import lyra_amd
    from lossy_steps_bench import gilbert, speech_ring
    P, T, n_rooms, ring, N, dev = 32, 9000, 4, 50, a.max_speakers, torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    ids = np.arange(P, dtype=np.int32)
    lanes = np.arange(P, P + a.lanes, dtype=np.int32)
    dtx = (np.arange(P) % 2).astype(np.int32)
    speech = speech_ring(ring, P, rng)
    prep = lyra_amd.LyraHip(device=0, max_streams=P)
    pk = np.zeros((ring, P, 23), np.uint8)
    d15 = torch.zeros((P, 15), dtype=torch.uint8, device=dev)
    for t in range(ring):
        prep.encode_dev(t_(ids), t_(speech[t]), 120, d15)
        prep.synchronize()
        pk[t, :, :15] = d15.cpu().numpy()
    prep.close()
    nb = gilbert(rng, T, P, 0.10).astype(np.int32) * 15              # [T][P] by meeting tick
    pk_all = pk[np.arange(T) % ring]                                 # [T][P][23]
    lines = []
    for every in (a.churn, 0):                                       # the churny meeting, then the like-for-like row
        present, room, n_events = draw_churn(rng, P, T, n_rooms, every)
        stays, n_present = stays_of(present, room)
        first = np.concatenate([[0], np.cumsum(n_present)[:-1]]).astype(np.int64)
        spans = [(int(p), int(first[p]), int(n_present[p])) for p in range(P)]
        F = int(n_present.sum())
        frame_of = np.full((T, P), -1, np.int64)                     # the meeting call's frame of (tick, participant)
        for p in range(P):
            frame_of[present[:, p], p] = first[p] + np.arange(n_present[p])
        here = frame_of >= 0
        pk_f, nb_f = np.zeros((F, 23), np.uint8), np.zeros(F, np.int32)
        pk_f[frame_of[here]], nb_f[frame_of[here]] = pk_all[here], nb[here]
        bits_f = np.full(F, 120, np.int32)
        plan = lyra_amd.codec.meeting_plan(spans, stays)
        # (b) the parent's method: everybody a row of every tick (absent: in no room), one call per stretch between events
        key = np.where(present, room, -1)
        cuts = [0] + [t for t in range(1, T) if (key[t] != key[t - 1]).any()] + [T]
        Fb = P * T
        spans_b = [(int(p), int(p) * T, T) for p in range(P)]
        pk_b = np.ascontiguousarray(pk_all.transpose(1, 0, 2)).reshape(Fb, 23)
        nb_b, bits_b = np.ascontiguousarray(nb.T).reshape(Fb), np.full(Fb, 120, np.int32)
        # (c) the ticks with the present rows only: per stretch of constant membership the rows, their index and their inputs
        stretches = []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            rows = np.flatnonzero(present[lo])
            if not rows.size:
                continue
            order, start = lyra_amd.codec.bridge_plan(room[lo, rows])
            stretches.append(dict(lo=lo, n=hi - lo, rows=rows, ids=t_(ids[rows]), order=t_(order), start=t_(start), dtx=t_(dtx[rows]),
                                  bits=t_(np.full(rows.size, 120, np.int32)), pk=t_(pk_all[lo:hi][:, rows]), nb=t_(nb[lo:hi][:, rows]),
                                  out=torch.zeros((hi - lo, rows.size, 23), dtype=torch.uint8, device=dev),
                                  len=torch.zeros((hi - lo, rows.size), dtype=torch.int32, device=dev),
                                  frames=t_(frame_of[lo:hi][:, rows])))
        ca, cb, cc = (lyra_amd.LyraHip(device=0, max_streams=P + a.lanes) for _ in range(3))
        try:
            ca.torch_order = cb.torch_order = cc.torch_order = False
            out_a, len_a = torch.zeros((F, 23), dtype=torch.uint8, device=dev), torch.zeros(F, dtype=torch.int32, device=dev)
            x_a, mix_a = (torch.zeros((F, 320), dtype=torch.int16, device=dev) for _ in range(2))
            out_b, len_b = torch.zeros((Fb, 23), dtype=torch.uint8, device=dev), torch.zeros(Fb, dtype=torch.int32, device=dev)
            x_b, mix_b = (torch.zeros((Fb, 320), dtype=torch.int16, device=dev) for _ in range(2))
            d_pk_a, d_pk_b = t_(pk_f), t_(pk_b)
            torch.cuda.synchronize()

            def form_a():
                ca.meeting_spans_dev(spans, stays, d_pk_a, nb_f, bits_f, out_a, len_a, x_a, mix_a, lane_ids=lanes, dtx=dtx, max_speakers=N)

            def form_b(n=None):
                for lo, hi in list(zip(cuts[:-1], cuts[1:]))[:n]:
                    part = [(i, f0 + lo, hi - lo) for (i, f0, _) in spans_b]
                    cb.bridge_spans_dev(part, key[lo], d_pk_b, nb_b, bits_b, out_b, len_b, x_b, mix_b, lane_ids=lanes, dtx=dtx,
                                        max_speakers=N)

            def form_c(n=None):
                for s in stretches[:n]:
                    for t in range(s["n"]):
                        args = (s["ids"], s["pk"][t], s["nb"][t], s["order"], s["start"], s["bits"], s["out"][t], s["len"][t])
                        if N:
                            cc.speakers_tick_dev(*args, N, None, s["dtx"])
                        else:
                            cc.bridge_tick_dev(*args, None, s["dtx"])

            def clocked(ctx, run):
                ctx.reset()
                ctx.synchronize()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                ctx.synchronize()
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            clocked(ca, form_a)                                          # warm-up of the three forms, not counted
            clocked(cb, lambda: form_b(4))
            clocked(cc, lambda: form_c(2))
            times = {"a": [], "b": [], "c": []}
            for _ in range(a.reps):                                      # alternating, in one process
                times["a"].append(clocked(ca, form_a))
                times["b"].append(clocked(cb, form_b))
                if every:
                    times["c"].append(clocked(cc, form_c))
            if every:                                                    # (a) and (c): the same outgoing packets and sizes
                for s in stretches:
                    f = s["frames"].reshape(-1)
                    assert torch.equal(len_a[f], s["len"].reshape(-1)) and torch.equal(out_a[f], s["out"].reshape(-1, 23)), \
                        f"the meeting call and the ticks differ in the stretch from tick {s['lo']}"
            # (b) agrees with (a) where a participant is present and in the same company: not asserted, absent rows differ by design
            how = "device events around one lyra_hip_spans_meeting_mix_dev call"
            try:
                st = torch.cuda.ExternalStream(ca.stream_handle(), device=dev)
            except Exception:
                st, how = None, "host clock around one lyra_hip_spans_meeting_mix_dev call and a synchronise"
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            per = []
            for rep in range(a.reps + 1):
                ca.synchronize()
                t0 = time.perf_counter()
                if st is not None:
                    e0.record(st)
                ca.meeting_spans_mix_dev(spans, stays, x_a, mix_a, N)
                if st is not None:
                    e1.record(st)
                ca.synchronize()
                if rep:
                    per.append(e0.elapsed_time(e1) if st is not None else (time.perf_counter() - t0) * 1e3)
            per.sort()

            def summary(ts):
                ts = sorted(ts)
                return {"seconds_median": round(ts[len(ts) // 2], 4), "min": round(ts[0], 4), "max": round(ts[-1], 4),
                        "times_real_time": round(T * 0.02 / ts[len(ts) // 2], 1)}

            def verdict(x, y):
                return "faster" if max(x) < min(y) else "SLOWER" if min(x) > max(y) else "inside the spreads"

            line = {"bench": "bridge", "case": "meeting_churn" if every else "meeting_constant", "participants": P, "rooms": n_rooms,
                    "ticks": T, "lanes": int(a.lanes), "max_speakers": N, "loss": 0.10, "reps": a.reps, "churn_ticks": every,
                    "events": n_events, "epochs": int(len(plan["epoch_tick"]) - 1), "entries": int(len(plan["entry_participant"])),
                    "present_frames": F, "meeting_dev": summary(times["a"]),
                    "cut_spans_bridge_dev": dict(summary(times["b"]), calls=len(cuts) - 1, frames=Fb,
                                                 note="the parent's method: absent participants are rows in no room, decoded and "
                                                      "encoded on every tick" if every else "one call, constant membership"),
                    "meeting_dev_vs_cut_calls": verdict(times["a"], times["b"]),
                    "pass": {"ms_median": round(per[len(per) // 2], 3), "min": round(per[0], 3), "max": round(per[-1], 3), "what": how},
                    "errors": {"bridge": int(ca.bridge_errors()), "lossy": int(ca.decode_lossy_errors()),
                               "mixed": int(ca.encode_mixed_errors())}}
            if every:
                line["tick_dev_present_rows"] = summary(times["c"])
                line["meeting_dev_vs_ticks"] = verdict(times["a"], times["c"])
                line["equal"] = True
            print(json.dumps(line), flush=True)
            lines.append(line)
        finally:
            ca.close()
            cb.close()
            cc.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


def main():
    import torch
    import lyra_amd
    from lyra_amd import codec
    from lossy_steps_bench import gilbert, speech_ring
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--hops", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--verify", type=int, default=12, help="ticks of the prefix on which the forms are compared")
    ap.add_argument("--max-speakers", type=int, default=0, help="run the loudest-N leg with this N instead of the legs above")
    ap.add_argument("--shared", action="store_true", help="with --max-speakers: the shared-encoder tick against the loudest-N tick")
    ap.add_argument("--layout", default=None, choices=["rooms_of_4", "rooms_of_16", "one_room"],
                    help="with --max-speakers: this layout only (a process of its own per layout)")
    ap.add_argument("--recording", action="store_true", help="the recorded-meeting leg: one time-parallel call against the ticks")
    ap.add_argument("--lanes", type=int, default=4096, help="with --recording: stream slots lent to the call")
    ap.add_argument("--churn", type=int, default=0, help="with --recording: the meeting with a schedule, one membership event in "
                                                         "this many ticks on average")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bridge.jsonl"))
    a = ap.parse_args()
    if a.recording:
        if a.shared:
            raise SystemExit("--recording has no shared-encoder form")
        return churn(a) if a.churn else recording(a)
    B, dev, ring = a.streams, torch.device("cuda", 0), 50
    rng = np.random.default_rng(3)
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    d_ids = torch.arange(B, dtype=torch.int32, device=dev)
    ids = np.arange(B, dtype=np.int32)
    # ---- the incoming packets: `ring` hops of speech per participant, encoded once at 120 bits -----------------------------
    speech = speech_ring(ring, B, rng)
    prep = lyra_amd.LyraHip(device=0, max_streams=B)
    pk = np.zeros((ring, B, 23), np.uint8)
    d15 = torch.zeros((B, 15), dtype=torch.uint8, device=dev)
    for t in range(ring):
        prep.encode_dev(d_ids, t_(speech[t]), 120, d15)
        prep.synchronize()
        pk[t, :, :15] = d15.cpu().numpy()
    prep.close()
    rx = gilbert(rng, a.hops, B, 0.10)
    nb = (rx.astype(np.int32) * 15)
    bits = np.full(B, 120, np.int32)
    dtx = (np.arange(B) % 2).astype(np.int32)
    d_pk, d_nb, d_bits, d_dtx = t_(pk), t_(nb), t_(bits), t_(dtx)
    layouts = {"rooms_of_4": ids // 4, "rooms_of_16": ids // 16, "one_room": np.zeros(B, np.int32)}
    if a.layout and a.max_speakers:
        layouts = {a.layout: layouts[a.layout]}
    lines, ref_b = [], []   # ref_b: form (b)'s packets and sizes on the prefix, rooms of 4

    def new_bufs():
        return ([torch.zeros((B, 23), dtype=torch.uint8, device=dev) for _ in range(2)],
                [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2)],
                [torch.zeros((B, 320), dtype=torch.int16, device=dev) for _ in range(2)],
                [torch.zeros((B, 320), dtype=torch.int16, device=dev) for _ in range(2)])

    def append(lines):
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")

    # ---- the shared-encoder leg, per layout: E encoder rows against B -------------------------------------------------------
    if a.shared:
        if not a.max_speakers:
            raise SystemExit("--shared needs --max-speakers N")
        N = a.max_speakers
        for name, room_of in layouts.items():
            order, start = codec.bridge_plan(room_of)
            n_rooms = start.size - 1
            E = n_rooms * (1 + N)
            d_order, d_start = t_(order), t_(start)
            csh, cs = (lyra_amd.LyraHip(device=0, max_streams=max(B, E)) for _ in range(2))
            try:
                csh.torch_order = cs.torch_order = False
                out_h, len_h, x_h, _ = new_bufs()
                out_s, len_s, _, _ = new_bufs()
                table = torch.full((n_rooms, codec.SHARED_SLOTS), -1, dtype=torch.int32, device=dev)
                e_ids = torch.arange(E, dtype=torch.int32, device=dev)
                e_bits = torch.full((E,), 120, dtype=torch.int32, device=dev)
                e_dtx = (torch.arange(E, dtype=torch.int32, device=dev) % 2).contiguous()
                e_mix = torch.zeros((E, 320), dtype=torch.int16, device=dev)
                e_pk = torch.zeros((E, 23), dtype=torch.uint8, device=dev)
                e_len = torch.zeros(E, dtype=torch.int32, device=dev)
                lv_h, lv_s = (torch.zeros(B, dtype=torch.int64, device=dev) for _ in range(2))
                sp_h, sp_s, slot_h = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
                torch.cuda.synchronize()

                def tick_h(t, check=False):
                    extra = (lv_h, sp_h, None, e_pk, e_len, slot_h) if check else (None,) * 6
                    csh.shared_tick_dev(d_ids, d_pk[t % ring], d_nb[t], d_order, d_start, out_h[t & 1], len_h[t & 1], N, table,
                                        e_ids, e_bits, None, e_dtx, None, 0, x_h[0] if check else None, None, None, *extra)

                def tick_s(t, check=False):
                    cs.speakers_tick_dev(d_ids, d_pk[t % ring], d_nb[t], d_order, d_start, d_bits, out_s[t & 1], len_s[t & 1], N,
                                         None, d_dtx, 0, None, None, None, None, *((lv_s, sp_s) if check else (None, None)))

                verified = 0
                for t in range(min(a.verify, a.hops)):
                    tick_h(t, True)
                    tick_s(t, True)
                    csh.synchronize()
                    cs.synchronize()
                    torch.cuda.synchronize()
                    slot, spk = slot_h.cpu().numpy(), sp_h.cpu().numpy()
                    if not (torch.equal(lv_h, lv_s) and torch.equal(sp_h, sp_s) and np.array_equal(slot >= 0, spk == 1)):
                        raise SystemExit(f"{name}: shared_tick_dev and speakers_tick_dev select differently at tick {t}")
                    rows = room_of * (1 + N) + np.where(slot >= 0, 1 + slot, 0)
                    if not (np.array_equal(out_h[t & 1].cpu().numpy(), e_pk.cpu().numpy()[rows]) and
                            np.array_equal(len_h[t & 1].cpu().numpy(), e_len.cpu().numpy()[rows])):
                        raise SystemExit(f"{name}: the fan-out of shared_tick_dev differs from its encoder packets at tick {t}")
                    verified += 1
                csh.reset()
                cs.reset()
                table.fill_(-1)
                times = timed({"shared_tick_dev": (lambda: [tick_h(t) for t in range(a.hops)], csh),
                               "speakers_tick_dev": (lambda: [tick_s(t) for t in range(a.hops)], cs)}, a.reps)
                line = {"bench": "bridge", "case": "shared", "layout": name, "streams": B, "rooms": int(n_rooms),
                        "max_speakers": N, "encoder_rows": int(E), "loss": 0.10, "hops": a.hops, "reps": a.reps,
                        "verified_ticks": verified}
                for k, ts in times.items():
                    line[k] = stats(B, a.hops, ts)
                med = lambda k: line[k]["ticks_x_streams_per_s_median"]   # noqa: E731
                line["shared_over_speakers"] = round(med("shared_tick_dev") / med("speakers_tick_dev"), 3)
                sh, sp = line["shared_tick_dev"], line["speakers_tick_dev"]
                line["verdict"] = ("SLOWER" if sh["max"] < sp["min"] else "faster" if sh["min"] > sp["max"] else "inside the spreads")
                # levels, selection, slot update and the E mixes alone
                csh.synchronize()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                per, n, how = [], 100, "device events around 100 calls back to back (four kernels)"
                try:
                    st = torch.cuda.ExternalStream(csh.stream_handle(), device=dev)
                except Exception:
                    st, how = None, "host clock around 100 calls back to back and a synchronise (four kernels + launches)"
                for r in range(a.reps + 1):
                    t0 = time.perf_counter()
                    if st is not None:
                        e0.record(st)
                    for _ in range(n):
                        csh.shared_mix_dev(x_h[0], d_ids, d_order, d_start, table, e_mix, N)
                    if st is not None:
                        e1.record(st)
                    csh.synchronize()
                    if r:
                        per.append((e0.elapsed_time(e1) * 1000.0 if st is not None else (time.perf_counter() - t0) * 1e6) / n)
                per.sort()
                line["shared_kernels_us"] = {"median": round(per[len(per) // 2], 2), "min": round(per[0], 2),
                                             "max": round(per[-1], 2), "what": how}
                # how many different packets a tick sends: one further pass of a few ticks
                csh.reset()
                table.fill_(-1)
                distinct, sent = [], []
                for t in range(min(20, a.hops)):
                    tick_h(t)
                    csh.synchronize()
                    p, ln = out_h[t & 1].cpu().numpy(), len_h[t & 1].cpu().numpy()
                    distinct.append(int(np.unique(p[ln > 0], axis=0).shape[0]))
                    sent.append(int((ln > 0).sum()))
                line["distinct_packets_per_tick"] = {"median": int(np.median(distinct)), "sent_to_streams_median": int(np.median(sent))}
                line["errors"] = {"bridge": int(csh.bridge_errors()), "lossy": int(csh.decode_lossy_errors()),
                                  "mixed": int(csh.encode_mixed_errors())}
                print(json.dumps(line), flush=True)
                lines.append(line)
            finally:
                csh.close()
                cs.close()
        append(lines)
        return

    # ---- the loudest-N leg, per layout (rooms of one size M, a room's rows together) ----------------------------------------
    if a.max_speakers:
        N = a.max_speakers
        for name, room_of in layouts.items():
            order, start = codec.bridge_plan(room_of)
            n_rooms = start.size - 1
            M = B // n_rooms
            k_sel = min(N, M)
            d_order, d_start, d_room = t_(order), t_(start), t_(room_of.astype(np.int64))
            cs, ca, ct = (lyra_amd.LyraHip(device=0, max_streams=B) for _ in range(3))
            try:
                cs.torch_order = ca.torch_order = False
                out_s, len_s, _, _ = new_bufs()
                out_a, len_a, _, _ = new_bufs()
                out_t, len_t, x_t, mix_t = new_bufs()
                rates16 = torch.full((B,), 16000, dtype=torch.int32, device=dev)
                offs = torch.arange(B, dtype=torch.int32, device=dev) * 320
                sums = torch.zeros((n_rooms, 320), dtype=torch.int32, device=dev)
                pos_key = (32767 - torch.arange(M, dtype=torch.int64, device=dev))[None, :]
                room_base = (torch.arange(n_rooms, dtype=torch.int64, device=dev) * M)[:, None]
                room_sel = torch.arange(n_rooms, dtype=torch.int64, device=dev)[:, None].expand(n_rooms, k_sel).reshape(-1)
                torch.cuda.synchronize()

                def tick_s(t):
                    cs.speakers_tick_dev(d_ids, d_pk[t % ring], d_nb[t], d_order, d_start, d_bits, out_s[t & 1], len_s[t & 1], N,
                                         None, d_dtx)

                def tick_a(t):
                    ca.bridge_tick_dev(d_ids, d_pk[t % ring], d_nb[t], d_order, d_start, d_bits, out_a[t & 1], len_a[t & 1],
                                       None, d_dtx)

                def tick_t(t):
                    k = t & 1
                    ct.decode_lossy_mixed_dev(d_ids, d_pk[t % ring], d_nb[t], 16000, x_t[k])
                    x = x_t[k].to(torch.int32)
                    x64 = x.to(torch.int64)
                    levels = (x64 * x64).sum(dim=1)
                    keys = (levels.view(n_rooms, M) << 15) | pos_key            # unique per room: louder first, then earlier
                    vals, idx = torch.topk(keys, k_sel, dim=1)
                    valid = ((vals >> 15) > 0).reshape(-1)                      # a zero-level row is no candidate
                    rows = (idx + room_base).reshape(-1)
                    sums.zero_()
                    sums.index_add_(0, room_sel, x[rows] * valid[:, None].to(torch.int32))
                    is_spk = torch.zeros(B, dtype=torch.int32, device=dev)
                    is_spk[rows] = valid.to(torch.int32)
                    mix_t[k].copy_((sums[d_room] - x * is_spk[:, None]).clamp_(-32768, 32767))
                    ct.encode_streams_dev(d_ids, mix_t[k], rates16, d_bits, out_t[k], len_t[k], d_dtx, offs, 320 * B)

                verified = 0
                for t in range(min(a.verify, a.hops)):
                    tick_s(t)
                    tick_t(t)
                    cs.synchronize()
                    ct.synchronize()
                    torch.cuda.synchronize()
                    ls, lt = len_s[t & 1].cpu().numpy(), len_t[t & 1].cpu().numpy()
                    ps, pt = out_s[t & 1].cpu().numpy(), out_t[t & 1].cpu().numpy()
                    if not (np.array_equal(ls, lt) and all(np.array_equal(ps[b, :ls[b]], pt[b, :ls[b]]) for b in range(B))):
                        raise SystemExit(f"{name}: speakers_tick_dev and python_select differ at tick {t}")
                    verified += 1
                cs.reset()
                ct.reset()
                times = timed({"speakers_tick_dev": (lambda: [tick_s(t) for t in range(a.hops)], cs),
                               "tick_dev": (lambda: [tick_a(t) for t in range(a.hops)], ca),
                               "python_select": (lambda: [tick_t(t) for t in range(a.hops)], ct)}, a.reps)
                line = {"bench": "bridge", "case": "speakers", "layout": name, "streams": B, "rooms": int(n_rooms),
                        "max_speakers": N, "loss": 0.10, "hops": a.hops, "reps": a.reps, "verified_ticks": verified}
                for k, ts in times.items():
                    line[k] = stats(B, a.hops, ts)
                med = lambda k: line[k]["ticks_x_streams_per_s_median"]   # noqa: E731
                line["speakers_over_tick_dev"] = round(med("speakers_tick_dev") / med("tick_dev"), 3)
                line["speakers_over_python_select"] = round(med("speakers_tick_dev") / med("python_select"), 3)
                # the three kernels alone, as "mix_kernel_us" below
                cs.synchronize()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                per, n, how = [], 100, "device events around 100 calls back to back (three kernels)"
                try:
                    st = torch.cuda.ExternalStream(cs.stream_handle(), device=dev)
                except Exception:
                    st, how = None, "host clock around 100 calls back to back and a synchronise (three kernels + launches)"
                for rep in range(a.reps + 1):
                    t0 = time.perf_counter()
                    if st is not None:
                        e0.record(st)
                    for _ in range(n):
                        cs.speakers_mix_dev(x_t[0], d_order, d_start, mix_t[1], N)
                    if st is not None:
                        e1.record(st)
                    cs.synchronize()
                    if rep:
                        per.append((e0.elapsed_time(e1) * 1000.0 if st is not None else (time.perf_counter() - t0) * 1e6) / n)
                per.sort()
                line["select_kernels_us"] = {"median": round(per[len(per) // 2], 2), "min": round(per[0], 2),
                                             "max": round(per[-1], 2), "what": how}
                # what DTX did not send: one further pass per mix, the empty outgoing packets counted tick by tick
                share = {}
                for form, ctx, tick, lens in (("speakers_tick_dev", cs, tick_s, len_s), ("tick_dev", ca, tick_a, len_a)):
                    ctx.reset()
                    empty = np.zeros(B, np.int64)
                    for t in range(a.hops):
                        tick(t)
                        ctx.synchronize()
                        empty += lens[t & 1].cpu().numpy() == 0
                    share[form] = {"all_streams": round(float(empty.sum()) / (B * a.hops), 4),
                                   "dtx_streams": round(float(empty[dtx != 0].sum()) / (int((dtx != 0).sum()) * a.hops), 4)}
                line["empty_share"] = share
                line["errors"] = {"bridge": int(cs.bridge_errors()), "lossy": int(cs.decode_lossy_errors()),
                                  "mixed": int(cs.encode_mixed_errors())}
                print(json.dumps(line), flush=True)
                lines.append(line)
            finally:
                cs.close()
                ca.close()
                ct.close()
        append(lines)
        return

    # ---- (a) against (b), per layout ---------------------------------------------------------------------------------------
    for name, room_of in layouts.items():
        order, start = codec.bridge_plan(room_of)
        n_rooms = start.size - 1
        d_order, d_start, d_room = t_(order), t_(start), t_(room_of.astype(np.int64))
        ca, cb = lyra_amd.LyraHip(device=0, max_streams=B), lyra_amd.LyraHip(device=0, max_streams=B)
        try:
            # (a) has no torch work between its calls: it runs as a C caller would, without the binding's brackets around every
            # `_dev` call (which order each call behind the WHOLE call before it); its inputs are complete before the first tick
            ca.torch_order = False
            out_a, len_a, _, _ = new_bufs()
            out_b, len_b, x_b, mix_b = new_bufs()
            rates16 = torch.full((B,), 16000, dtype=torch.int32, device=dev)
            offs = torch.arange(B, dtype=torch.int32, device=dev) * 320
            sums = torch.zeros((n_rooms, 320), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def tick_a(t):
                ca.bridge_tick_dev(d_ids, d_pk[t % ring], d_nb[t], d_order, d_start, d_bits, out_a[t & 1], len_a[t & 1],
                                   None, d_dtx)

            def tick_b(t):
                k = t & 1
                cb.decode_lossy_mixed_dev(d_ids, d_pk[t % ring], d_nb[t], 16000, x_b[k])
                x = x_b[k].to(torch.int32)
                sums.zero_()
                sums.index_add_(0, d_room, x)
                mix_b[k].copy_((sums[d_room] - x).clamp_(-32768, 32767))
                cb.encode_streams_dev(d_ids, mix_b[k], rates16, d_bits, out_b[k], len_b[k], d_dtx, offs, 320 * B)

            verified = 0
            for t in range(min(a.verify, a.hops)):
                tick_a(t)
                tick_b(t)
                ca.synchronize()
                cb.synchronize()
                torch.cuda.synchronize()
                la, lb = len_a[t & 1].cpu().numpy(), len_b[t & 1].cpu().numpy()
                pa, pb = out_a[t & 1].cpu().numpy(), out_b[t & 1].cpu().numpy()
                same = np.array_equal(la, lb) and all(np.array_equal(pa[b, :la[b]], pb[b, :la[b]]) for b in range(B))
                if not same:
                    raise SystemExit(f"{name}: tick_dev and python_mix differ at tick {t}")
                verified += 1
                if name == "rooms_of_4":
                    ref_b.append((pb.copy(), lb.copy()))
            ca.reset()
            cb.reset()
            times = timed({"tick_dev": (lambda: [tick_a(t) for t in range(a.hops)], ca),
                           "python_mix": (lambda: [tick_b(t) for t in range(a.hops)], cb)}, a.reps)
            line = {"bench": "bridge", "case": "dev", "layout": name, "streams": B, "rooms": int(n_rooms), "loss": 0.10,
                    "hops": a.hops, "reps": a.reps, "verified_ticks": verified}
            for k, ts in times.items():
                line[k] = stats(B, a.hops, ts)
            line["tick_dev_over_python_mix"] = round(line["tick_dev"]["ticks_x_streams_per_s_median"] /
                                                     line["python_mix"]["ticks_x_streams_per_s_median"], 3)
            # the mix alone: events on the encode-side stream around back-to-back calls (no binding brackets)
            ca.synchronize()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            per, n, how = [], 100, "device events around 100 calls back to back (memset + kernel)"
            try:
                st = torch.cuda.ExternalStream(ca.stream_handle(), device=dev)
            except Exception:   # no way to put an event on the library's stream: the host clock around the same calls
                st, how = None, "host clock around 100 calls back to back and a synchronise (memset + kernel + launches)"
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                if st is not None:
                    e0.record(st)
                for _ in range(n):
                    ca.bridge_mix_dev(x_b[0], d_order, d_start, mix_b[1])
                if st is not None:
                    e1.record(st)
                ca.synchronize()
                if rep:
                    per.append((e0.elapsed_time(e1) * 1000.0 if st is not None else (time.perf_counter() - t0) * 1e6) / n)
            per.sort()
            line["mix_kernel_us"] = {"median": round(per[len(per) // 2], 2), "min": round(per[0], 2), "max": round(per[-1], 2), "what": how}
            line["errors"] = {"bridge": int(ca.bridge_errors()), "lossy": int(ca.decode_lossy_errors()),
                              "mixed": int(ca.encode_mixed_errors())}
            print(json.dumps(line), flush=True)
            lines.append(line)
        finally:
            ca.close()
            cb.close()

    # ---- (c) the host forms, rooms of 4 ------------------------------------------------------------------------------------
    room_of = layouts["rooms_of_4"]
    cc, ch = lyra_amd.LyraHip(device=0, max_streams=B), lyra_amd.LyraHip(device=0, max_streams=B)
    try:
        rates16 = np.full(B, 16000, np.int32)
        first_rows = np.flatnonzero(np.diff(room_of, prepend=-1))

        def host_three(t):
            ch.decode_streams_begin(pk[t % ring], nb[t], rates16)
            x, _, _ = ch.decode_streams_end()
            ch.encode_streams_begin(np_mix(x.reshape(B, 320), room_of, first_rows), rates16, bits, dtx)
            return ch.encode_streams_end()

        def begin_end(hops, keep=None):
            for t in range(hops):
                cc.bridge_begin(pk[t % ring], nb[t], room_of, bits, None, dtx)
                if t >= 1:
                    got = cc.bridge_end()
                    if keep is not None:
                        keep.append(got)
            got = cc.bridge_end()
            if keep is not None:
                keep.append(got)

        n_ver = min(a.verify, a.hops)
        got = []
        begin_end(n_ver, got)
        for t in range(n_ver):
            want, (pb, lb) = host_three(t), ref_b[t]
            for form, (p, n) in (("begin_end", got[t][:2]), ("host_three_calls", want)):
                if not (np.array_equal(n, lb) and all(np.array_equal(p[b, :lb[b]], pb[b, :lb[b]]) for b in range(B))):
                    raise SystemExit(f"{form} and python_mix differ at tick {t}")
        cc.reset()
        ch.reset()
        times = timed({"begin_end": (lambda: begin_end(a.hops), cc),
                       "host_three_calls": (lambda: [host_three(t) for t in range(a.hops)], ch)}, a.reps)
        line = {"bench": "bridge", "case": "host", "layout": "rooms_of_4", "streams": B, "loss": 0.10, "hops": a.hops,
                "reps": a.reps, "verified_ticks": n_ver}
        for k, ts in times.items():
            line[k] = stats(B, a.hops, ts)
        line["begin_end_over_host_three_calls"] = round(line["begin_end"]["ticks_x_streams_per_s_median"] /
                                                        line["host_three_calls"]["ticks_x_streams_per_s_median"], 3)
        print(json.dumps(line), flush=True)
        lines.append(line)
    finally:
        cc.close()
        ch.close()

    # ---- (d) the ceiling: run_steps, independent legs, no mix --------------------------------------------------------------
    cd = lyra_amd.LyraHip(device=0, max_streams=B)
    try:
        d_ring = t_(speech)
        d_rx = t_(rx)
        pkts = [torch.zeros((B, 15), dtype=torch.uint8, device=dev) for _ in range(2)]
        lens = [torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2)]
        outs = [torch.zeros((B, 320), dtype=torch.int16, device=dev) for _ in range(2)]

        def steps():
            cd.run_steps_dev(d_ids, 120, a.hops, 0, d_ring, pkts, outs, d_packet_bytes=lens, dtx=True, packet_loss=True,
                             d_received_ring=d_rx)

        times = timed({"run_steps": (steps, cd)}, a.reps)
        line = {"bench": "bridge", "case": "ceiling", "streams": B, "loss": 0.10, "hops": a.hops, "reps": a.reps,
                "run_steps": stats(B, a.hops, times["run_steps"]),
                "what": "encode (DTX) + lossy decode legs of lyra_hip_run_steps_dev, no mix, not verified against the bridge"}
        print(json.dumps(line), flush=True)
        lines.append(line)
    finally:
        cd.close()
    append(lines)


if __name__ == "__main__":
    main()
