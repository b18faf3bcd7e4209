#!/usr/bin/env python3
"""One long recording, encode then decode, time-parallel against hop by hop (BASELINE config #1: one file).

   python tools/span_bench.py [--hops 180000] [--lanes 4096] [--bits 184] [--rate 16000] [--dtx | --lossy | --mixed | --rates [--packed]]
                              [--out profiles/span_transcode.jsonl]

--rate 8000 / 32000 / 48000: the recording is at that rate and both legs run the `_ext` span calls and the file functions at it
(encode from the rate, decode to it); the baseline is the unchanged hop-by-hop calls at the same rate, lyra_hip_resample +
lyra_hip_encode / lyra_hip_decode + lyra_hip_resample per hop.  A third record, kernel_share, then gives the part of
span_resample_kernel in the device time of one encode + decode span call: this script runs its device leg once more as a child
under `rocprofv3 --kernel-trace --stats` (a run of its own, so the timed legs are not traced).

--dtx (with or without --rate): encode only, LyraEncoder's DTX on a half-silent recording (two seconds of speech, two of digital
silence, in turns).  dtx_transcode times lyra_hip_encode_spans_dtx_dev on device buffers (`verified`: a prefix of packets and
packet sizes against lyra_hip_resample + lyra_hip_encode_dtx per hop on a twin context); dtx_file_transcode times file_demo --dtx
with --time-parallel (EncodeWavsTimeParallel(enable_dtx)) against hop by hop (EncodeWavs(enable_dtx)) as whole processes, `verified`:
the same .lyra; kernel_share gives the part of span_noise_scan_kernel -- the serial floor of the call -- and of span_logmel_kernel
in the summed kernel time of the device leg.

--lossy (with or without --rate): decode only, a recording captured from a lossy link and one encoded with DTX.  Two
lossy_transcode records, trace "gilbert" (two-state loss chain: 5 % of the good hops start a burst, a burst ends after a hop with
probability 0.25 -- bursts of 4 hops on average, every length from isolated losses to full comfort noise) and trace "dtx" (the
sizes of lyra_hip_encode_spans_dtx_dev on the half-silent recording): lyra_hip_decode_spans_lossy_dev on device buffers against the
only other way to do the job, lyra_hip_decode_lossy_dev hop by hop on a twin context (B = 1, every call enqueued without a wait, one
synchronise at the end); `verified`: all four outputs of all hops equal.  kernel_share gives the part of span_lossy_scan_kernel --
the serial floor -- of span_logmel_map_kernel and of span_cng_kernel in the summed kernel time of the device leg.

--mixed (with or without --rate): per-frame bitrates (include/lyra_hip_spans_mixed.h).  The bitrate cycles 3200 -> 6000 -> 9200
every 50 hops.  One mixed_transcode record: lyra_hip_encode_spans_mixed_dev against the uniform span call at 184 bits on the same
audio, and lyra_hip_decode_spans_lossy_mixed_dev on the "gilbert" trace against lyra_hip_decode_spans_lossy_dev at 184 bits on the
same trace (`*_over_uniform`: mixed time / uniform time); both also against the only other way to do the job, the hop-by-hop mixed
calls lyra_hip_encode_mixed_dev / lyra_hip_decode_lossy_mixed_dev on a twin context (B = 1, every call enqueued without a wait,
one synchronise at the end); `verified`: packets up to their size and sizes, and all four decoder outputs, of all hops equal.

--rates: per-span sample rates (include/lyra_hip_spans_rates.h).  Four recordings of --hops hops each, at 8, 16, 32 and 48 kHz,
with --lanes lanes.  One rates_transcode record with, for the encode, lossy-decode ("gilbert" trace) and plain-decode families,
  (a) `*_s`               one rates call for all four recordings, the lanes shared;
  (b) `*_split_s`         the same work as four uniform span calls, one per rate, the lanes given to each in turn
                          (lyra_hip_encode_spans_mixed_dev, lyra_hip_decode_spans_lossy_mixed_dev, lyra_hip_decode_spans_ext_dev);
  (c) `*_hop_by_hop_s`    the hop-by-hop rates calls on a twin context (B = 4, every call enqueued without a wait, one synchronise
                          at the end; plain decode: lyra_hip_decode_dev and lyra_hip_resample_dev per rate);
`verified`: every output of (a) equals that of (b) byte for byte; steps / steps_split: the step counts of (a) and (b) from
lyra_hip_spans_plan (lossy: from lyra_hip_spans_lossy_plan_mixed).  kernel_share gives the part of span_resample_rates_kernel in
the summed kernel time of one call of each family.

--rates --packed: the packed external-rate layout and the host-buffer forms (include/lyra_hip_spans_packed.h).  The four
recordings of --rates, from HOST arrays, two ways, five timed runs each behind a warm one, per direction (encode, lossy decode on
the "gilbert" trace, plain decode):
  (a) `padded`   what a caller of the `_rates_dev` forms has to do: pad every row to 960 samples on the host, upload, call,
                 synchronise, download, and for the decodes cut the rows back to rate / 50 samples;
  (b) `packed`   one call of lyra_hip_encode_spans_packed / lyra_hip_decode_spans_lossy_packed / lyra_hip_decode_spans_packed.
One rates_packed_transcode record: per direction and way the median with min and max in seconds and the bytes moved each way;
`verified`: both ways give the same packets, sizes and samples; and `resample_pass_ms`: from lyra_hip_profile_*, the time of
span_resample_rates_kernel and of span_resample_packed_kernel per direction on the same recordings (median, min, max of five).

Records, appended to --out:
  span_transcode   lyra_hip_encode_spans_dev + lyra_hip_decode_spans_dev on device buffers, one stream of --hops hops with
                   --lanes lanes: wall time per direction (after a warm call), useful frames/s (the recording's hops, warm-up
                   hops not counted), the plan's step count and work inflation (L + W) / L, and `verified`: a prefix of
                   packets and PCM compared with the hop-by-hop calls lyra_hip_encode / lyra_hip_decode on a twin context.
  file_transcode   the same recording as a WAV file through lyra_amd/file_demo, hop by hop (EncodeFiles / DecodeFiles: one
                   blocking call per hop, B = 1) and with --time-parallel, timed in this run as whole processes (context
                   creation and file I/O included); `verified`: both runs wrote the same .lyra and the same decoded WAV.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
import wave

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def recording(hops, rate=16000):
    """speech of the golden recordings, looped, with a slowly varying gain and a little noise so that no two hops are equal
    (at another rate the same samples, read as a signal at that rate)"""
    w = np.load(os.path.join(ROOT, "tests", "golden", "sample_wavs.npz"))
    src = np.concatenate([w["sample1_16kHz"], w["sample2_16kHz"]]).astype(np.float32)
    n = hops * (rate // 50)
    rng = np.random.default_rng(7)
    x = src[np.arange(n) % src.size] * (0.6 + 0.4 * np.sin(np.arange(n) * 1e-5)) + rng.integers(-60, 61, n)
    return np.clip(x, -32768, 32767).astype(np.int16).reshape(hops, rate // 50)


def half_silent(pcm, rate):
    """two seconds of the recording, two of digital silence, in turns"""
    out = pcm.copy()
    for at in range(100, out.shape[0], 200):
        out[at:at + 100] = 0
    return out


def dtx_device_leg(args, pcm):
    import torch
    import lyra_amd
    from lyra_amd import codec
    dev = torch.device("cuda", 0)
    hops, ext = pcm.shape[0], args.rate != 16000
    ctx = lyra_amd.LyraHip(device=0, max_streams=args.lanes + 1, requant="xnnpack")
    ctx.set_encoder_sample_rate(args.rate)
    lanes = np.arange(1, args.lanes + 1, dtype=np.int32)
    spans = [(0, 0, hops)]
    d_pcm = torch.from_numpy(pcm).to(dev)
    d_pk = torch.zeros((hops, codec.packet_size(args.bits)), dtype=torch.uint8, device=dev)
    d_nb = torch.zeros(hops, dtype=torch.int32, device=dev)
    d_p16 = torch.zeros((hops, 320), dtype=torch.int16, device=dev) if ext else None
    times, front = [], []
    for rep in range(args.reps + 1):   # rep 0 warms (allocations, code)
        ctx.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.encode_spans_dtx_dev(spans, d_pcm, args.bits, d_pk, d_nb, lanes, sample_rate_hz=args.rate, d_pcm16=d_p16)
        ctx.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    nb = d_nb.cpu().numpy()
    for rep in range(0 if args.device_leg_only else args.reps):   # the estimator alone (log-mel pass + scan) on the call's 16 kHz audio
        ctx.reset()
        src16 = d_p16 if ext else d_pcm
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.noise_spans_dev(spans, src16, d_nb, side="encoder")
        ctx.synchronize()
        front.append(time.perf_counter() - t0)
    pk = d_pk.cpu().numpy()
    twin = lyra_amd.LyraHip(device=0, max_streams=1, requant="xnnpack")
    twin.set_encoder_sample_rate(args.rate)
    n, ok = min(hops, args.verify_hops), True
    for h in range(n):
        x16 = twin.resample(pcm[h:h + 1], args.rate, 16000, [0], side="encoder") if ext else pcm[h:h + 1]
        p, size = twin.encode_dtx(x16, args.bits, [0])
        ok = ok and size[0] == nb[h] and (size[0] == 0 or np.array_equal(p[0], pk[h]))
    t, f = float(np.median(times)), float(np.median(front)) if front else 0.0
    return dict(kind="dtx_transcode", rate=args.rate, hops=hops, lanes=int(args.lanes), bits=args.bits, active_hops=int((nb > 0).sum()),
                encode_s=round(t, 5), encode_frames_per_s=round(hops / t), estimator_s=round(f, 5), estimator_share=round(f / t, 4),
                reps=args.reps, verified=bool(ok), verified_hops=n)


def dtx_file_leg(args, pcm):
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "file_demo")
    bitrate = {64: 3200, 120: 6000, 184: 9200}[args.bits]
    hops = min(pcm.shape[0], args.file_hops) if args.file_hops else pcm.shape[0]
    rec = dict(kind="dtx_file_transcode", rate=args.rate, hops=hops, bits=args.bits, lanes=int(args.lanes))
    with tempfile.TemporaryDirectory() as tmp:
        wav = os.path.join(tmp, "recording.wav")
        with wave.open(wav, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(args.rate)
            w.writeframes(pcm[:hops].tobytes())
        outs = {}
        for name, flag in (("time_parallel", ["--time-parallel=%d" % args.lanes]), ("hop_by_hop", [])):
            out_dir = os.path.join(tmp, name)
            os.mkdir(out_dir)
            t0 = time.perf_counter()
            r = subprocess.run([demo, *flag, "--dtx", lyra_amd.default_model_dir(), str(bitrate), out_dir, wav],
                               capture_output=True, text=True, timeout=args.file_timeout)
            rec[name + "_s"] = round(time.perf_counter() - t0, 3)
            if r.returncode != 0:
                rec[name + "_error"] = r.stderr[-300:]
            outs[name] = os.path.join(out_dir, "recording.lyra")
            print(json.dumps({name + "_s": rec[name + "_s"]}), flush=True)
        a, b = outs["time_parallel"], outs["hop_by_hop"]
        rec["verified"] = bool(os.path.isfile(a) and os.path.isfile(b) and open(a, "rb").read() == open(b, "rb").read())
        if os.path.isfile(a):
            rec["lyra_bytes"] = os.path.getsize(a)
    if rec.get("time_parallel_s") and rec.get("hop_by_hop_s"):
        rec["hop_by_hop_over_time_parallel"] = round(rec["hop_by_hop_s"] / rec["time_parallel_s"], 2)
    return rec


def gilbert(hops, p_loss=0.05, p_recover=0.25, seed=5):
    """received[h] of a two-state loss chain"""
    rng = np.random.default_rng(seed)
    u = rng.random(hops)
    rx, lost = np.ones(hops, bool), False
    for h in range(hops):
        lost = (u[h] >= p_recover) if lost else (u[h] < p_loss)
        rx[h] = not lost
    return rx


def lossy_device_leg(args, pcm, trace):
    import torch
    import lyra_amd
    from lyra_amd import codec
    dev = torch.device("cuda", 0)
    hops, ext, nbytes = pcm.shape[0], args.rate != 16000, codec.packet_size(args.bits)
    ctx = lyra_amd.LyraHip(device=0, max_streams=args.lanes + 1, requant="xnnpack")
    ctx.set_encoder_sample_rate(args.rate)
    lanes = np.arange(1, args.lanes + 1, dtype=np.int32)
    spans = [(0, 0, hops)]
    d_pk = torch.zeros((hops, nbytes), dtype=torch.uint8, device=dev)
    d_w16 = torch.zeros((hops, 320), dtype=torch.int16, device=dev) if ext else None
    if trace == "dtx":
        d_nb = torch.zeros(hops, dtype=torch.int32, device=dev)
        ctx.encode_spans_dtx_dev(spans, torch.from_numpy(half_silent(pcm, args.rate)).to(dev), args.bits, d_pk, d_nb, lanes,
                                 sample_rate_hz=args.rate, d_pcm16=d_w16)
        ctx.synchronize()
        pb = d_nb.cpu().numpy()
    else:
        ctx.encode_spans_dev(spans, torch.from_numpy(pcm).to(dev), args.bits, d_pk, lanes, sample_rate_hz=args.rate, d_pcm16=d_w16)
        ctx.synchronize()
        pb = np.where(gilbert(hops), nbytes, 0).astype(np.int32)

    def outputs():
        return (torch.zeros((hops, 320), dtype=torch.int16, device=dev),
                torch.zeros((hops, args.rate // 50), dtype=torch.int16, device=dev) if ext else None,
                torch.zeros(hops, dtype=torch.int32, device=dev), torch.zeros(hops, dtype=torch.int32, device=dev))
    got, times = outputs(), []
    for rep in range(args.reps + 1):   # rep 0 warms (allocations, code)
        ctx.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.decode_spans_lossy_dev(spans, d_pk, pb, args.bits, got[0], lanes, sample_rate_hz=args.rate, d_pcm_ext=got[1],
                                   d_is_noise=got[2], d_is_comfort_noise=got[3])
        ctx.synchronize()
        if rep:
            times.append(time.perf_counter() - t0)
    plan = codec.spans_lossy_plan(spans, pb, nbytes, [0], lanes, args.lanes + 1)
    t = float(np.median(times))
    rec = dict(kind="lossy_transcode", trace=trace, rate=args.rate, hops=hops, lanes=int(args.lanes), bits=args.bits,
               received_hops=int((pb > 0).sum()), gen_hops=int(plan["counts"]["n_gen"][0]), cng_hops=int(plan["counts"]["n_cng"][0]),
               snapshots=int(plan["counts"]["n_versions"][0]), steps=int(plan["n_steps"]), decode_s=round(t, 5),
               decode_frames_per_s=round(hops / t), reps=args.reps)
    if args.device_leg_only:
        return rec
    twin = lyra_amd.LyraHip(device=0, max_streams=1, requant="xnnpack")
    want, d_pb, d_ids = outputs(), torch.from_numpy(pb).to(dev), torch.zeros(1, dtype=torch.int32, device=dev)
    base = []
    for rep in range(2):   # rep 0 warms
        twin.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for h in range(hops):
            twin.decode_lossy_dev(d_ids, d_pk[h:h + 1], d_pb[h:h + 1], args.bits, args.rate, want[0][h:h + 1],
                                  want[1][h:h + 1] if ext else None, want[2][h:h + 1], want[3][h:h + 1])
        twin.synchronize()
        base.append(time.perf_counter() - t0)
    same = all(torch.equal(a, b) for a, b in zip(got, want) if a is not None)
    rec.update(hop_by_hop_s=round(base[-1], 5), hop_by_hop_over_time_parallel=round(base[-1] / t, 2), verified=bool(same),
               verified_hops=hops)
    return rec


def mixed_device_leg(args, pcm):
    import torch
    import lyra_amd
    from lyra_amd import codec
    dev = torch.device("cuda", 0)
    hops, ext, row = pcm.shape[0], args.rate != 16000, codec.MAX_PACKET_BYTES
    ctx = lyra_amd.LyraHip(device=0, max_streams=args.lanes + 1, requant="xnnpack")
    lanes = np.arange(1, args.lanes + 1, dtype=np.int32)
    spans = [(0, 0, hops)]
    bits = np.array([64, 120, 184], np.int32)[(np.arange(hops) // 50) % 3]
    rx = gilbert(hops)
    pb = np.where(rx, (bits + 7) // 8, 0).astype(np.int32)
    d_pcm = torch.from_numpy(pcm).to(dev)
    d_w16 = torch.zeros((hops, 320), dtype=torch.int16, device=dev) if ext else None
    d_pk, d_pk184 = (torch.zeros((hops, row), dtype=torch.uint8, device=dev) for _ in range(2))
    d_nb = torch.zeros(hops, dtype=torch.int32, device=dev)

    def outputs():
        return (torch.zeros((hops, 320), dtype=torch.int16, device=dev),
                torch.zeros((hops, args.rate // 50), dtype=torch.int16, device=dev) if ext else None,
                torch.zeros(hops, dtype=torch.int32, device=dev), torch.zeros(hops, dtype=torch.int32, device=dev))
    got, uni = outputs(), outputs()
    legs = {   # the 8- and 15-byte packets are prefixes of the 184-bit one: the decode legs read d_pk184
        "encode": lambda: ctx.encode_spans_mixed_dev(spans, d_pcm, bits, d_pk, d_nb, lanes, sample_rate_hz=args.rate, d_pcm16=d_w16),
        "encode_uniform": lambda: ctx.encode_spans_dev(spans, d_pcm, 184, d_pk184, lanes, sample_rate_hz=args.rate, d_pcm16=d_w16),
        "decode": lambda: ctx.decode_spans_lossy_mixed_dev(spans, d_pk184, pb, got[0], lanes, sample_rate_hz=args.rate,
                                                           d_pcm_ext=got[1], d_is_noise=got[2], d_is_comfort_noise=got[3]),
        "decode_uniform": lambda: ctx.decode_spans_lossy_dev(spans, d_pk184, np.where(rx, row, 0).astype(np.int32), 184, uni[0], lanes,
                                                             sample_rate_hz=args.rate, d_pcm_ext=uni[1], d_is_noise=uni[2],
                                                             d_is_comfort_noise=uni[3]),
    }
    times = {k: [] for k in legs}
    for rep in range(args.reps + 1):   # rep 0 warms (allocations, code)
        for name, call in legs.items():
            ctx.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    t = {k: float(np.median(v)) for k, v in times.items()}
    plan = codec.spans_lossy_plan_mixed(spans, pb, [0], lanes, args.lanes + 1)
    rec = dict(kind="mixed_transcode", rate=args.rate, hops=hops, lanes=int(args.lanes), switch_every=50,
               received_hops=int(rx.sum()), steps_decode=int(plan["n_steps"]), reps=args.reps,
               encode_s=round(t["encode"], 5), encode_uniform_s=round(t["encode_uniform"], 5),
               encode_over_uniform=round(t["encode"] / t["encode_uniform"], 3), encode_frames_per_s=round(hops / t["encode"]),
               decode_s=round(t["decode"], 5), decode_uniform_s=round(t["decode_uniform"], 5),
               decode_over_uniform=round(t["decode"] / t["decode_uniform"], 3), decode_frames_per_s=round(hops / t["decode"]),
               mixed_errors=int(ctx.encode_mixed_errors()))
    if args.device_leg_only:
        return rec
    # hop by hop on a twin: a short warm run, then the whole recording
    twin = lyra_amd.LyraHip(device=0, max_streams=1, requant="xnnpack")
    d_ids, d_bits, d_pb = torch.zeros(1, dtype=torch.int32, device=dev), torch.from_numpy(bits).to(dev), torch.from_numpy(pb).to(dev)
    t_pk, t_nb, want = torch.zeros_like(d_pk), torch.zeros_like(d_nb), outputs()
    base = {}
    for n in (min(hops, 500), hops):
        twin.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for h in range(n):
            twin.encode_mixed_dev(d_ids, d_pcm[h:h + 1], args.rate, d_bits[h:h + 1], t_pk[h:h + 1], t_nb[h:h + 1])
        twin.synchronize()
        t1 = time.perf_counter()
        for h in range(n):
            twin.decode_lossy_mixed_dev(d_ids, d_pk184[h:h + 1], d_pb[h:h + 1], args.rate, want[0][h:h + 1],
                                        want[1][h:h + 1] if ext else None, want[2][h:h + 1], want[3][h:h + 1])
        twin.synchronize()
        base = dict(encode=t1 - t0, decode=time.perf_counter() - t1)
    live = torch.arange(row, device=dev)[None, :] < d_nb[:, None]
    same_enc = torch.equal(d_nb, t_nb) and torch.equal(d_nb.cpu(), torch.from_numpy((bits + 7) // 8)) and \
        torch.equal(torch.where(live, d_pk, 0), torch.where(live, t_pk, 0))
    same_dec = all(torch.equal(a, b) for a, b in zip(got, want) if a is not None)
    rec.update(encode_hop_by_hop_s=round(base["encode"], 5), decode_hop_by_hop_s=round(base["decode"], 5),
               encode_hop_by_hop_over_time_parallel=round(base["encode"] / t["encode"], 2),
               decode_hop_by_hop_over_time_parallel=round(base["decode"] / t["decode"], 2),
               verified=bool(same_enc and same_dec), verified_hops=hops)
    return rec


RATES = (8000, 16000, 32000, 48000)


def rates_device_leg(args):
    import torch
    import lyra_amd
    from lyra_amd import codec
    dev = torch.device("cuda", 0)
    hops, row, EXT, nbytes = args.hops, codec.MAX_PACKET_BYTES, codec.MAX_EXT_HOP, codec.packet_size(args.bits)
    F, n_streams = 4 * hops, 4 + args.lanes
    ctx = lyra_amd.LyraHip(device=0, max_streams=n_streams, requant="xnnpack")
    lanes = np.arange(4, n_streams, dtype=np.int32)
    spans = [(k, k * hops, hops) for k in range(4)]
    pcm = [recording(hops, r) for r in RATES]
    ext = np.zeros((F, EXT), np.int16)
    for k, x in enumerate(pcm):
        ext[k * hops:(k + 1) * hops, :x.shape[1]] = x
    bits = np.full(F, args.bits, np.int32)
    rx = gilbert(F)
    pb = np.where(rx, nbytes, 0).astype(np.int32)
    z = lambda *shape, dtype=torch.int16: torch.zeros(shape, dtype=dtype, device=dev)
    d_ext, d_p16, d_pk, d_nb = torch.from_numpy(ext).to(dev), z(F, 320), z(F, row, dtype=torch.uint8), z(F, dtype=torch.int32)
    lossy = (z(F, 320), z(F, EXT), z(F, dtype=torch.int32), z(F, dtype=torch.int32))
    plain = (z(F, 320), z(F, EXT))
    d_pkn = z(F, nbytes, dtype=torch.uint8)   # the plain decode's rows are nbytes apart
    one = {
        "encode": lambda: ctx.encode_spans_rates_dev(spans, d_ext, RATES, d_p16, bits, d_pk, d_nb, lanes),
        "lossy_decode": lambda: ctx.decode_spans_lossy_rates_dev(spans, d_pk, pb, RATES, lossy[0], lossy[1], lanes, d_is_noise=lossy[2],
                                                                 d_is_comfort_noise=lossy[3]),
        "plain_decode": lambda: ctx.decode_spans_rates_dev(spans, d_pkn, args.bits, RATES, plain[0], plain[1], lanes),
    }

    def timed(calls, reps):
        times = {k: [] for k in calls}
        for rep in range(reps + 1):   # rep 0 warms (allocations, code)
            for name, call in calls.items():
                ctx.reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                ctx.synchronize()
                if rep:
                    times[name].append(time.perf_counter() - t0)
                if name == "encode":
                    d_pkn.copy_(d_pk[:, :nbytes])
        return {k: float(np.median(v)) for k, v in times.items()}
    t = timed(one, args.reps)
    if args.device_leg_only:
        return dict(kind="rates_transcode", hops=hops, lanes=int(args.lanes))
    # (b) four uniform span calls on the same context, recording k as stream k, the lanes given to each in turn
    span1 = lambda k: [(k, 0, hops)]
    u_ext = [torch.from_numpy(x).to(dev) for x in pcm]
    u_p16 = [z(hops, 320) for _ in RATES]
    u_pk, u_nb = [z(hops, row, dtype=torch.uint8) for _ in RATES], [z(hops, dtype=torch.int32) for _ in RATES]
    u_lossy = [(z(hops, 320), z(hops, r // 50), z(hops, dtype=torch.int32), z(hops, dtype=torch.int32)) for r in RATES]
    u_plain = [(z(hops, 320), z(hops, r // 50)) for r in RATES]
    u_pkn = [z(hops, nbytes, dtype=torch.uint8) for _ in RATES]
    cut = lambda a, k: a[k * hops:(k + 1) * hops]

    def split_encode():
        for k, r in enumerate(RATES):
            ctx.encode_spans_mixed_dev(span1(k), u_ext[k], cut(bits, k), u_pk[k], u_nb[k], lanes, sample_rate_hz=r,
                                       d_pcm16=u_p16[k] if r != 16000 else None)

    def split_lossy():
        for k, r in enumerate(RATES):
            o = u_lossy[k]
            ctx.decode_spans_lossy_mixed_dev(span1(k), u_pk[k], cut(pb, k), o[0], lanes, sample_rate_hz=r,
                                             d_pcm_ext=o[1] if r != 16000 else None, d_is_noise=o[2], d_is_comfort_noise=o[3])

    def split_plain():
        for k, r in enumerate(RATES):
            o = u_plain[k]
            ctx.decode_spans_dev(span1(k), u_pkn[k], args.bits, o[1] if r != 16000 else o[0], lanes, sample_rate_hz=r,
                                 d_pcm16=o[0] if r != 16000 else None)
    ts = {}
    for name, call in (("encode", split_encode), ("lossy_decode", split_lossy), ("plain_decode", split_plain)):
        times = []
        for rep in range(args.reps + 1):
            ctx.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            if rep:
                times.append(time.perf_counter() - t0)
        ts[name] = float(np.median(times))
        if name == "encode":
            for k in range(4):
                u_pkn[k].copy_(u_pk[k][:, :nbytes])
    same = True
    for k, r in enumerate(RATES):
        hop = r // 50
        same = same and torch.equal(cut(d_nb, k), u_nb[k]) and torch.equal(cut(d_pk, k)[:, :nbytes], u_pk[k][:, :nbytes])
        same = same and (r == 16000 or torch.equal(cut(d_p16, k), u_p16[k]))
        same = same and torch.equal(cut(lossy[0], k), u_lossy[k][0]) and torch.equal(cut(lossy[2], k), u_lossy[k][2]) and \
            torch.equal(cut(lossy[3], k), u_lossy[k][3]) and torch.equal(cut(plain[0], k), u_plain[k][0])
        same = same and torch.equal(cut(lossy[1], k)[:, :hop], u_lossy[k][1] if r != 16000 else u_lossy[k][0])
        same = same and torch.equal(cut(plain[1], k)[:, :hop], u_plain[k][1] if r != 16000 else u_plain[k][0])
    # (c) hop by hop on a twin, B = 4
    twin = lyra_amd.LyraHip(device=0, max_streams=4, requant="xnnpack")
    d_ids, d_rates = torch.arange(4, dtype=torch.int32, device=dev), torch.tensor(RATES, dtype=torch.int32, device=dev)
    h_ext = d_ext.view(4, hops, EXT).transpose(0, 1).contiguous()           # [hops][4][960]
    h_bits = torch.full((4,), args.bits, dtype=torch.int32, device=dev)
    h_pk, h_nb = z(hops, 4, row, dtype=torch.uint8), z(hops, 4, dtype=torch.int32)
    h_pb = torch.from_numpy(pb).to(dev).view(4, hops).transpose(0, 1).contiguous()
    h_out = (z(hops, 4, 320), z(hops, 4, EXT), z(hops, 4, dtype=torch.int32), z(hops, 4, dtype=torch.int32))
    h_pkn, h_16 = z(hops, 4, nbytes, dtype=torch.uint8), z(hops, 4, 320)
    h_rs = {r: z(hops, 1, r // 50) for r in RATES if r != 16000}
    one_id = {r: torch.tensor([k], dtype=torch.int32, device=dev) for k, r in enumerate(RATES)}

    def hbh_encode(n):
        for h in range(n):
            twin.encode_rates_dev(d_ids, h_ext[h], d_rates, h_bits, h_pk[h], h_nb[h])

    def hbh_lossy(n):
        for h in range(n):
            twin.decode_lossy_rates_dev(d_ids, h_pk[h], h_pb[h], d_rates, h_out[0][h], h_out[1][h], h_out[2][h], h_out[3][h])

    def hbh_plain(n):
        for h in range(n):
            twin.decode_dev(d_ids, h_pkn[h], args.bits, h_16[h])
            for k, r in enumerate(RATES):
                if r != 16000:
                    twin.resample_dev(one_id[r], h_16[h, k:k + 1], 16000, r, h_rs[r][h], side="decoder")
    tc = {}
    for name, call in (("encode", hbh_encode), ("lossy_decode", hbh_lossy), ("plain_decode", hbh_plain)):
        for n in (min(hops, 300), hops):   # a short warm run, then the whole recordings
            twin.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call(n)
            twin.synchronize()
            tc[name] = time.perf_counter() - t0
        if name == "encode":
            h_pkn.copy_(h_pk[:, :, :nbytes])
    same_hbh = torch.equal(h_pk.transpose(0, 1).reshape(F, row)[:, :nbytes], d_pk[:, :nbytes]) and \
        torch.equal(h_out[0].transpose(0, 1).reshape(F, 320), lossy[0]) and torch.equal(h_16.transpose(0, 1).reshape(F, 320), plain[0])
    _, steps = codec.spans_plan("encoder", spans, lanes, n_streams)
    _, steps1 = codec.spans_plan("encoder", span1(0), lanes, n_streams)
    lossy_steps = codec.spans_lossy_plan_mixed(spans, pb, [0] * 4, lanes, n_streams)["n_steps"]
    lossy_split = sum(codec.spans_lossy_plan_mixed(span1(k), cut(pb, k), [0], lanes, n_streams)["n_steps"] for k in range(4))
    rec = dict(kind="rates_transcode", hops=hops, recordings=4, lanes=int(args.lanes), bits=args.bits, reps=args.reps,
               warmup=codec.span_warmup_frames("encoder"), steps=int(steps), steps_split=int(4 * steps1),
               lossy_steps=int(lossy_steps), lossy_steps_split=int(lossy_split), received_hops=int(rx.sum()),
               verified=bool(same), verified_hop_by_hop=bool(same_hbh))
    for name in one:
        rec.update({name + "_s": round(t[name], 5), name + "_split_s": round(ts[name], 5), name + "_hop_by_hop_s": round(tc[name], 5),
                    name + "_split_over_one": round(ts[name] / t[name], 3), name + "_hop_by_hop_over_one": round(tc[name] / t[name], 2)})
    return rec


def rates_packed_leg(args):
    import ctypes as C
    import torch
    import lyra_amd
    from lyra_amd import codec
    dev = torch.device("cuda", 0)
    hops, row, EXT, nbytes = args.hops, codec.MAX_PACKET_BYTES, codec.MAX_EXT_HOP, codec.packet_size(args.bits)
    F, n_streams, runs = 4 * hops, 4 + args.lanes, 5
    ctx = lyra_amd.LyraHip(device=0, max_streams=n_streams, requant="xnnpack")
    lanes = np.arange(4, n_streams, dtype=np.int32)
    spans = [(k, k * hops, hops) for k in range(4)]
    sp, rates = codec._spans(spans), np.asarray(RATES, np.int32)
    pcm = [recording(hops, r) for r in RATES]
    flat = np.concatenate([x.reshape(-1) for x in pcm])
    offsets, total = codec.spans_packed_layout(spans, RATES)
    assert total == flat.size
    bits = np.full(F, args.bits, np.int32)
    pb = np.where(gilbert(F), nbytes, 0).astype(np.int32)
    head = (ctx.h, sp.ctypes.data, sp.size, lanes.ctypes.data, lanes.size)
    z = lambda *shape, dtype=torch.int16: torch.zeros(shape, dtype=dtype, device=dev)
    moved = {}

    def unpad(rows):   # [F][960] -> the flat layout
        return np.concatenate([rows[k * hops:(k + 1) * hops, :r // 50].reshape(-1) for k, r in enumerate(RATES)])

    def padded_encode():
        ext = np.zeros((F, EXT), np.int16)
        for k, x in enumerate(pcm):
            ext[k * hops:(k + 1) * hops, :x.shape[1]] = x
        d_pk, d_nb = z(F, row, dtype=torch.uint8), z(F, dtype=torch.int32)
        ctx.encode_spans_rates_dev(spans, torch.from_numpy(ext).to(dev), RATES, z(F, 320), bits, d_pk, d_nb, lanes)
        ctx.synchronize()
        moved["encode", "padded"] = (ext.nbytes, F * row + F * 4)
        return d_pk.cpu().numpy(), d_nb.cpu().numpy()

    def packed_encode():
        moved["encode", "packed"] = (flat.nbytes, F * row + F * 4)
        return ctx.encode_spans_packed(spans, flat, RATES, bits, lanes)

    def padded_decode(lossy, rows_np):
        d_ext = z(F, EXT)
        if lossy:
            ctx.decode_spans_lossy_rates_dev(spans, torch.from_numpy(rows_np).to(dev), pb, RATES, z(F, 320), d_ext, lanes)
        else:
            ctx.decode_spans_rates_dev(spans, torch.from_numpy(rows_np).to(dev), args.bits, RATES, z(F, 320), d_ext, lanes)
        ctx.synchronize()
        moved["lossy_decode" if lossy else "plain_decode", "padded"] = (rows_np.nbytes, F * EXT * 2)
        return unpad(d_ext.cpu().numpy())

    def packed_decode(lossy, rows_np):   # through the C ABI: without the optional 16 kHz output
        out = np.zeros(total, np.int16)
        if lossy:
            rc = ctx.L.lyra_hip_decode_spans_lossy_packed(*head, rows_np.ctypes.data, pb.ctypes.data, rates.ctypes.data, None,
                                                          out.ctypes.data, total, None, None, None)
        else:
            rc = ctx.L.lyra_hip_decode_spans_packed(*head, rows_np.ctypes.data, args.bits, rates.ctypes.data, None, out.ctypes.data,
                                                    total, None)
        assert rc == 0, ctx.last_error()
        moved["lossy_decode" if lossy else "plain_decode", "packed"] = (rows_np.nbytes, out.nbytes)
        return out

    def timed(call):
        times, result = [], None
        for run in range(runs + 1):   # run 0 warms (allocations, code)
            ctx.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result = call()
            if run:
                times.append(time.perf_counter() - t0)
        return times, result

    rec = dict(kind="rates_packed_transcode", hops=hops, recordings=4, lanes=int(args.lanes), bits=args.bits, runs=runs,
               samples_packed=int(total), samples_padded=int(F * EXT))
    stat = lambda v: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))
    t_pad, (pk, nb) = timed(padded_encode)
    t_pkd, (pk2, nb2) = timed(packed_encode)
    ok = bool(np.array_equal(nb, nb2) and np.array_equal(pk, pk2))
    rec["encode"] = dict(padded_s=stat(t_pad), packed_s=stat(t_pkd))
    rows23, rows_n = np.ascontiguousarray(pk), np.ascontiguousarray(pk[:, :nbytes])
    for name, lossy, rows_np in (("lossy_decode", True, rows23), ("plain_decode", False, rows_n)):
        t_pad, a = timed(lambda: padded_decode(lossy, rows_np))
        t_pkd, b = timed(lambda: packed_decode(lossy, rows_np))
        ok = ok and bool(np.array_equal(a, b))
        rec[name] = dict(padded_s=stat(t_pad), packed_s=stat(t_pkd))
    for (name, way), (up, down) in moved.items():
        rec[name][way + "_bytes_up"], rec[name][way + "_bytes_down"] = int(up), int(down)
    rec["verified"] = ok
    # the resampler pass alone, on device buffers: the padded kernel and the packed one, per direction
    kernels = ("span_resample_rates_kernel", "span_resample_packed_kernel")
    ext = np.zeros((F, EXT), np.int16)
    for k, x in enumerate(pcm):
        ext[k * hops:(k + 1) * hops, :x.shape[1]] = x
    d_pad, d_flat, d_p16 = torch.from_numpy(ext).to(dev), torch.from_numpy(flat).to(dev), z(F, 320)
    d_pk, d_nb, d_pkn = z(F, row, dtype=torch.uint8), z(F, dtype=torch.int32), torch.from_numpy(rows_n).to(dev)
    passes = {
        ("encode", kernels[0]): lambda: ctx.encode_spans_rates_dev(spans, d_pad, RATES, d_p16, bits, d_pk, d_nb, lanes),
        ("encode", kernels[1]): lambda: ctx.encode_spans_packed_dev(spans, d_flat, RATES, d_p16, bits, d_pk, d_nb, lanes),
        ("plain_decode", kernels[0]): lambda: ctx.decode_spans_rates_dev(spans, d_pkn, args.bits, RATES, d_p16, d_pad, lanes),
        ("plain_decode", kernels[1]): lambda: ctx.decode_spans_packed_dev(spans, d_pkn, args.bits, RATES, d_p16, d_flat, lanes),
    }
    ctx.profile_enable(True, only=list(kernels))
    rec["resample_pass_ms"] = {}
    for (name, kernel), call in passes.items():
        ms = []
        for run in range(runs + 1):
            ctx.reset()
            call()
            ctx.synchronize()
            got = ctx.profile_read()[kernel]
            assert got[1] == 1, (kernel, got)
            if run:
                ms.append(got[0])
        rec["resample_pass_ms"].setdefault(name, {})[kernel] = stat(ms)
    ctx.profile_enable(False)
    return rec


def device_leg(args, pcm):
    import torch
    import lyra_amd
    from lyra_amd import codec
    dev = torch.device("cuda", 0)
    hops = pcm.shape[0]
    ctx = lyra_amd.LyraHip(device=0, max_streams=args.lanes + 1, requant="xnnpack")
    lanes = np.arange(1, args.lanes + 1, dtype=np.int32)
    spans = [(0, 0, hops)]
    chunks, steps = codec.spans_plan("encoder", spans, lanes, args.lanes + 1)
    W = codec.span_warmup_frames("encoder")
    lane_chunks = chunks[chunks["n_warmup"] > 0]
    L = int(lane_chunks["n_frames"].max()) if lane_chunks.size else hops
    d_pcm = torch.from_numpy(pcm).to(dev)
    d_pk = torch.zeros((hops, codec.packet_size(args.bits)), dtype=torch.uint8, device=dev)
    d_out = torch.zeros((hops, args.rate // 50), dtype=torch.int16, device=dev)
    ext = args.rate != 16000
    kw = dict(sample_rate_hz=args.rate, d_pcm16=torch.zeros((hops, 320), dtype=torch.int16, device=dev)) if ext else {}
    times = {"encode": [], "decode": []}
    for rep in range(args.reps + 1):   # rep 0 warms (allocations, code)
        ctx.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.encode_spans_dev(spans, d_pcm, args.bits, d_pk, lanes, **kw)
        ctx.synchronize()
        t1 = time.perf_counter()
        ctx.decode_spans_dev(spans, d_pk, args.bits, d_out, lanes, **kw)
        ctx.synchronize()
        t2 = time.perf_counter()
        if rep:
            times["encode"].append(t1 - t0)
            times["decode"].append(t2 - t1)
    pk, out = d_pk.cpu().numpy(), d_out.cpu().numpy()
    # verified: a prefix against the hop-by-hop calls on a twin context (it crosses the first chunk boundaries)
    twin = lyra_amd.LyraHip(device=0, max_streams=1, requant="xnnpack")
    n = min(hops, args.verify_hops)
    ok = True
    for h in range(n):
        x16 = twin.resample(pcm[h:h + 1], args.rate, 16000, [0], side="encoder") if ext else pcm[h:h + 1]
        p = twin.encode(x16, args.bits, [0])
        o = twin.decode(p, args.bits, [0])
        if ext:
            o = twin.resample(o, 16000, args.rate, [0], side="decoder")
        ok = ok and np.array_equal(p[0], pk[h]) and np.array_equal(o[0], out[h])
    enc, dec = float(np.median(times["encode"])), float(np.median(times["decode"]))
    return dict(kind="span_transcode", rate=args.rate, hops=hops, lanes=int(args.lanes), bits=args.bits, chunks=int(len(chunks)), steps=int(steps),
                warmup=W, chunk_hops=L, inflation=round((L + W) / L, 4) if lane_chunks.size else 1.0,
                encode_s=round(enc, 5), decode_s=round(dec, 5), encode_frames_per_s=round(hops / enc),
                decode_frames_per_s=round(hops / dec), reps=args.reps, verified=bool(ok), verified_hops=n)


def file_leg(args, pcm):
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "file_demo")
    bitrate = {64: 3200, 120: 6000, 184: 9200}[args.bits]
    hops = min(pcm.shape[0], args.file_hops) if args.file_hops else pcm.shape[0]
    rec = dict(kind="file_transcode", rate=args.rate, hops=hops, bits=args.bits, lanes=int(args.lanes))
    with tempfile.TemporaryDirectory() as tmp:
        wav = os.path.join(tmp, "recording.wav")
        with wave.open(wav, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(args.rate)
            w.writeframes(pcm[:hops].tobytes())
        outs = {}
        for name, flag in (("time_parallel", ["--time-parallel=%d" % args.lanes]), ("hop_by_hop", [])):
            out_dir = os.path.join(tmp, name)
            os.mkdir(out_dir)
            t0 = time.perf_counter()
            r = subprocess.run([demo, *flag, "--decode-rate=%d" % args.rate, lyra_amd.default_model_dir(), str(bitrate), out_dir, wav],
                               capture_output=True, text=True, timeout=args.file_timeout)
            rec[name + "_s"] = round(time.perf_counter() - t0, 3)
            if r.returncode != 0:
                rec[name + "_error"] = r.stderr[-300:]
            outs[name] = out_dir
            print(json.dumps({name + "_s": rec[name + "_s"]}), flush=True)
        same = True
        for f in ("recording.lyra", "recording_decoded.wav"):
            a, b = (os.path.join(outs[k], f) for k in ("time_parallel", "hop_by_hop"))
            same = same and os.path.isfile(a) and os.path.isfile(b) and open(a, "rb").read() == open(b, "rb").read()
        rec["verified"] = bool(same)
    if rec.get("time_parallel_s") and rec.get("hop_by_hop_s"):
        rec["hop_by_hop_over_time_parallel"] = round(rec["hop_by_hop_s"] / rec["time_parallel_s"], 2)
    return rec


def kernel_share_leg(args):
    """this script's device leg (one warm and one timed call per direction) as a child under rocprofv3 --kernel-trace --stats:
    the share of span_resample_kernel in the summed kernel time of the process"""
    import csv
    import glob
    rec = dict(kind="kernel_share", rate=args.rate, hops=args.hops, lanes=int(args.lanes), bits=args.bits, dtx=bool(args.dtx))
    names = ["span_noise_scan_kernel", "span_logmel_kernel", "span_resample_kernel"] if args.dtx else ["span_resample_kernel"]
    if args.rates:
        rec = dict(kind="kernel_share", rates=True, hops=args.hops, lanes=int(args.lanes), bits=args.bits)
        names = ["span_resample_rates_kernel"]
    if args.lossy:
        rec["lossy"] = True
        names = ["span_lossy_scan_kernel", "span_logmel_map_kernel", "span_cng_kernel", "span_resample_kernel"]
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "span", "--",
               sys.executable, os.path.abspath(__file__), "--device-leg-only", "--reps", "1", "--verify-hops", "0",
               "--hops", str(args.hops), "--lanes", str(args.lanes), "--bits", str(args.bits), "--rate", str(args.rate)]
        cmd += ["--dtx"] if args.dtx else []
        cmd += ["--lossy"] if args.lossy else []
        cmd += ["--rates"] if args.rates else []
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.file_timeout)
        stats = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not stats:
            rec["error"] = (r.stderr or r.stdout)[-300:]
            return rec
        total, mine, calls = 0, dict.fromkeys(names, 0), dict.fromkeys(names, 0)
        for row in csv.DictReader(open(stats[0])):
            ns = int(float(row["TotalDurationNs"]))
            total += ns
            for k in names:
                if k in row["Name"]:
                    mine[k] += ns
                    calls[k] += int(row["Calls"])
        rec["kernel_time_ms"] = round(total / 1e6, 3)
        for k in names:
            short = k[:-len("_kernel")]
            rec.update({short + "_ms": round(mine[k] / 1e6, 3), short + "_calls": calls[k],
                        short + "_share": round(mine[k] / total, 5) if total else None})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hops", type=int, default=180000)
    ap.add_argument("--lanes", type=int, default=4096)
    ap.add_argument("--bits", type=int, default=184)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--verify-hops", type=int, default=400)
    ap.add_argument("--file-hops", type=int, default=0, help="hops of the file leg (0: all)")
    ap.add_argument("--file-timeout", type=int, default=900)
    ap.add_argument("--skip-file-leg", action="store_true")
    ap.add_argument("--rate", type=int, default=16000, choices=[8000, 16000, 32000, 48000])
    ap.add_argument("--dtx", action="store_true", help="LyraEncoder's DTX on a half-silent recording, encode only")
    ap.add_argument("--lossy", action="store_true", help="decode only: a Gilbert loss trace and a DTX trace, time-parallel against hop by hop")
    ap.add_argument("--mixed", action="store_true", help="per-frame bitrates, switching every 50 hops: against the uniform span calls "
                    "and the hop-by-hop mixed calls")
    ap.add_argument("--rates", action="store_true", help="per-span sample rates: four recordings at 8 / 16 / 32 / 48 kHz in one call "
                    "against four uniform span calls and the hop-by-hop rates calls")
    ap.add_argument("--packed", action="store_true", help="with --rates: the packed layout and the host-buffer forms against padding "
                    "on the host around the `_rates_dev` forms, and the two resampler kernels' times")
    ap.add_argument("--device-leg-only", action="store_true", help="the device leg alone, nothing recorded (the traced child)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "span_transcode.jsonl"))
    args = ap.parse_args()
    if args.packed:
        if not args.rates:
            ap.error("--packed goes with --rates")
        rec = rates_packed_leg(args)
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        return
    if args.rates:
        recs = [rates_device_leg(args)]
        print(json.dumps(recs[0]), flush=True)
        if not args.device_leg_only:
            recs.append(kernel_share_leg(args))
            print(json.dumps(recs[-1]), flush=True)
            with open(args.out, "a") as f:
                for r in recs:
                    f.write(json.dumps(r) + "\n")
        return
    pcm = recording(args.hops, args.rate)
    if args.mixed:
        rec = mixed_device_leg(args, pcm)
        print(json.dumps(rec), flush=True)
        if not args.device_leg_only:
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
        return
    if args.lossy:
        recs = []
        for trace in ("gilbert", "dtx"):
            recs.append(lossy_device_leg(args, pcm, trace))
            print(json.dumps(recs[-1]), flush=True)
        if not args.device_leg_only:
            recs.append(kernel_share_leg(args))
            print(json.dumps(recs[-1]), flush=True)
            with open(args.out, "a") as f:
                for r in recs:
                    f.write(json.dumps(r) + "\n")
        return
    if args.dtx:
        pcm = half_silent(pcm, args.rate)
    recs = [dtx_device_leg(args, pcm) if args.dtx else device_leg(args, pcm)]
    print(json.dumps(recs[0]), flush=True)
    if args.device_leg_only:
        return
    if not args.skip_file_leg:
        recs.append(dtx_file_leg(args, pcm) if args.dtx else file_leg(args, pcm))
        print(json.dumps(recs[-1]), flush=True)
    if args.rate != 16000 or args.dtx:
        recs.append(kernel_share_leg(args))
        print(json.dumps(recs[-1]), flush=True)
    with open(args.out, "a") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
