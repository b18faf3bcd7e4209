"""lyra_hip_decode_spans_lossy on the GPU (include/lyra_hip.h "Time-parallel spans", packet loss): LyraDecoder's loss path --
concealment, comfort noise, cross-fades, the decoder-side NoiseEstimator -- over whole spans.  Every comparison is BIT FOR BIT
against lyra_hip_decode_lossy_dev hop by hop on a twin context with the same stream ids and comfort-noise seed: the 16 kHz
hops, the external-rate hops, is_noise, is_comfort_noise, the filler outside the spans, the span streams' exported state (the
whole blob: decoder stages, estimator, comfort-noise and resampler slots) and the lanes' against the twin's untouched lanes.

The loss traces are built here, and what they have to exercise is asserted before anything is compared (_assert_trace): on
the plan -- a burst that starts inside a lane chunk's warm-up, one that straddles a chunk boundary -- and on the TWIN's
output -- two comfort-noise stretches of the 350-frame span read different estimates, the comfort-noise hops are not silent,
a received tick cross-fades back from comfort noise.

Stream kind: the contexts here (96 streams) run on the CU-masked streams the library picks up to 1,024 streams, which are
blocking streams with respect to the NULL stream; the case with streams="plain" runs on hipStreamNonBlocking streams, the kind
of a 4,096-stream context (tests/gpu_plumbing.py make_ctx)."""
import os
import subprocess
import wave

import numpy as np
import pytest

from gpu_plumbing import FILL, _filled, make_ctx, stream_cases
from signals import _bursts, _long_trace, _speech_hops as _speech, _stretches
from span_cases import (CNG, GEN, _check_rows, _check_state, _dirty_lane, _layout, _packets,
                        _twin_decode_lossy as _twin_decode)

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MAX_STREAMS = 96
SEED = 0x5EEDC0DE


def _ctx(mode="xnnpack", rate=16000, streams=None):
    return make_ctx(MAX_STREAMS, mode, rate, SEED, streams=streams)


def _assert_trace(where, plan, k_long, rx_long, est_after, want_16, want_cn, need_plan_bursts):
    """what the trace has to exercise (module docstring); plan: the call's, k_long: the 350-frame span's index in it"""
    import lyra_amd.codec as codec
    W = codec.span_warmup_frames("decoder")
    counts = plan["counts"]
    g0 = int(counts["n_gen"][:k_long].sum())
    grx = plan["gen_received"]
    lane_chunks = [c for c in plan["chunks"] if c["span"] == k_long and c["n_warmup"] > 0]
    assert len(lane_chunks) >= 2, (where, "the long span is not cut into several lane chunks")
    if need_plan_bursts:
        starts = lambda lo, hi: [g for g in range(max(lo, g0 + 1), hi) if not grx[g] and grx[g - 1]]
        assert any(starts(int(c["first_frame"]) - W, int(c["first_frame"])) for c in lane_chunks), (where, "no burst starts in a warm-up")
        assert any(not grx[int(c["first_frame"])] and not grx[int(c["first_frame"]) - 1] for c in lane_chunks), \
            (where, "no burst straddles a chunk boundary")
    assert k_long == 0   # (the long span is the call's first: its lists lie in front)
    info = plan["info"][:350]
    runs = _stretches((info & CNG) != 0)
    assert len(runs) >= 2, (where, "fewer than two comfort-noise stretches")
    assert any((info[a:b] & GEN == 0).any() for a, b in runs), (where, "no tick of pure comfort noise")
    seen = [est_after[a - 1] for a, b in runs if a > 0]
    assert any(not np.array_equal(seen[0], e) for e in seen[1:]), (where, "every comfort-noise stretch reads the same estimate")
    pure = np.flatnonzero(want_cn == 1)
    assert len(pure) and np.abs(want_16[pure].astype(np.int32)).max() > 0, (where, "the comfort noise is silent")
    # on the twin's output: a tick with a packet that is no longer comfort noise, right behind one that was
    back = [h for h in range(1, 350) if rx_long[h] and want_cn[h - 1] == 1 and want_cn[h] == 0]
    assert back, (where, "no received tick cross-fades back from comfort noise")
    assert counts["n_versions"][k_long] >= 2


CASES = [(16000, 184, "xnnpack", "loss"), (48000, 64, "xnnpack", "loss"), (8000, 184, "builtin_mixed", "loss"),
         (16000, 64, "xnnpack", "dtx")]


@pytest.mark.parametrize("rate,num_bits,mode,kind", CASES)
def test_one_call_of_mixed_span_lengths_equals_hop_by_hop_lossy(golden_dir, rate, num_bits, mode, kind):
    """Span lengths 350, 1, 0, 26 (all lost), W + 18 (a burst at its very start and one at its very end) and 7 (all received) in
    one call with 40 lanes, two pairs of spans touching; kind "dtx": the long span's packets and sizes are encode_spans_dtx's on
    the half-silent input."""
    import torch
    import lyra_amd.codec as codec
    W = codec.span_warmup_frames("decoder")
    ctx, twin, enc = _ctx(mode), _ctx(mode), _ctx(mode)
    dev = torch.device("cuda", 0)
    hop, nb = rate // 50, (num_bits + 7) // 8
    lanes = np.arange(24, 24 + 40, dtype=np.int32)
    lengths = {7: 350, 11: 1, 3: 0, 20: 26, 5: W + 18, 9: 7}
    gaps = [2, 0, 3, 3, 0, 1]
    rx = {11: np.zeros(1, bool), 3: np.zeros(0, bool), 20: np.zeros(26, bool),
          5: _bursts(W + 18, (0, 5), (12, 1), (20, 6), (W + 9, 9)), 9: np.ones(7, bool)}
    pk = {i: _packets(enc, golden_dir, n, num_bits, 300 + i) for i, n in lengths.items()}
    spans, buf = _layout(pk, gaps)
    F = len(buf)
    def sizes_of(rx7):
        pb = np.full(F, FILL, np.int32)
        for (i, first, n) in spans:
            pb[first:first + n] = np.where(rx7 if i == 7 else rx[i], nb, 0)
        return pb
    def plan_of(rx7):
        return codec.spans_lossy_plan(spans, sizes_of(rx7), nb, [0] * len(spans), lanes, MAX_STREAMS), spans[0][1]
    if kind == "dtx":
        enc.reset([0])
        pk[7], sizes = enc.encode_spans_dtx([(0, 0, 350)], _speech(golden_dir, 350, 41, half_silent=True), num_bits,
                                            np.arange(1, 41, dtype=np.int32))
        rx[7] = sizes > 0
        assert 60 <= rx[7].sum() <= 290 and max(b - a for a, b in _stretches(~rx[7])) >= 8, "the DTX trace"
        spans, buf = _layout(pk, gaps)
    else:
        rx[7] = _long_trace(plan_of)
    _dirty_lane((ctx, twin), int(lanes[3]), golden_dir)
    where = f"{mode}/{rate}/{num_bits}/{kind}"
    want_16, want_ext, want_n, want_cn, est = _twin_decode(twin, pk, rx, rate, num_bits, watch=7)
    pb = sizes_of(rx[7])
    plan, _ = plan_of(rx[7])
    _assert_trace(where, plan, 0, rx[7], est, want_16[7], want_cn[7], kind == "loss")
    d_pk = torch.from_numpy(buf).to(dev)
    d_16, d_ext = _filled(dev, F, 320, np.int16), _filled(dev, F, hop, np.int16)
    d_n, d_cn = _filled(dev, F, 1, np.int32).view(-1), _filled(dev, F, 1, np.int32).view(-1)
    ctx.decode_spans_lossy_dev(spans, d_pk, pb, num_bits, d_16, lanes, sample_rate_hz=rate,
                               d_pcm_ext=d_ext if rate != 16000 else None, d_is_noise=d_n, d_is_comfort_noise=d_cn)
    ctx.synchronize()
    _check_rows(where + " is_comfort_noise", d_cn.cpu().numpy().reshape(F, 1), spans, want_cn)
    _check_rows(where + " is_noise", d_n.cpu().numpy().reshape(F, 1), spans, want_n)
    _check_rows(where + " pcm16", d_16.cpu().numpy(), spans, want_16)
    if rate != 16000:
        _check_rows(where + " pcm_ext", d_ext.cpu().numpy(), spans, want_ext)
    else:
        assert (d_ext.cpu().numpy().view(np.uint8) == FILL).all()
    assert np.array_equal(d_pk.cpu().numpy(), buf), f"{where}: the packet buffer was written"
    _check_state(where, ctx, twin, list(lengths), lanes)


@pytest.mark.parametrize("n_lanes,streams", stream_cases([40, 0], plain=40))
def test_span_continues_a_live_lossy_stream_mid_burst_and_is_continued(golden_dir, n_lanes, streams):
    """5 lost ticks hop by hop, a span of 200 that begins inside that burst and ends inside another, 10 more ticks hop by hop
    (two lost, then packets): all three pieces equal the twin that went hop by hop throughout.  n_lanes = 0: sequential."""
    ctx, twin, enc = _ctx(streams=streams), _ctx(streams=streams), _ctx()
    sid, k, n, tail, bits, rate = 13, 5, 200, 10, 120, 32000
    lanes = np.arange(30, 30 + n_lanes, dtype=np.int32)
    pk = _packets(enc, golden_dir, k + n + tail, bits, 55)
    rx = _bursts(k + n + tail, (0, 9), (40, 1), (70, 11), (120, 4), (150, 30), (k + n - 3, 5))
    want = _twin_decode(twin, {sid: pk}, {sid: rx}, rate, bits)
    head = _twin_decode(ctx, {sid: pk[:k]}, {sid: rx[:k]}, rate, bits)
    pb = np.where(rx, (bits + 7) // 8, 0)
    mid = ctx.decode_spans_lossy([(sid, k, n)], pk, pb, bits, lanes, sample_rate_hz=rate)
    for a in mid:
        assert not a[:k].any() and not a[k + n:].any()
    rest = _twin_decode(ctx, {sid: pk[k + n:]}, {sid: rx[k + n:]}, rate, bits)
    for name, w, h, m, r in zip(("pcm16", "pcm_ext", "is_noise", "is_comfort_noise"), want, head, mid, rest):
        got = np.concatenate([h[sid], m[k:k + n], r[sid]])
        diff = np.flatnonzero((got.reshape(len(got), -1) != w[sid].reshape(len(got), -1)).any(axis=1))
        assert len(diff) == 0, (name, list(diff[:8]), len(diff))
    assert want[3][sid][k:k + n].any() and not want[3][sid][k:k + n].all()
    _check_state("continued stream", ctx, twin, [sid], lanes)


def test_refusals_change_nothing(golden_dir):
    """LYRA_HIP_EINVAL before the first kernel: no slot, no buffer changes; the call that follows equals the twin."""
    import torch
    import lyra_amd.codec as codec
    ctx, twin, enc = _ctx(), _ctx(), _ctx()
    dev = torch.device("cuda", 0)
    F, rate, bits, nb = 60, 48000, 184, 23
    lanes = np.arange(1, 9, dtype=np.int32)
    pk = _packets(enc, golden_dir, F + 4, bits, 8)
    rx = _bursts(F + 4, (2, 2), (10, 9), (30, 3), (50, 12))
    for c in (ctx, twin):   # slots that are not the reset state, a burst in progress
        _twin_decode(c, {0: pk[:4]}, {0: rx[:4]}, rate, bits)
    pk, rx = pk[4:], rx[4:]
    before = ctx.export_streams(np.arange(0, 9))
    d_pk = torch.from_numpy(pk).to(dev)
    d_16, d_ext = _filled(dev, F, 320, np.int16), _filled(dev, F, 960, np.int16)
    d_n, d_cn = _filled(dev, F, 1, np.int32).view(-1), _filled(dev, F, 1, np.int32).view(-1)
    d_odd = _filled(dev, F + 1, 320, np.int16).view(-1)[1:1 + F * 320].view(F, 320)   # 2 bytes off a 16-byte boundary
    assert d_odd.data_ptr() % 16 == 2
    pb = np.where(rx, nb, 0).astype(np.int32)
    wrong = pb.copy(); wrong[7] = 15
    ok = [(0, 0, F)]
    # a size of another bitrate | a negative size | no sizes | bad rate | bad bit counts | overlapping spans | a lane that is
    # also a span id | an id outside the context | misaligned or missing 16 kHz buffer | no external-rate buffer at 48 kHz
    cases = [dict(pb=wrong), dict(pb=-pb), dict(pb=None), dict(rate=44100), dict(bits=186), dict(bits=0),
             dict(spans=[(0, 0, F), (9, 10, 5)]), dict(lanes=[0, 1]), dict(spans=[(MAX_STREAMS, 0, F)]), dict(d_16=d_odd),
             dict(d_16=None), dict(d_ext=None)]
    for case in cases:
        sp = codec._spans(case.get("spans", ok))
        ln = np.asarray(case.get("lanes", lanes), np.int32)
        p = case.get("pb", pb)
        t16, text = case.get("d_16", d_16), case.get("d_ext", d_ext)
        rc = ctx.L.lyra_hip_decode_spans_lossy_dev(ctx.h, sp.ctypes.data, sp.size, ln.ctypes.data, ln.size, d_pk.data_ptr(),
                                                   p.ctypes.data if p is not None else None, case.get("bits", bits),
                                                   case.get("rate", rate), t16.data_ptr() if t16 is not None else None,
                                                   text.data_ptr() if text is not None else None, d_n.data_ptr(), d_cn.data_ptr())
        assert rc == -1, (list(case), rc)   # LYRA_HIP_EINVAL
    ctx.synchronize()
    assert np.array_equal(ctx.export_streams(np.arange(0, 9)), before)
    for t in (d_16, d_ext, d_n, d_cn, d_odd):
        assert (t.cpu().numpy().view(np.uint8) == FILL).all()
    want_16, want_ext, want_n, want_cn, _ = _twin_decode(twin, {0: pk}, {0: rx}, rate, bits)
    ctx.decode_spans_lossy_dev(ok, d_pk, pb, bits, d_16, lanes, sample_rate_hz=rate, d_pcm_ext=d_ext, d_is_noise=d_n,
                               d_is_comfort_noise=d_cn)
    ctx.synchronize()
    assert np.array_equal(d_16.cpu().numpy(), want_16[0]) and np.array_equal(d_ext.cpu().numpy(), want_ext[0])
    assert np.array_equal(d_n.cpu().numpy(), want_n[0]) and np.array_equal(d_cn.cpu().numpy(), want_cn[0])
    _check_state("after the refusals", ctx, twin, [0], lanes)


def test_host_form_without_the_optional_outputs_and_in_serial_order(golden_dir):
    """The C host form with is_noise and is_comfort_noise NULL at 16 kHz, on a context in strict call order."""
    import lyra_amd.codec as codec
    ctx, twin, enc = _ctx(), _ctx(), _ctx()
    ctx.set_serial(True)
    n, bits, nb = 90, 64, 8
    lanes = np.arange(40, 48, dtype=np.int32)
    pk = _packets(enc, golden_dir, n, bits, 77)
    rx = _bursts(n, (20, 10), (45, 2), (70, 14))
    want_16 = _twin_decode(twin, {2: pk}, {2: rx}, 16000, bits)[0]
    sp = codec._spans([(2, 0, n)])
    pb = np.where(rx, nb, 0).astype(np.int32)
    out = np.zeros((n, 320), np.int16)
    rc = ctx.L.lyra_hip_decode_spans_lossy(ctx.h, sp.ctypes.data, sp.size, lanes.ctypes.data, lanes.size, pk.ctypes.data,
                                           pb.ctypes.data, bits, 16000, out.ctypes.data, None, None, None)
    assert rc == 0, ctx.last_error()
    assert np.array_equal(out, want_16[2])
    _check_state("host form", ctx, twin, [2], lanes)


@pytest.mark.parametrize("rate,decode_rate", [(16000, 16000), (48000, 8000)])
def test_file_demo_decodes_its_own_dtx_encode_time_parallel_as_hop_by_hop(golden_dir, tmp_path, rate, decode_rate):
    """8 s of the half-silent recording through file_demo --dtx --time-parallel: DecodeFeaturesTimeParallel with the packet
    sizes (lyra_hip_decode_spans_lossy) and DecodeFeaturesBatch with them (BatchLyraDecoder hop by hop) give the same samples;
    the trace has empty packets and packets."""
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "file_demo")
    assert os.path.exists(demo), "lyra_amd/file_demo not built (__graft_entry__.build())"
    hops = 400
    pcm = _speech(golden_dir, hops, 77, half_silent=True)
    if rate != 16000:   # the same samples read as a signal at `rate`
        pcm = np.ascontiguousarray(np.tile(pcm.reshape(-1), rate // 16000)[:hops * (rate // 50)])
    wav = str(tmp_path / "talk.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(pcm.tobytes())
    r = subprocess.run([demo, "--time-parallel=64", "--dtx", "--decode-rate=%d" % decode_rate, lyra_amd.default_model_dir(), "6000",
                        str(tmp_path), wav], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("dtx round trip:")]
    assert line and line[0].endswith("decode equal"), r.stdout[-500:]
    n_hops, n_empty = int(line[0].split()[3]), int(line[0].split()[5])
    assert n_hops == hops and 60 <= n_empty <= hops - 60, line[0]
