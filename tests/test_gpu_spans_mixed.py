"""The span calls with a bitrate per frame on the GPU (include/lyra_hip_spans_mixed.h): lyra_hip_encode_spans_mixed[_dev] and
lyra_hip_decode_spans_lossy_mixed[_dev].  Every comparison is BIT FOR BIT against the hop-by-hop mixed calls --
lyra_hip_encode_mixed_dev, lyra_hip_decode_lossy_mixed_dev -- on a twin context with the same stream ids and comfort-noise seed:
packet rows up to their size, the filler behind them, packet_bytes, the PCM and flags of the decoder, the filler outside the
spans, the span streams' exported blobs and the lanes' against the twin's untouched lanes.

The bit schedules and size schedules are drawn per frame and then adjusted on the call's plan, so that what they have to
exercise holds by construction; it is asserted before anything is compared (_assert_encode_schedule, _assert_size_changes)."""
import os
import subprocess
import wave

import numpy as np
import pytest

from gpu_plumbing import FILL, _filled, make_ctx
from signals import _audio_dtx as _audio, _bursts, _plain, _speech_hops as _speech, _stretches
from span_cases import (BITS, ROW, _by_frame, _check_packets, _check_rows, _check_state, _decode_schedule, _dirty_lane,
                        _draw_sizes, _encode_plan, _layout, _other, _packets, _rows_of, _twin_decode_mixed as _twin_decode,
                        _twin_encode_rows as _twin_encode)

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MAX_STREAMS = 96
SEED = 0x5EEDC0DE
EINVAL = -1


def _ctx(mode="xnnpack", rate=16000):
    return make_ctx(MAX_STREAMS, mode, rate, SEED)


# ---- encode -------------------------------------------------------------------------------------------------------------------
def _producing_rows(chunks, n_steps, W, frame_of):
    """per step: [(quantizer row, buffer frame)] of the rows that produce, as span_run_steps lays the batch out; frame_of: the
    plan's (compacted) frame index -> buffer frame"""
    steps_of = [int(c["n_warmup"]) + int(c["n_frames"]) for c in chunks]
    n_own = sum(1 for c in chunks if c["n_warmup"] == 0)
    out = []
    for i in range(n_steps):
        own = sum(1 for r in range(n_own) if steps_of[r] > i)
        lanes = sum(1 for r in range(n_own, len(chunks)) if steps_of[r] > i)
        B = n_own + lanes if lanes else own
        Bq = own if i < W else B
        out.append([(r, frame_of(int(chunks[r]["first_frame"]) - int(chunks[r]["n_warmup"]) + i)) for r in range(Bq)
                    if i < steps_of[r] and i >= chunks[r]["n_warmup"]])
    return out


def _encode_schedule(rng, F, chunks, n_steps, W, frame_map):
    """a bit count per frame, drawn from BITS, then adjusted on the plan: the facts _assert_encode_schedule asks for"""
    bits = rng.choice(BITS, F).astype(np.int32)
    fixed = set()
    lane = next(c for c in chunks if c["n_warmup"] > 0)   # a lane chunk's first frame differs from the frame in front of it
    f0, f1 = frame_map[int(lane["first_frame"]) - 1], frame_map[int(lane["first_frame"])]
    if bits[f0] == bits[f1]:
        bits[f1] = _other(bits[f1], BITS)
    fixed |= {f0, f1}
    rows = _producing_rows(chunks, n_steps, W, frame_map.__getitem__)
    tiles = ([f for r, f in step if r // 16 == t and f not in fixed] for step in rows[W:] for t in range(3))
    tile = next(t for t in tiles if len(t) >= 2)
    bits[tile[0]], bits[tile[1]] = 4, 184                  # a 4-bit and a 184-bit row in one 16-row tile
    fixed |= set(tile[:2])
    for step in rows:                                      # no step whose rows all share one count
        frames = [f for _, f in step]
        if len(frames) >= 2 and len(set(bits[frames].tolist())) < 2:
            f = next(f for f in frames if f not in fixed)
            bits[f] = _other(bits[f], BITS)
    return bits


def _assert_encode_schedule(where, bits, chunks, n_steps, W, frame_map):
    rows = _producing_rows(chunks, n_steps, W, frame_map.__getitem__)
    lanes = [c for c in chunks if c["n_warmup"] > 0]
    assert any(bits[frame_map[int(c["first_frame"])]] != bits[frame_map[int(c["first_frame"]) - 1]] for c in lanes), \
        (where, "no lane chunk starts on a bitrate switch")
    tiles = [{int(bits[f]) for r, f in step if r // 16 == t} for step in rows for t in range(3)]
    assert any({4, 184} <= t for t in tiles), (where, "no tile holds a 4-bit and a 184-bit row")
    assert all(step for step in rows), (where, "a step produces nothing")
    assert all(len({int(bits[f]) for _, f in step}) >= 2 for step in rows), (where, "a step's rows share one bit count")


ENCODE_CASES = [(16000, False, "xnnpack"), (48000, True, "xnnpack"), (8000, False, "builtin_mixed")]


@pytest.mark.parametrize("rate,dtx,mode", ENCODE_CASES)
def test_one_encode_call_of_mixed_span_lengths_equals_hop_by_hop(golden_dir, rate, dtx, mode):
    """Span lengths 350, 1, 0, 26, W + 18 and 7 in one call with 40 lanes, two pairs of spans touching, a bit count per frame
    from {4, 8, 12, 64, 100, 120, 180, 184}.  Without DTX the plan has 42 rows and 34 steps: three quantizer tiles, the last
    partial.  With DTX the steps run on the compacted frames, and the 350-frame span is the half-silent input."""
    import torch
    import lyra_amd.codec as codec
    W = codec.span_warmup_frames("encoder")
    ctx, twin, probe = _ctx(mode, rate), _ctx(mode, rate), _ctx(mode, rate)
    dev = torch.device("cuda", 0)
    lanes = np.arange(24, 24 + 40, dtype=np.int32)
    lengths = {7: 350, 11: 1, 3: 0, 20: 26, 5: W + 18, 9: 7}
    gaps = [2, 0, 3, 3, 0, 1]
    # the long span: speech, digital silence and low noise in turns; the others plain speech, so that with DTX too every step
    # has at least two rows that produce
    ext = {i: _audio(golden_dir, n, rate, 200 + i) if i == 7 else _plain(golden_dir, n, rate, 200 + i) for i, n in lengths.items()}
    spans, buf = _layout(ext, gaps)
    F = len(buf)
    where = f"{mode}/{rate}/dtx={dtx}"
    active = {i: np.ones(n, bool) for i, n in lengths.items()}
    if dtx:   # the decisions do not depend on the bit counts: a uniform DTX call on a third context gives them
        sizes = probe.encode_spans_dtx(spans, buf, 64, lanes, sample_rate_hz=rate)[1]
        active = {i: sizes[first:first + n] > 0 for (i, first, n) in spans}
        assert 60 <= active[7].sum() <= 290 and max(b - a for a, b in _stretches(~active[7])) >= 8, (where, "the DTX trace")
    chunks, n_steps, frame_map, _ = _encode_plan(spans, active, lanes)
    if not dtx:
        assert (len(chunks), n_steps) == (42, 34), (len(chunks), n_steps)
    bits = _encode_schedule(np.random.default_rng(rate + 7), F, chunks, n_steps, W, frame_map)
    _assert_encode_schedule(where, bits, chunks, n_steps, W, frame_map)
    outside = np.ones(F, bool)
    for (i, first, n) in spans:
        outside[first:first + n] = False
    bits[outside] = 85   # frames outside the spans hold no bit count at all
    want_pk, want_nb = _twin_encode(twin, ext, {i: bits[first:first + n] for (i, first, n) in spans}, rate, dtx)
    if dtx:
        assert all(np.array_equal(want_nb[i] > 0, active[i]) for i in lengths), (where, "DTX decisions")
    assert all(np.array_equal(want_nb[i][want_nb[i] > 0], (bits[first:first + n][want_nb[i] > 0] + 7) // 8)
               for (i, first, n) in spans)
    d_ext, d_p16 = torch.from_numpy(buf).to(dev), _filled(dev, F, 320, np.int16)
    d_pk, d_nb = _filled(dev, F, ROW, np.uint8), _filled(dev, F, 1, np.int32).view(-1)
    ctx.encode_spans_mixed_dev(spans, d_ext, bits, d_pk, d_nb, lanes, sample_rate_hz=rate,
                               d_pcm16=d_p16 if rate != 16000 else None, dtx=dtx)
    ctx.synchronize()
    _check_packets(where, d_pk.cpu().numpy(), d_nb.cpu().numpy(), spans, want_pk, want_nb)
    assert np.array_equal(d_ext.cpu().numpy(), buf), f"{where}: the input buffer was written"
    if rate == 16000:
        assert (d_p16.cpu().numpy().view(np.uint8) == FILL).all()
    _check_state(where, ctx, twin, list(lengths), lanes)
    assert ctx.encode_mixed_errors() == 0, f"{where}: a row of a step carried an invalid bit count"


# ---- decode -------------------------------------------------------------------------------------------------------------------
_prefix_checked = []


def _assert_prefixes(enc, golden_dir):
    """the quantizer is greedy: the 64- and 120-bit packets of a hop are the first 8 and 15 bytes of its 184-bit packet"""
    if _prefix_checked:
        return
    full = _packets(enc, golden_dir, 30, 184, 31)
    for bits, nb in ((64, 8), (120, 15)):
        assert np.array_equal(_packets(enc, golden_dir, 30, bits, 31), full[:, :nb]), f"{bits}-bit packets are no prefix"
    _prefix_checked.append(True)


DECODE_CASES = [(16000, "xnnpack"), (48000, "xnnpack"), (32000, "builtin_mixed")]


@pytest.mark.parametrize("rate,mode", DECODE_CASES)
def test_one_lossy_decode_call_of_mixed_span_lengths_equals_hop_by_hop(golden_dir, rate, mode):
    """The span layout of the encode test through decode_spans_lossy_mixed_dev: the loss trace of test_gpu_spans_lossy.py on the
    350-frame span, every received packet at 8, 15 or 23 bytes."""
    import torch
    import lyra_amd.codec as codec
    W = codec.span_warmup_frames("decoder")
    ctx, twin, enc = _ctx(mode), _ctx(mode), _ctx(mode)
    _assert_prefixes(enc, golden_dir)
    dev = torch.device("cuda", 0)
    hop = rate // 50
    lanes = np.arange(24, 24 + 40, dtype=np.int32)
    lengths = {7: 350, 11: 1, 3: 0, 20: 26, 5: W + 18, 9: 7}
    gaps = [2, 0, 3, 3, 0, 1]
    rx = {11: np.zeros(1, bool), 3: np.zeros(0, bool), 20: np.zeros(26, bool),
          5: _bursts(W + 18, (0, 5), (12, 1), (20, 6), (W + 9, 9)), 9: np.ones(7, bool)}
    pk184 = {i: _packets(enc, golden_dir, n, 184, 300 + i) for i, n in lengths.items()}
    spans, _ = _layout(pk184, gaps)
    F = spans[-1][1] + spans[-1][2] + 2
    where = f"{mode}/{rate}"
    pb = _decode_schedule(where, np.random.default_rng(rate + 3), spans, rx, lanes, F, W)
    pb_all = _by_frame(spans, pb, F)
    rows = {i: _rows_of(pk184[i], pb[i]) for i in lengths}
    spans2, buf = _layout(rows, gaps)
    assert spans2 == spans and len(buf) == F
    _dirty_lane((ctx, twin), int(lanes[3]), golden_dir)
    want_16, want_ext, want_n, want_cn = _twin_decode(twin, rows, pb, rate)
    assert want_cn[7].any() and not want_cn[7].all()
    d_pk = torch.from_numpy(buf).to(dev)
    d_16, d_ext = _filled(dev, F, 320, np.int16), _filled(dev, F, hop, np.int16)
    d_n, d_cn = _filled(dev, F, 1, np.int32).view(-1), _filled(dev, F, 1, np.int32).view(-1)
    ctx.decode_spans_lossy_mixed_dev(spans, d_pk, pb_all, d_16, lanes, sample_rate_hz=rate,
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
    assert ctx.decode_lossy_errors() == 0


# ---- continuation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_lanes", [40, 0])
def test_decode_span_continues_a_live_stream_mid_burst_and_is_continued(golden_dir, n_lanes):
    """5 ticks hop by hop (three packets of 8 bytes, then a burst), a span of 200 that begins inside that burst and whose first
    packet has another size, 10 more ticks hop by hop: all three pieces and the final blob equal the twin that went hop by hop
    throughout.  n_lanes = 0: sequential."""
    ctx, twin, enc = _ctx(), _ctx(), _ctx()
    sid, k, n, tail, rate = 13, 5, 200, 10, 32000
    lanes = np.arange(30, 30 + n_lanes, dtype=np.int32)
    pk184 = _packets(enc, golden_dir, k + n + tail, 184, 55)
    rx = _bursts(k + n + tail, (3, 6), (40, 1), (70, 11), (120, 4), (150, 30), (k + n - 3, 5))
    pb = _draw_sizes(np.random.default_rng(9), rx)
    pb[:3] = 8
    in_span = k + int(np.flatnonzero(rx[k:])[0])
    pb[in_span] = 23
    assert not rx[k] and pb[in_span] != pb[:k][pb[:k] > 0][-1], "the span starts mid-burst, its first packet on a switch"
    rows = _rows_of(pk184, pb)
    want = _twin_decode(twin, {sid: rows}, {sid: pb}, rate)
    head = _twin_decode(ctx, {sid: rows[:k]}, {sid: pb[:k]}, rate)
    mid = ctx.decode_spans_lossy_mixed([(sid, k, n)], rows, pb, lanes, sample_rate_hz=rate)
    for a in mid:
        assert not a[:k].any() and not a[k + n:].any()
    rest = _twin_decode(ctx, {sid: rows[k + n:]}, {sid: pb[k + n:]}, rate)
    for name, w, h, m, r in zip(("pcm16", "pcm_ext", "is_noise", "is_comfort_noise"), want, head, mid, rest):
        got = np.concatenate([h[sid], m[k:k + n], r[sid]])
        diff = np.flatnonzero((got.reshape(len(got), -1) != w[sid].reshape(len(got), -1)).any(axis=1))
        assert len(diff) == 0, (name, list(diff[:8]), len(diff))
    assert want[3][sid][k:k + n].any() and not want[3][sid][k:k + n].all()
    _check_state("continued stream", ctx, twin, [sid], lanes)


@pytest.mark.parametrize("n_lanes", [40, 0])
@pytest.mark.parametrize("middle", ["mixed", "uniform"])
def test_encode_span_continues_a_live_stream_and_is_continued(golden_dir, n_lanes, middle):
    """5 hops hop by hop, a span of 200 with a bitrate switch on its first frame, 10 hops hop by hop.  middle "uniform": the
    span goes through encode_spans at 120 bits -- a stream may move between the uniform and the mixed span call."""
    ctx, twin = _ctx(), _ctx()
    sid, k, n, tail, rate = 13, 5, 200, 10, 16000
    lanes = np.arange(30, 30 + n_lanes, dtype=np.int32)
    x = _speech(golden_dir, k + n + tail, 66)
    bits = np.random.default_rng(10).choice(BITS, k + n + tail).astype(np.int32)
    if middle == "uniform":
        bits[k:k + n] = 120
    bits[k - 1] = 64
    bits[k] = 120
    want_pk, want_nb = _twin_encode(twin, {sid: x}, {sid: bits}, rate)
    head_pk, head_nb = _twin_encode(ctx, {sid: x[:k]}, {sid: bits[:k]}, rate)
    if middle == "mixed":
        mid_pk, mid_nb = ctx.encode_spans_mixed([(sid, k, n)], x, bits, lanes, sample_rate_hz=rate)
        assert not mid_pk[:k].any() and not mid_pk[k + n:].any() and not mid_nb[:k].any() and not mid_nb[k + n:].any()
        mid_pk, mid_nb = mid_pk[k:k + n], mid_nb[k:k + n]
    else:
        mid_pk, mid_nb = ctx.encode_spans([(sid, k, n)], x, 120, lanes)[k:k + n], np.full(n, 15, np.int32)
    rest_pk, rest_nb = _twin_encode(ctx, {sid: x[k + n:]}, {sid: bits[k + n:]}, rate)
    assert np.array_equal(np.concatenate([head_nb[sid], mid_nb, rest_nb[sid]]), want_nb[sid])
    for name, got, at in (("head", head_pk[sid], 0), ("span", mid_pk, k), ("tail", rest_pk[sid], k + n)):
        for h, row in enumerate(got):
            size = want_nb[sid][at + h]
            assert np.array_equal(row[:size], want_pk[sid][at + h][:size]), (middle, name, h)
    _check_state(f"continued stream ({middle})", ctx, twin, [sid], lanes)
    assert ctx.encode_mixed_errors() == 0


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(golden_dir):
    """LYRA_HIP_EINVAL before the first kernel on either side: no slot, no buffer changes; a bad value on a frame outside every
    span is not looked at; the valid call that follows equals the twin."""
    import torch
    import lyra_amd.codec as codec
    rate, hop = 48000, 960
    ctx, twin, enc = _ctx(rate=16000), _ctx(rate=16000), _ctx()   # (the estimator is set for 16 kHz: DTX at 48 kHz is refused)
    dev = torch.device("cuda", 0)
    n, F = 60, 64
    ok = [(0, 2, n)]
    lanes = np.arange(1, 9, dtype=np.int32)
    # streams that are not in the reset state, a burst in progress on the decode side
    x = _audio(golden_dir, 4 + n, rate, 77)
    rng = np.random.default_rng(5)
    bits = rng.choice(BITS, 4 + n).astype(np.int32)
    pk184 = _packets(enc, golden_dir, 4 + n, 184, 8)
    rx = _bursts(4 + n, (2, 4), (14, 9), (34, 3), (54, 12))
    pb = _draw_sizes(rng, rx)
    rows = _rows_of(pk184, pb)
    for c in (ctx, twin):
        _twin_encode(c, {0: x[:4]}, {0: bits[:4]}, rate)
        _twin_decode(c, {0: rows[:4]}, {0: pb[:4]}, rate)
    x, bits, rows, pb = x[4:], bits[4:], rows[4:], pb[4:]
    before = ctx.export_streams(np.arange(0, 9))
    def framed(v, fill):   # two filler frames in front, two behind
        out = np.full((F,) + v.shape[1:], fill, v.dtype)
        out[2:2 + n] = v
        return out
    bits_f, pb_f = framed(bits, 186), framed(pb, 16)   # values no frame of a span may hold: outside, nobody looks
    x_buf = framed(x, 21845)   # (0x5555: FILL bytes)
    d_x = torch.from_numpy(x_buf).to(dev)
    d_rows = torch.from_numpy(framed(rows, FILL)).to(dev)
    d_p16, d_pk, d_nb = _filled(dev, F, 320, np.int16), _filled(dev, F, ROW, np.uint8), _filled(dev, F, 1, np.int32).view(-1)
    d_16, d_ext = _filled(dev, F, 320, np.int16), _filled(dev, F, hop, np.int16)
    d_n, d_cn = _filled(dev, F, 1, np.int32).view(-1), _filled(dev, F, 1, np.int32).view(-1)
    d_odd = _filled(dev, F + 1, hop, np.int16).view(-1)[1:1 + F * hop].view(F, hop)   # 2 bytes off a 16-byte boundary
    d_odd16 = _filled(dev, F + 1, 320, np.int16).view(-1)[1:1 + F * 320].view(F, 320)
    assert d_odd.data_ptr() % 16 == 2 and d_odd16.data_ptr() % 16 == 2
    def with_at(v, at, value):
        out = v.copy()
        out[at] = value
        return out
    ptr = lambda t: t.data_ptr() if t is not None else None
    host = lambda a: a.ctypes.data if a is not None else None
    enc_cases = [dict(bits=with_at(bits_f, 9, b)) for b in (0, 2, 186, -4)] + \
                [dict(bits=None), dict(d_nb=None), dict(rate=44100), dict(spans=[(0, 2, n), (9, 10, 5)]), dict(lanes=[0, 1]),
                 dict(d_x=d_odd), dict(dtx=1)]
    for case in enc_cases:
        sp = codec._spans(case.get("spans", ok))
        ln = np.asarray(case.get("lanes", lanes), np.int32)
        rc = ctx.L.lyra_hip_encode_spans_mixed_dev(ctx.h, sp.ctypes.data, sp.size, ln.ctypes.data, ln.size,
                                                   ptr(case.get("d_x", d_x)), case.get("rate", rate), ptr(d_p16),
                                                   host(case.get("bits", bits_f)), case.get("dtx", 0), ptr(d_pk),
                                                   ptr(case.get("d_nb", d_nb)))
        assert rc == EINVAL, ("encode", list(case), rc)
    dec_cases = [dict(pb=with_at(pb_f, 9, 16)), dict(pb=None), dict(rate=44100), dict(spans=[(0, 2, n), (9, 10, 5)]),
                 dict(lanes=[0, 1]), dict(d_ext=d_odd), dict(d_16=d_odd16)]
    for case in dec_cases:
        sp = codec._spans(case.get("spans", ok))
        ln = np.asarray(case.get("lanes", lanes), np.int32)
        rc = ctx.L.lyra_hip_decode_spans_lossy_mixed_dev(ctx.h, sp.ctypes.data, sp.size, ln.ctypes.data, ln.size, ptr(d_rows),
                                                         host(case.get("pb", pb_f)), case.get("rate", rate),
                                                         ptr(case.get("d_16", d_16)), ptr(case.get("d_ext", d_ext)),
                                                         ptr(d_n), ptr(d_cn))
        assert rc == EINVAL, ("decode", list(case), rc)
    ctx.synchronize()
    assert np.array_equal(ctx.export_streams(np.arange(0, 9)), before)
    for t in (d_p16, d_pk, d_nb, d_16, d_ext, d_n, d_cn, d_odd, d_odd16):
        assert (t.cpu().numpy().view(np.uint8) == FILL).all()
    assert np.array_equal(d_x.cpu().numpy(), x_buf)
    # the valid calls: bits_f and pb_f hold 186 and 16 on the frames outside the span
    want_pk, want_nb = _twin_encode(twin, {0: x}, {0: bits}, rate)
    want_16, want_ext, want_n, want_cn = _twin_decode(twin, {0: rows}, {0: pb}, rate)
    ctx.encode_spans_mixed_dev(ok, d_x, bits_f, d_pk, d_nb, lanes, sample_rate_hz=rate, d_pcm16=d_p16)
    ctx.decode_spans_lossy_mixed_dev(ok, d_rows, pb_f, d_16, lanes, sample_rate_hz=rate, d_pcm_ext=d_ext, d_is_noise=d_n,
                                     d_is_comfort_noise=d_cn)
    ctx.synchronize()
    _check_packets("after the refusals", d_pk.cpu().numpy(), d_nb.cpu().numpy(), ok, want_pk, want_nb)
    for name, t, w in (("pcm16", d_16, want_16), ("pcm_ext", d_ext, want_ext)):
        _check_rows("after the refusals " + name, t.cpu().numpy(), ok, w)
    for name, t, w in (("is_noise", d_n, want_n), ("is_comfort_noise", d_cn, want_cn)):
        _check_rows("after the refusals " + name, t.cpu().numpy().reshape(F, 1), ok, w)
    _check_state("after the refusals", ctx, twin, [0], lanes)
    assert ctx.encode_mixed_errors() == 0 and ctx.decode_lossy_errors() == 0


# ---- host forms ---------------------------------------------------------------------------------------------------------------
def test_host_forms_without_the_optional_outputs_and_in_serial_order(golden_dir):
    """The C host forms on a context in strict call order: encode with DTX (bytes behind a packet and the rows of noise frames
    read back as zero), lossy decode with is_noise and is_comfort_noise NULL."""
    import lyra_amd.codec as codec
    ctx, twin, enc = _ctx(), _ctx(), _ctx()
    ctx.set_serial(True)
    n = 90
    lanes = np.arange(40, 48, dtype=np.int32)
    sp = codec._spans([(2, 1, n)])
    rng = np.random.default_rng(14)
    # encode: frame 0 and the frame behind the span are filler
    x = _audio(golden_dir, n, 16000, 33)
    bits = rng.choice(BITS, n).astype(np.int32)
    want_pk, want_nb = _twin_encode(twin, {2: x}, {2: bits}, 16000, dtx=True)
    assert 5 <= (want_nb[2] == 0).sum() <= n - 10, "the input has noise frames and packets"
    x_f = np.concatenate([np.full((1, 320), 21845, np.int16), x, np.full((1, 320), 21845, np.int16)])
    bits_f = np.concatenate([[85], bits, [85]]).astype(np.int32)
    pk, nb = np.full((n + 2, ROW), FILL, np.uint8), np.full(n + 2, 0x55555555, np.int32)
    rc = ctx.L.lyra_hip_encode_spans_mixed(ctx.h, sp.ctypes.data, sp.size, lanes.ctypes.data, lanes.size, x_f.ctypes.data, 16000,
                                           bits_f.ctypes.data, 1, pk.ctypes.data, nb.ctypes.data)
    assert rc == 0, ctx.last_error()
    assert np.array_equal(nb[1:1 + n], want_nb[2]) and (nb[[0, -1]] == 0x55555555).all() and (pk[[0, -1]] == FILL).all()
    for h in range(n):
        size = want_nb[2][h]
        assert np.array_equal(pk[1 + h, :size], want_pk[2][h][:size]), h
        assert not pk[1 + h, size:].any(), (h, "bytes behind the packet do not read back as zero")
    assert ctx.encode_mixed_errors() == 0
    # decode
    pk184 = _packets(enc, golden_dir, n, 184, 77)
    rx = _bursts(n, (20, 10), (45, 2), (70, 14))
    pb = _draw_sizes(rng, rx)
    rows = _rows_of(pk184, pb)
    want_16 = _twin_decode(twin, {2: rows}, {2: pb}, 16000)[0]
    rows_f = np.concatenate([np.full((1, ROW), FILL, np.uint8), rows, np.full((1, ROW), FILL, np.uint8)])
    pb_f = np.concatenate([[85], pb, [85]]).astype(np.int32)
    out = np.full((n + 2, 320), 21845, np.int16)
    rc = ctx.L.lyra_hip_decode_spans_lossy_mixed(ctx.h, sp.ctypes.data, sp.size, lanes.ctypes.data, lanes.size, rows_f.ctypes.data,
                                                 pb_f.ctypes.data, 16000, out.ctypes.data, None, None, None)
    assert rc == 0, ctx.last_error()
    assert np.array_equal(out[1:1 + n], want_16[2]) and (out[[0, -1]] == 21845).all()
    _check_state("host forms", ctx, twin, [2], lanes)


# ---- file_demo ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,decode_rate", [(16000, 16000), (48000, 8000)])
def test_file_demo_bitrate_schedule_time_parallel_equals_hop_by_hop(golden_dir, tmp_path, rate, decode_rate):
    """400 hops of golden speech through file_demo --time-parallel=64 --bitrate-schedule=25: the schedule 3200 -> 6000 -> 9200
    every 25 hops, encoded and decoded time-parallel and hop by hop (BatchLyraEncoder with set_bitrate, BatchLyraDecoder with
    each hop's size), gives the same packets and the same samples."""
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "file_demo")
    assert os.path.exists(demo), "lyra_amd/file_demo not built (__graft_entry__.build())"
    hops = 400
    pcm = _speech(golden_dir, hops, 78)
    if rate != 16000:   # the same samples read as a signal at `rate`
        pcm = np.ascontiguousarray(np.tile(pcm.reshape(-1), rate // 16000)[:hops * (rate // 50)])
    wav = str(tmp_path / "talk.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(pcm.tobytes())
    r = subprocess.run([demo, "--time-parallel=64", "--bitrate-schedule=25", "--decode-rate=%d" % decode_rate,
                        lyra_amd.default_model_dir(), "6000", str(tmp_path), wav], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    line = [l for l in r.stdout.splitlines() if l.startswith("mixed round trip:")]
    assert line and line[0].endswith("encode equal decode equal"), r.stdout[-500:]
    words = line[0].split()
    assert int(words[3]) == hops, line[0]
    per_size = [int(words[words.index(k) + 1]) for k in ("x8", "x15", "x23")]
    assert all(c >= hops // 4 for c in per_size) and sum(per_size) == hops, line[0]   # the schedule reached all three bitrates
