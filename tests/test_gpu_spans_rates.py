"""The span calls with a sample rate per span on the GPU (include/lyra_hip_spans_rates.h): lyra_hip_encode_spans_rates[_dev],
lyra_hip_decode_spans_lossy_rates[_dev] and lyra_hip_decode_spans_rates[_dev].  Every comparison is BIT FOR BIT against the
hop-by-hop calls on a twin context with the same stream ids and comfort-noise seed -- lyra_hip_encode_rates_dev,
lyra_hip_decode_lossy_rates_dev, lyra_hip_decode + lyra_hip_resample(DECODER): packet rows up to their size and the filler behind
them, packet_bytes, the 16 kHz rows, the external-rate rows up to rate / 50 samples and the filler behind them, the flags, the
filler outside the spans, the span streams' exported blobs and the lanes' against the twin's untouched lanes.

External-rate rows are 960 samples apart.  What lies behind a row's rate / 50 samples is FILL in the span call's buffer and zero
in the twin's, so a call that read it would differ.  In the shared layout spans of different rates touch in the buffer: frame 0
of the second has to take its resampler history from its stream's slot, not from the 34 samples in front of it."""
import functools

import numpy as np
import pytest

from gpu_plumbing import FILL, _dev, _filled, make_ctx
from signals import _audio_dtx as _audio, _bursts, _pattern, _plain, _stretches
import span_cases
from span_cases import (BITS, EXT, FILL16, ROW, _by_frame, _check_packets, _check_rows, _check_state, _decode_schedule,
                        _dirty_lane, _draw_sizes, _encode_plan, _in_pos_offsets, _layout, _packets, _padded, _rows_of)

pytestmark = pytest.mark.gpu
MAX_STREAMS = 96
SEED = 0x5EEDC0DE
EINVAL = -1
# (stream id, frames, rate) in buffer order and the filler rows in front of each: lengths 0, 1, 3 and 5 leave a resampler
# workgroup (four frames) partly empty or cross its boundary, 60 / 61 / 140 run on lanes; 7|11, 20|5 and 9|13 touch in the
# buffer at different rates; all four rates; a 16 kHz span on lanes and a short one
LAYOUT = [(7, 140, 48000), (11, 1, 8000), (3, 0, 32000), (20, 60, 8000), (5, 5, 16000), (9, 3, 32000), (13, 61, 16000)]
GAPS = [2, 0, 3, 3, 0, 1, 0]
RATE_OF = {i: r for i, _, r in LAYOUT}
LANES = np.arange(24, 24 + 40, dtype=np.int32)
# what each stream has heard before its span: speech, then enough digital silence for the estimator to sit on it (7 hops: odd)
WARM = "SSZZZZZ"
SHORT = {0: "", 1: "Z", 3: "ZSZ", 5: "ZSZZZ"}  # short spans by hand: a noise frame and an active one wherever there are two


def _ctx(mode="xnnpack"):
    return make_ctx(MAX_STREAMS, mode, cng_seed=SEED)


def _span_audio(golden_dir, n, rate, seed):
    """[n][rate / 50]: half-silent audio for the long spans, the hand-made patterns for the short ones"""
    return _pattern(golden_dir, SHORT[n], rate, seed) if n in SHORT else _audio(golden_dir, n, rate, seed)


# ---- the twins and the check of the external-rate rows, at this layout's rates ------------------------------------------------
def _twin_encode(twin, aux, ext_by_id, bits_by_id, dtx=False):
    return span_cases._twin_encode_rows(twin, ext_by_id, bits_by_id, RATE_OF, dtx, aux)


_twin_decode = functools.partial(span_cases._twin_decode_rates, rate_of=RATE_OF)          # (twin, pk_by_id, pb_by_id)
_twin_decode_plain = functools.partial(span_cases._twin_decode_plain, rate_of=RATE_OF)    # (twin, pk_by_id, num_bits)
_check_ext = functools.partial(span_cases._check_ext, rate_of=RATE_OF)                    # (where, got, spans, want_by_id)


def _rates_of(spans):
    return np.array([RATE_OF[i] for (i, _, _) in spans], np.int32)


def _has_lane_chunks(chunks):
    return any(c["n_warmup"] > 0 for c in chunks)


# ---- 1: encode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtx,mode", [(False, "xnnpack"), (True, "xnnpack"), (True, "builtin_mixed")])
def test_one_encode_call_at_all_four_rates_equals_hop_by_hop(golden_dir, dtx, mode):
    """Seven spans at 48, 8, 32, 8, 16, 32 and 16 kHz in one call with 40 lanes, a bit count per frame, every stream live (seven
    hops hop by hop first).  With DTX every span of more than one frame has noise frames and active ones in the twin's result
    (a span of one frame cannot have both)."""
    import torch
    ctx, twin, aux = _ctx(mode), _ctx(mode), _ctx(mode)
    dev = _dev()
    where = f"{mode}/dtx={dtx}"
    rng = np.random.default_rng(17)
    warm = {i: _pattern(golden_dir, WARM, r, 500 + i) for i, _, r in LAYOUT}
    warm_bits = {i: rng.choice(BITS, len(WARM)) for i in warm}
    for c in (ctx, twin):
        _twin_encode(c, aux if c is twin else None, warm, warm_bits, dtx)
    ext = {i: _span_audio(golden_dir, n, r, 200 + i) for i, n, r in LAYOUT}
    spans, buf = _layout({i: _padded(v, FILL16) for i, v in ext.items()}, GAPS)
    F = len(buf)
    bits = rng.choice(BITS, F).astype(np.int32)
    outside = np.ones(F, bool)
    for (i, first, n) in spans:
        outside[first:first + n] = False
    bits[outside] = 85   # frames outside the spans hold no bit count at all
    want_pk, want_nb, want_16 = _twin_encode(twin, aux, ext, {i: bits[first:first + n] for (i, first, n) in spans}, dtx)
    active = {i: want_nb[i] > 0 for i in ext}
    if dtx:
        for i, n, _ in LAYOUT:
            assert n < 2 or (active[i].any() and not active[i].all()), (where, i, "no noise frame, or no active frame")
    else:
        assert all(a.all() for a in active.values())
    chunks, n_steps, _, _ = _encode_plan(spans, active, LANES)
    assert _has_lane_chunks(chunks), (where, "the plan has no lane chunks")
    d_ext, d_p16 = torch.from_numpy(buf).to(dev), _filled(dev, F, 320, np.int16)
    d_pk, d_nb = _filled(dev, F, ROW, np.uint8), _filled(dev, F, 1, np.int32).view(-1)
    ctx.encode_spans_rates_dev(spans, d_ext, _rates_of(spans), d_p16, bits, d_pk, d_nb, LANES, dtx=dtx)
    ctx.synchronize()
    _check_packets(where, d_pk.cpu().numpy(), d_nb.cpu().numpy(), spans, want_pk, want_nb)
    _check_rows(where + " pcm16", d_p16.cpu().numpy(), spans, want_16)
    assert np.array_equal(d_ext.cpu().numpy(), buf), f"{where}: the input buffer was written"
    _check_state(where, ctx, twin, [i for i, _, _ in LAYOUT], LANES)
    assert ctx.encode_mixed_errors() == 0 and ctx.rates_errors() == 0


# ---- 2: lossy decode --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["xnnpack", "builtin_mixed"])
def test_one_lossy_decode_call_at_all_four_rates_equals_hop_by_hop(golden_dir, mode):
    """The layout of the encode test with the 48 kHz span 350 frames long, which is what the loss trace of
    test_gpu_spans_lossy.py (_long_trace) and the size schedule of test_gpu_spans_mixed.py (_decode_schedule) are built for: bursts
    on both sides of the concealment limit, full comfort noise and the fade back, one inside a lane chunk's warm-up and one
    across a chunk boundary; every received packet at 8, 15 or 23 bytes.  The 61-frame 16 kHz span loses every packet."""
    import torch
    import lyra_amd.codec as codec
    W = codec.span_warmup_frames("decoder")
    ctx, twin, enc = _ctx(mode), _ctx(mode), _ctx(mode)
    dev = _dev()
    where = mode
    lengths = {i: 350 if i == 7 else n for i, n, _ in LAYOUT}
    rx = {11: np.zeros(1, bool), 3: np.zeros(0, bool), 20: _bursts(60, (0, 5), (12, 1), (20, 6), (38, 14)), 5: np.ones(5, bool),
          9: _bursts(3, (1, 1)), 13: np.zeros(61, bool)}
    pk184 = {i: _packets(enc, golden_dir, n, 184, 300 + i) for i, n in lengths.items()}
    spans, _ = _layout(pk184, GAPS)
    F = spans[-1][1] + spans[-1][2] + 2
    pb = _decode_schedule(where, np.random.default_rng(3), spans, rx, LANES, F, W)
    pb_all = _by_frame(spans, pb, F)
    rows = {i: _rows_of(pk184[i], pb[i]) for i in lengths}
    spans2, buf = _layout(rows, GAPS)
    assert spans2 == spans and len(buf) == F
    _dirty_lane((ctx, twin), int(LANES[3]), golden_dir)
    want_16, want_ext, want_n, want_cn = _twin_decode(twin, rows, pb)
    assert want_cn[7].any() and not want_cn[7].all() and want_cn[20].any() and not want_cn[20].all()
    assert any(b < 350 and pb[7][b] > 0 for _, b in _stretches(want_cn[7] != 0)), "no received tick behind comfort noise"
    d_pk = torch.from_numpy(buf).to(dev)
    d_16, d_ext = _filled(dev, F, 320, np.int16), _filled(dev, F, EXT, np.int16)
    d_n, d_cn = _filled(dev, F, 1, np.int32).view(-1), _filled(dev, F, 1, np.int32).view(-1)
    ctx.decode_spans_lossy_rates_dev(spans, d_pk, pb_all, _rates_of(spans), d_16, d_ext, LANES, d_is_noise=d_n,
                                     d_is_comfort_noise=d_cn)
    ctx.synchronize()
    _check_rows(where + " is_comfort_noise", d_cn.cpu().numpy().reshape(F, 1), spans, want_cn)
    _check_rows(where + " is_noise", d_n.cpu().numpy().reshape(F, 1), spans, want_n)
    _check_rows(where + " pcm16", d_16.cpu().numpy(), spans, want_16)
    _check_ext(where + " pcm_ext", d_ext.cpu().numpy(), spans, want_ext)
    assert np.array_equal(d_pk.cpu().numpy(), buf), f"{where}: the packet buffer was written"
    _check_state(where, ctx, twin, list(lengths), LANES)
    assert ctx.decode_lossy_errors() == 0 and ctx.rates_errors() == 0


# ---- 3: plain decode ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_bits", [64, 184])
def test_one_plain_decode_call_at_all_four_rates_equals_decode_plus_resample(golden_dir, num_bits):
    import torch
    import lyra_amd.codec as codec
    ctx, twin, enc = _ctx(), _ctx(), _ctx()
    dev = _dev()
    where = f"plain/{num_bits}"
    pk = {i: _packets(enc, golden_dir, n, num_bits, 400 + i) for i, n, _ in LAYOUT}
    spans, buf = _layout(pk, GAPS)
    F = len(buf)
    chunks, _ = codec.spans_plan("decoder", spans, LANES, MAX_STREAMS)
    assert _has_lane_chunks(chunks), (where, "the plan has no lane chunks")
    want_16, want_ext = _twin_decode_plain(twin, pk, num_bits)
    d_pk = torch.from_numpy(buf).to(dev)
    d_16, d_ext = _filled(dev, F, 320, np.int16), _filled(dev, F, EXT, np.int16)
    ctx.decode_spans_rates_dev(spans, d_pk, num_bits, _rates_of(spans), d_16, d_ext, LANES)
    ctx.synchronize()
    _check_rows(where + " pcm16", d_16.cpu().numpy(), spans, want_16)
    _check_ext(where + " pcm_ext", d_ext.cpu().numpy(), spans, want_ext)
    assert np.array_equal(d_pk.cpu().numpy(), buf), f"{where}: the packet buffer was written"
    _check_state(where, ctx, twin, [i for i, _, _ in LAYOUT], LANES)
    assert ctx.rates_errors() == 0


# ---- 4: continuation ------------------------------------------------------------------------------------------------------------
def _encode_rates(ctx, spans, ext, rates, bits, lanes):
    """encode_spans_rates_dev on zeroed device buffers, synchronised: packets [F][23], packet_bytes [F], pcm16 [F][320]"""
    import torch
    dev, F = _dev(), len(ext)
    d_pk, d_nb = torch.zeros((F, ROW), dtype=torch.uint8, device=dev), torch.zeros(F, dtype=torch.int32, device=dev)
    d_16 = torch.zeros((F, 320), dtype=torch.int16, device=dev)
    ctx.encode_spans_rates_dev(spans, torch.from_numpy(ext).to(dev), rates, d_16, bits, d_pk, d_nb, lanes)
    ctx.synchronize()
    return d_pk.cpu().numpy(), d_nb.cpu().numpy(), d_16.cpu().numpy()


def _decode_lossy_rates(ctx, spans, rows, pb, rates, lanes):
    """decode_spans_lossy_rates_dev on zeroed device buffers, synchronised: pcm16, pcm_ext [F][960], is_noise, is_cn"""
    import torch
    dev, F = _dev(), len(rows)
    d_16, d_ext = torch.zeros((F, 320), dtype=torch.int16, device=dev), torch.zeros((F, EXT), dtype=torch.int16, device=dev)
    d_n, d_cn = torch.zeros(F, dtype=torch.int32, device=dev), torch.zeros(F, dtype=torch.int32, device=dev)
    ctx.decode_spans_lossy_rates_dev(spans, torch.from_numpy(np.ascontiguousarray(rows)).to(dev), pb, rates, d_16, d_ext, lanes,
                                     d_is_noise=d_n, d_is_comfort_noise=d_cn)
    ctx.synchronize()
    return d_16.cpu().numpy(), d_ext.cpu().numpy(), d_n.cpu().numpy(), d_cn.cpu().numpy()


def _set_phase(contexts, sid, side, value):
    """a decimation phase no call sequence reaches but a blob may carry (test_gpu_spans_ext.py): RS_IN_POS of the side's slot"""
    off = _in_pos_offsets(contexts[0], 90)[0 if side == "encoder" else 1]
    blob = contexts[0].export_streams([sid])
    assert np.array_equal(blob, contexts[1].export_streams([sid]))
    blob[0, off] = value
    for c in contexts:
        c.import_streams([sid], blob)
    return off


@pytest.mark.parametrize("n_lanes", [40, 0])
def test_encode_span_continues_a_live_stream_with_a_decimation_phase_and_is_continued(golden_dir, n_lanes):
    """48 kHz: 7 hops hop by hop, RS_IN_POS set to 4 (phase 1 of 3), a rates span of 60 frames, a uniform span call of 40 frames
    at 48 kHz and 120 bits, 5 hops hop by hop: packets, the 16 kHz rows of the rates call and the blobs equal the twin that went
    hop by hop throughout."""
    ctx, twin, aux = _ctx(), _ctx(), _ctx()
    sid, k, n1, n2, tail = 7, 7, 60, 40, 5
    assert RATE_OF[sid] == 48000
    lanes = np.arange(30, 30 + n_lanes, dtype=np.int32)
    total = k + n1 + n2 + tail
    x = _plain(golden_dir, total, 48000, 66)
    bits = np.random.default_rng(10).choice(BITS, total).astype(np.int32)
    bits[k + n1:k + n1 + n2] = 120
    cut = lambda d, a, b: {sid: d[a:b]}
    head = _twin_encode(ctx, None, cut(x, 0, k), cut(bits, 0, k))
    want_head = _twin_encode(twin, aux, cut(x, 0, k), cut(bits, 0, k))
    off = _set_phase((ctx, twin), sid, "encoder", 4)
    aux.import_streams([sid], twin.export_streams([sid]))
    want = _twin_encode(twin, aux, cut(x, k, total), cut(bits, k, total))
    mid_pk, mid_nb, mid_16 = _encode_rates(ctx, [(sid, k, n1)], _padded(x[:k + n1], FILL16), [48000], bits[:k + n1], lanes)
    assert not mid_pk[:k].any() and not mid_nb[:k].any() and not mid_16[:k].any()
    uni = ctx.encode_spans([(sid, 0, n2)], x[k + n1:k + n1 + n2], 120, lanes, sample_rate_hz=48000)
    rest = _twin_encode(ctx, None, cut(x, k + n1 + n2, total), cut(bits, k + n1 + n2, total))
    got_nb = np.concatenate([mid_nb[k:], np.full(n2, 15, np.int32), rest[1][sid]])
    assert np.array_equal(got_nb, want[1][sid])
    got_pk = np.concatenate([mid_pk[k:], np.pad(uni, ((0, 0), (0, ROW - 15))), rest[0][sid]])
    for h, row in enumerate(got_pk):
        assert np.array_equal(row[:got_nb[h]], want[0][sid][h][:got_nb[h]]), (h, "packet")
    assert np.array_equal(head[0][sid], want_head[0][sid])
    assert np.array_equal(mid_16[k:], want[2][sid][:n1]), "the 16 kHz rows of the rates call"
    _check_state("continued encode", ctx, twin, [sid], lanes)
    assert ctx.export_streams([sid])[0, off] == (4 + (n1 + n2 + tail) * 960) % 6


@pytest.mark.parametrize("n_lanes", [40, 0])
def test_decode_span_continues_a_live_stream_mid_burst_with_a_decimation_phase_and_is_continued(golden_dir, n_lanes):
    """8 kHz: 5 ticks hop by hop that end inside a burst, RS_IN_POS set to 3 (phase 1 of 2), a rates span of 60 ticks that ends
    inside another burst, a uniform lossy span call of 40 ticks at 8 kHz, 5 ticks hop by hop."""
    ctx, twin, enc = _ctx(), _ctx(), _ctx()
    sid, k, n1, n2, tail = 20, 5, 60, 40, 5
    assert RATE_OF[sid] == 8000
    lanes = np.arange(30, 30 + n_lanes, dtype=np.int32)
    total = k + n1 + n2 + tail
    pk184 = _packets(enc, golden_dir, total, 184, 55)
    rx = _bursts(total, (3, 6), (30, 12), (k + n1 - 2, 5), (k + n1 + 20, 3))
    assert not rx[k] and not rx[k + n1], "both span calls start mid-burst"
    pb = _draw_sizes(np.random.default_rng(9), rx)
    pb[k + n1:k + n1 + n2] = np.where(rx[k + n1:k + n1 + n2], ROW, 0)
    rows = _rows_of(pk184, pb)
    cut = lambda d, a, b: {sid: d[a:b]}
    head = _twin_decode(ctx, cut(rows, 0, k), cut(pb, 0, k))
    want_head = _twin_decode(twin, cut(rows, 0, k), cut(pb, 0, k))
    off = _set_phase((ctx, twin), sid, "decoder", 3)
    want = _twin_decode(twin, cut(rows, k, total), cut(pb, k, total))
    mid = _decode_lossy_rates(ctx, [(sid, k, n1)], rows[:k + n1], pb[:k + n1], [8000], lanes)
    for a in mid:
        assert not a[:k].any()
    assert not mid[1][k:, 160:].any(), "samples behind the 8 kHz hop were written"
    uni = ctx.decode_spans_lossy([(sid, 0, n2)], rows[k + n1:k + n1 + n2], pb[k + n1:k + n1 + n2], 184, lanes, sample_rate_hz=8000)
    rest = _twin_decode(ctx, cut(rows, k + n1 + n2, total), cut(pb, k + n1 + n2, total))
    for q, name in enumerate(("pcm16", "pcm_ext", "is_noise", "is_comfort_noise")):
        m = mid[q][k:, :160] if q == 1 else mid[q][k:]
        got = np.concatenate([m, uni[q], rest[q][sid]])
        diff = np.flatnonzero((got.reshape(len(got), -1) != want[q][sid].reshape(len(got), -1)).any(axis=1))
        assert len(diff) == 0, (name, list(diff[:8]), len(diff))
        assert np.array_equal(head[q][sid], want_head[q][sid]), name
    assert want[3][sid][:n1].any() and not want[3][sid][:n1].all(), "the rates span has comfort noise and generated hops"
    _check_state("continued decode", ctx, twin, [sid], lanes)
    assert ctx.export_streams([sid])[0, off] == (3 + (n1 + n2 + tail) * 320) % 6


# ---- 5: all spans at 16000 ------------------------------------------------------------------------------------------------------
def test_all_spans_at_16000_equal_the_mixed_span_calls(golden_dir):
    """Outputs and blobs equal encode_spans_mixed_dev (with DTX) / decode_spans_lossy_mixed_dev at 16000, the pcm_ext rows carry
    the copy, and the resampler slots -- dirtied first, alike on both -- are what they were."""
    import torch
    ctx, twin, enc = _ctx(), _ctx(), _ctx()
    dev = _dev()
    lanes = np.arange(40, 60, dtype=np.int32)
    spans, F = [(2, 1, 70), (6, 71, 3)], 76
    ids = [2, 6]
    fresh = ctx.export_streams(ids)
    for c in (ctx, twin):
        c.resample(_plain(golden_dir, 2, 48000, 3), 48000, 16000, ids, side="encoder")
        c.resample(_plain(golden_dir, 2, 16000, 4), 16000, 32000, ids, side="decoder")
    dirtied = ctx.export_streams(ids)
    slots = fresh != dirtied
    assert slots.sum() > 60, "the resampler slots were dirtied"
    x = np.full((F, 320), FILL16, np.int16)
    x[1:71], x[71:74] = _audio(golden_dir, 70, 16000, 9), _pattern(golden_dir, "SZS", 16000, 10)
    rng = np.random.default_rng(5)
    bits = rng.choice(BITS, F).astype(np.int32)
    rates = [16000, 16000]
    t_pk, t_nb = _filled(dev, F, ROW, np.uint8), _filled(dev, F, 1, np.int32).view(-1)
    twin.encode_spans_mixed_dev(spans, torch.from_numpy(x).to(dev), bits, t_pk, t_nb, lanes, dtx=True)
    d_pk, d_nb, d_p16 = _filled(dev, F, ROW, np.uint8), _filled(dev, F, 1, np.int32).view(-1), _filled(dev, F, 320, np.int16)
    ctx.encode_spans_rates_dev(spans, torch.from_numpy(_padded(x, FILL16)).to(dev), rates, d_p16, bits, d_pk, d_nb, lanes, dtx=True)
    ctx.synchronize(); twin.synchronize()
    nb = d_nb.cpu().numpy()
    assert np.array_equal(d_pk.cpu().numpy(), t_pk.cpu().numpy()) and np.array_equal(nb, t_nb.cpu().numpy())
    assert (nb[1:71] == 0).any() and (nb[1:71] > 0).any()
    p16 = d_p16.cpu().numpy()
    assert np.array_equal(p16[1:74], x[1:74]) and (p16[[0, 74, 75]] == FILL16).all(), "d_pcm16 holds the copy of the span rows"
    _check_state("16000 encode", ctx, twin, ids, lanes)
    # decode
    pk184 = _packets(enc, golden_dir, 73, 184, 77)
    pb = np.full(F, 85, np.int32)
    pb[1:74] = _draw_sizes(rng, _bursts(73, (20, 10), (45, 2), (60, 9), (71, 1)))
    rows = np.full((F, ROW), FILL, np.uint8)
    rows[1:74] = _rows_of(pk184, pb[1:74])
    d_rows = torch.from_numpy(rows).to(dev)
    t = [_filled(dev, F, 320, np.int16), _filled(dev, F, 1, np.int32).view(-1), _filled(dev, F, 1, np.int32).view(-1)]
    twin.decode_spans_lossy_mixed_dev(spans, d_rows, pb, t[0], lanes, d_is_noise=t[1], d_is_comfort_noise=t[2])
    d = [_filled(dev, F, 320, np.int16), _filled(dev, F, 1, np.int32).view(-1), _filled(dev, F, 1, np.int32).view(-1)]
    d_ext = _filled(dev, F, EXT, np.int16)
    ctx.decode_spans_lossy_rates_dev(spans, d_rows, pb, rates, d[0], d_ext, lanes, d_is_noise=d[1], d_is_comfort_noise=d[2])
    ctx.synchronize(); twin.synchronize()
    for a, b, name in zip(d, t, ("pcm16", "is_noise", "is_comfort_noise")):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), name
    ext, p16 = d_ext.cpu().numpy(), d[0].cpu().numpy()
    assert np.array_equal(ext[1:74, :320], p16[1:74]) and (ext[1:74, 320:] == FILL16).all() and (ext[[0, 74, 75]] == FILL16).all()
    assert d[2].cpu().numpy()[1:74].any()
    _check_state("16000 decode", ctx, twin, ids, lanes)
    assert np.array_equal(ctx.export_streams(ids)[slots], dirtied[slots]), "a resampler slot changed"


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(golden_dir):
    """LYRA_HIP_EINVAL from each `_dev` form before the first kernel: every buffer still holds the filler, the blobs and the three
    error counters are what they were."""
    import torch
    import lyra_amd.codec as codec
    ctx, enc = _ctx(), _ctx()
    dev = _dev()
    n, F = 20, 24
    ok = [(7, 2, n), (20, 2 + n, 0)]
    lanes = np.arange(40, 48, dtype=np.int32)
    ids = np.concatenate([[7, 20], lanes])
    # streams that are not in the reset state, a burst in progress on the decode side
    x = _plain(golden_dir, 4, 48000, 77)
    pk184 = _packets(enc, golden_dir, 4, 184, 8)
    _twin_encode(ctx, None, {7: x}, {7: [64, 120, 184, 8]})
    _twin_decode(ctx, {7: pk184}, {7: [23, 23, 0, 0]})
    before = ctx.export_streams(ids)
    counters = (ctx.rates_errors(), ctx.encode_mixed_errors(), ctx.decode_lossy_errors())
    bits_f, pb_f = np.full(F, 184, np.int32), np.full(F, 23, np.int32)
    bits_f[[0, 1, F - 2, F - 1]], pb_f[[0, 1, F - 2, F - 1]] = 186, 16   # outside the spans nobody looks
    d_x, d_rows = _filled(dev, F, EXT, np.int16), _filled(dev, F, ROW, np.uint8)
    d_p16, d_pk, d_nb = _filled(dev, F, 320, np.int16), _filled(dev, F, ROW, np.uint8), _filled(dev, F, 1, np.int32).view(-1)
    d_ext, d_n, d_cn = _filled(dev, F, EXT, np.int16), _filled(dev, F, 1, np.int32).view(-1), _filled(dev, F, 1, np.int32).view(-1)
    d_odd = _filled(dev, F + 1, EXT, np.int16).view(-1)[1:1 + F * EXT].view(F, EXT)   # 2 bytes off a 16-byte boundary
    d_odd16 = _filled(dev, F + 1, 320, np.int16).view(-1)[1:1 + F * 320].view(F, 320)
    assert d_odd.data_ptr() % 16 == 2 and d_odd16.data_ptr() % 16 == 2
    NULL = "null"
    def with_at(v, at, value):
        out = v.copy()
        out[at] = value
        return out
    def arg(case, key, default, to):
        v = case.get(key, default)
        return None if v is NULL else to(v)
    ptr, host = (lambda t: t.data_ptr()), (lambda a: np.ascontiguousarray(a, np.int32).ctypes.data)
    common = [dict(rates=[44100, 8000]), dict(rates=[48000, 44100]), dict(rates=[0, 8000]), dict(rates=NULL), dict(p16=NULL),
              dict(p16=d_odd16), dict(ext=NULL), dict(ext=d_odd), dict(spans=[(7, 2, n), (20, 10, 5)]), dict(lanes=[7, 41]),
              dict(spans=[(MAX_STREAMS, 2, n), (20, 2 + n, 0)])]
    held = []
    def call(form, case):
        sp = codec._spans(case.get("spans", ok))
        ln = np.asarray(case.get("lanes", lanes), np.int32)
        rates = case.get("rates", [48000, 8000])
        rates = None if rates is NULL else np.asarray(rates, np.int32)
        held.append((sp, ln, rates))
        head = (ctx.h, sp.ctypes.data, sp.size, ln.ctypes.data, ln.size)
        p_rates = None if rates is None else rates.ctypes.data
        if form == "encode":
            return ctx.L.lyra_hip_encode_spans_rates_dev(*head, arg(case, "ext", d_x, ptr), p_rates, arg(case, "p16", d_p16, ptr),
                                                         arg(case, "bits", bits_f, host), case.get("dtx", 0), ptr(d_pk),
                                                         arg(case, "d_nb", d_nb, ptr))
        if form == "lossy":
            return ctx.L.lyra_hip_decode_spans_lossy_rates_dev(*head, ptr(d_rows), arg(case, "pb", pb_f, host), p_rates,
                                                               arg(case, "p16", d_p16, ptr), arg(case, "ext", d_ext, ptr),
                                                               ptr(d_n), ptr(d_cn))
        return ctx.L.lyra_hip_decode_spans_rates_dev(*head, ptr(d_rows), case.get("num_bits", 184), p_rates,
                                                     arg(case, "p16", d_p16, ptr), arg(case, "ext", d_ext, ptr))
    own = {"encode": [dict(bits=with_at(bits_f, 9, b)) for b in (0, 2, 186, -4)] + [dict(bits=NULL), dict(d_nb=NULL)],
           "lossy": [dict(pb=with_at(pb_f, 9, s)) for s in (16, 7, -8)] + [dict(pb=NULL)],
           "plain": [dict(num_bits=b) for b in (0, 186, 63)]}
    for form in ("encode", "lossy", "plain"):
        for dtx in ((0, 1) if form == "encode" else (0,)):
            for case in common + own[form]:
                rc = call(form, {**case, "dtx": dtx})
                assert rc == EINVAL, (form, dtx, list(case), rc)
    ctx.synchronize()
    assert np.array_equal(ctx.export_streams(ids), before)
    for t in (d_x, d_rows, d_p16, d_pk, d_nb, d_ext, d_n, d_cn, d_odd, d_odd16):
        assert (t.cpu().numpy().view(np.uint8) == FILL).all()
    assert (ctx.rates_errors(), ctx.encode_mixed_errors(), ctx.decode_lossy_errors()) == counters
    for form in ("encode", "lossy", "plain"):   # and the valid call is accepted
        assert call(form, {}) == 0, (form, ctx.last_error())
    ctx.synchronize()
