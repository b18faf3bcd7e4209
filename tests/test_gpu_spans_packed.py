"""The span calls with a sample rate per span on a PACKED external-rate buffer, on the GPU (include/lyra_hip_spans_packed.h):
the three `_dev` forms and the three host-buffer forms.  Every comparison is BIT FOR BIT against the hop-by-hop calls on a twin
context with the same stream ids and comfort-noise seed, as in test_gpu_spans_rates.py, whose layout, signals and twins these
tests reuse; the encode test also holds the call to encode_spans_rates_dev on the same audio padded.

The external-rate buffer is flat and the spans touch in it at different rates (or lie 8 samples of filler apart): frame 0 of a
span has to take its resampler history from its stream's slot, a later frame from the 34 samples in front of its row, and a
decode writes a span's own samples and nothing else -- every other sample must still hold the filler."""
import functools
import os
import subprocess

import numpy as np
import pytest

from gpu_plumbing import FILL, _dev, _filled, make_ctx
from packed_cases import HOPS, LAYOUT, LAYOUT_OFFSETS, LAYOUT_TOTAL, _back_to_back, _check_flat, _flat, _scattered
from signals import _audio_dtx as _audio, _bursts, _pattern, _plain, _read_wav, _stretches, _write_wav
import span_cases
from span_cases import (BITS, EXT, FILL16, ROW, _by_frame, _check_packets, _check_rows, _check_state, _decode_schedule,
                        _dirty_lane, _draw_sizes, _encode_plan, _in_pos_offsets, _layout, _packets, _padded, _rows_of)

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MAX_STREAMS = 96
SEED = 0x5EEDC0DE
EINVAL = -1
GAPS = [2, 0, 3, 3, 0, 1, 0]          # filler frames in front of each span in the frame-major buffers
RATE_OF = {i: r for i, _, r in LAYOUT}
LANES = np.arange(24, 24 + 40, dtype=np.int32)
WARM = "SSZZZZZ"                       # what each stream has heard before its span (seven hops: odd)
SHORT = {0: "", 1: "Z", 3: "ZSZ", 5: "ZSZZZ"}

_twin_decode = functools.partial(span_cases._twin_decode_rates, rate_of=RATE_OF)
_twin_decode_plain = functools.partial(span_cases._twin_decode_plain, rate_of=RATE_OF)


def _ctx(mode="xnnpack"):
    return make_ctx(MAX_STREAMS, mode, cng_seed=SEED)


def _twin_encode(twin, aux, ext_by_id, bits_by_id, dtx=False):
    return span_cases._twin_encode_rows(twin, ext_by_id, bits_by_id, RATE_OF, dtx, aux)


def _span_audio(golden_dir, n, rate, seed):
    return _pattern(golden_dir, SHORT[n], rate, seed) if n in SHORT else _audio(golden_dir, n, rate, seed)


def _rates_of(spans):
    return np.array([RATE_OF[i] for (i, _, _) in spans], np.int32)


def _frames_of(spans):
    return [n for (_, _, n) in spans]


# ---- 1: encode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtx,mode", [(False, "xnnpack"), (True, "xnnpack")])
def test_one_packed_encode_call_at_all_four_rates_equals_hop_by_hop_and_the_padded_call(golden_dir, dtx, mode):
    """Seven spans at 48, 8, 32, 8, 16, 32 and 16 kHz back to back in the flat buffer (ext_offsets = NULL), 40 lanes, a bit count
    per frame, every stream live.  Lengths 0, 1, 3 and 5 leave a four-frame workgroup partly empty or cross it; every span touches
    its predecessor at another rate."""
    import torch
    ctx, twin, aux, pad = _ctx(mode), _ctx(mode), _ctx(mode), _ctx(mode)
    dev = _dev()
    where = f"{mode}/dtx={dtx}"
    rng = np.random.default_rng(17)
    warm = {i: _pattern(golden_dir, WARM, r, 500 + i) for i, _, r in LAYOUT}
    warm_bits = {i: rng.choice(BITS, len(WARM)) for i in warm}
    for c in (ctx, twin, pad):
        _twin_encode(c, aux if c is twin else None, warm, warm_bits, dtx)
    ext = {i: _span_audio(golden_dir, n, r, 200 + i) for i, n, r in LAYOUT}
    spans, padded = _layout({i: _padded(v, FILL16) for i, v in ext.items()}, GAPS)
    rates, F = _rates_of(spans), len(padded)
    offsets, total = _back_to_back(_frames_of(spans), rates)
    assert offsets == LAYOUT_OFFSETS and total == LAYOUT_TOTAL
    flat = _flat(spans, rates, ext, offsets, total)
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
    chunks, _, _, _ = _encode_plan(spans, active, LANES)
    assert any(c["n_warmup"] > 0 for c in chunks), (where, "the plan has no lane chunks")
    d_flat, d_p16 = torch.from_numpy(flat).to(dev), _filled(dev, F, 320, np.int16)
    d_pk, d_nb = _filled(dev, F, ROW, np.uint8), _filled(dev, F, 1, np.int32).view(-1)
    ctx.encode_spans_packed_dev(spans, d_flat, rates, d_p16, bits, d_pk, d_nb, LANES, dtx=dtx)
    ctx.synchronize()
    got = [d_pk.cpu().numpy(), d_nb.cpu().numpy(), d_p16.cpu().numpy()]
    _check_packets(where, got[0], got[1], spans, want_pk, want_nb)
    _check_rows(where + " pcm16", got[2], spans, want_16)
    assert np.array_equal(d_flat.cpu().numpy(), flat), f"{where}: the input buffer was written"
    _check_state(where, ctx, twin, [i for i, _, _ in LAYOUT], LANES)
    assert ctx.encode_mixed_errors() == 0 and ctx.rates_errors() == 0
    # the padded call on the same audio: every output buffer byte for byte, and the blobs
    p_p16, p_pk, p_nb = _filled(dev, F, 320, np.int16), _filled(dev, F, ROW, np.uint8), _filled(dev, F, 1, np.int32).view(-1)
    pad.encode_spans_rates_dev(spans, torch.from_numpy(padded).to(dev), rates, p_p16, bits, p_pk, p_nb, LANES, dtx=dtx)
    pad.synchronize()
    for a, b, name in zip(got, (p_pk, p_nb, p_p16), ("packets", "packet_bytes", "pcm16")):
        assert np.array_equal(a, b.cpu().numpy()), f"{where}: {name} differs from encode_spans_rates_dev"
    _check_state(where + " padded", ctx, pad, [i for i, _, _ in LAYOUT], LANES)


# ---- 2: lossy decode, explicit offsets ----------------------------------------------------------------------------------------------
def test_one_packed_lossy_decode_call_with_scattered_offsets_equals_hop_by_hop(golden_dir):
    """The layout with the 48 kHz span 350 frames long and the loss trace of test_gpu_spans_rates.py: comfort noise and fades on
    two spans.  In the flat buffer the spans lie in another order than in the list, 8 samples of filler between neighbours, in
    front of the first and behind the last: every filler sample must still be filler."""
    import torch
    import lyra_amd.codec as codec
    W = codec.span_warmup_frames("decoder")
    ctx, twin, enc = _ctx(), _ctx(), _ctx()
    dev = _dev()
    where = "lossy"
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
    rates = _rates_of(spans)
    offsets, total = _scattered(_frames_of(spans), rates, order=[4, 6, 0, 2, 5, 1, 3])
    assert sorted(offsets) != offsets and all(o % 8 == 0 for o in offsets)
    _dirty_lane((ctx, twin), int(LANES[3]), golden_dir)
    want_16, want_ext, want_n, want_cn = _twin_decode(twin, rows, pb)
    assert want_cn[7].any() and not want_cn[7].all() and want_cn[20].any() and not want_cn[20].all()
    assert any(b < 350 and pb[7][b] > 0 for _, b in _stretches(want_cn[7] != 0)), "no received tick behind comfort noise"
    d_pk = torch.from_numpy(buf).to(dev)
    d_16, d_ext = _filled(dev, F, 320, np.int16), _filled(dev, total, 1, np.int16).view(-1)
    d_n, d_cn = _filled(dev, F, 1, np.int32).view(-1), _filled(dev, F, 1, np.int32).view(-1)
    ctx.decode_spans_lossy_packed_dev(spans, d_pk, pb_all, rates, d_16, d_ext, LANES, d_is_noise=d_n, d_is_comfort_noise=d_cn,
                                      ext_offsets=offsets)
    ctx.synchronize()
    _check_rows(where + " is_comfort_noise", d_cn.cpu().numpy().reshape(F, 1), spans, want_cn)
    _check_rows(where + " is_noise", d_n.cpu().numpy().reshape(F, 1), spans, want_n)
    _check_rows(where + " pcm16", d_16.cpu().numpy(), spans, want_16)
    _check_flat(where + " pcm_ext", d_ext.cpu().numpy(), spans, rates, offsets, want_ext)
    assert np.array_equal(d_pk.cpu().numpy(), buf), f"{where}: the packet buffer was written"
    _check_state(where, ctx, twin, list(lengths), LANES)
    assert ctx.decode_lossy_errors() == 0 and ctx.rates_errors() == 0


# ---- 3: plain decode ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_bits", [64, 184])
def test_one_packed_plain_decode_call_equals_decode_plus_resample(golden_dir, num_bits):
    import torch
    ctx, twin, enc = _ctx(), _ctx(), _ctx()
    dev = _dev()
    where = f"plain/{num_bits}"
    pk = {i: _packets(enc, golden_dir, n, num_bits, 400 + i) for i, n, _ in LAYOUT}
    spans, buf = _layout(pk, GAPS)
    F, rates = len(buf), _rates_of(spans)
    want_16, want_ext = _twin_decode_plain(twin, pk, num_bits)
    d_pk = torch.from_numpy(buf).to(dev)
    d_16, d_ext = _filled(dev, F, 320, np.int16), _filled(dev, LAYOUT_TOTAL, 1, np.int16).view(-1)
    ctx.decode_spans_packed_dev(spans, d_pk, num_bits, rates, d_16, d_ext, LANES)
    ctx.synchronize()
    _check_rows(where + " pcm16", d_16.cpu().numpy(), spans, want_16)
    _check_flat(where + " pcm_ext", d_ext.cpu().numpy(), spans, rates, LAYOUT_OFFSETS, want_ext)
    assert np.array_equal(d_pk.cpu().numpy(), buf), f"{where}: the packet buffer was written"
    _check_state(where, ctx, twin, [i for i, _, _ in LAYOUT], LANES)
    assert ctx.rates_errors() == 0


# ---- 4: continuation ------------------------------------------------------------------------------------------------------------
def _set_phase(contexts, sid, side, value):
    """a decimation phase no call sequence reaches but a blob may carry: RS_IN_POS of the side's slot, on every context"""
    off = _in_pos_offsets(contexts[0], 90)[0 if side == "encoder" else 1]
    blob = contexts[0].export_streams([sid])
    assert np.array_equal(blob, contexts[1].export_streams([sid]))
    blob[0, off] = value
    for c in contexts:
        c.import_streams([sid], blob)
    return off


@pytest.mark.parametrize("n_lanes", [40, 0])
def test_packed_encode_span_continues_a_live_stream_with_a_decimation_phase_and_is_continued(golden_dir, n_lanes):
    """48 kHz: 7 hops hop by hop, RS_IN_POS set to 4 (phase 1 of 3), a PACKED span of 60 frames, a padded encode_spans_rates_dev
    span of 40 frames, 5 hops hop by hop: packets, the 16 kHz rows, the blobs and the final phase word equal the twin that went
    hop by hop throughout."""
    import torch
    ctx, twin, aux = _ctx(), _ctx(), _ctx()
    dev = _dev()
    sid, k, n1, n2, tail = 7, 7, 60, 40, 5
    lanes = np.arange(30, 30 + n_lanes, dtype=np.int32)
    total = k + n1 + n2 + tail
    x = _plain(golden_dir, total, 48000, 66)
    bits = np.random.default_rng(10).choice(BITS, total).astype(np.int32)
    cut = lambda d, a, b: {sid: d[a:b]}
    head = _twin_encode(ctx, None, cut(x, 0, k), cut(bits, 0, k))
    want_head = _twin_encode(twin, aux, cut(x, 0, k), cut(bits, 0, k))
    off = _set_phase((ctx, twin), sid, "encoder", 4)
    aux.import_streams([sid], twin.export_streams([sid]))
    want = _twin_encode(twin, aux, cut(x, k, total), cut(bits, k, total))
    F = k + n1 + n2
    d_pk, d_nb = torch.zeros((F, ROW), dtype=torch.uint8, device=dev), torch.zeros(F, dtype=torch.int32, device=dev)
    d_16 = torch.zeros((F, 320), dtype=torch.int16, device=dev)
    # the packed span: frames k .. k + n1 of the frame-major buffers, its samples 16 samples into a flat buffer of its own
    flat = np.full(16 + n1 * 960 + 8, FILL16, np.int16)
    flat[16:16 + n1 * 960] = x[k:k + n1].reshape(-1)
    ctx.encode_spans_packed_dev([(sid, k, n1)], torch.from_numpy(flat).to(dev), [48000], d_16, bits[:F], d_pk, d_nb, lanes,
                                ext_offsets=[16])
    # the padded span behind it: frames k + n1 .. of the same buffers
    ctx.encode_spans_rates_dev([(sid, k + n1, n2)], torch.from_numpy(_padded(x[:F], FILL16)).to(dev), [48000], d_16, bits[:F], d_pk,
                               d_nb, lanes)
    ctx.synchronize()
    mid_pk, mid_nb, mid_16 = d_pk.cpu().numpy(), d_nb.cpu().numpy(), d_16.cpu().numpy()
    assert not mid_pk[:k].any() and not mid_nb[:k].any() and not mid_16[:k].any()
    rest = _twin_encode(ctx, None, cut(x, F, total), cut(bits, F, total))
    got_nb = np.concatenate([mid_nb[k:], rest[1][sid]])
    assert np.array_equal(got_nb, want[1][sid])
    got_pk = np.concatenate([mid_pk[k:], rest[0][sid]])
    for h, row in enumerate(got_pk):
        assert np.array_equal(row[:got_nb[h]], want[0][sid][h][:got_nb[h]]), (h, "packet")
    assert np.array_equal(head[0][sid], want_head[0][sid])
    assert np.array_equal(mid_16[k:], want[2][sid][:n1 + n2]), "the 16 kHz rows of the two span calls"
    _check_state("continued encode", ctx, twin, [sid], lanes)
    assert ctx.export_streams([sid])[0, off] == (4 + (n1 + n2 + tail) * 960) % 6


@pytest.mark.parametrize("n_lanes", [40, 0])
def test_packed_decode_span_continues_a_live_stream_mid_burst_with_a_decimation_phase_and_is_continued(golden_dir, n_lanes):
    """8 kHz: 5 ticks hop by hop that end inside a burst, RS_IN_POS set to 3 (phase 1 of 2), a PACKED span of 60 ticks that ends
    inside another burst, a padded decode_spans_lossy_rates_dev span of 40 ticks, 5 ticks hop by hop."""
    import torch
    ctx, twin, enc = _ctx(), _ctx(), _ctx()
    dev = _dev()
    sid, k, n1, n2, tail = 20, 5, 60, 40, 5
    lanes = np.arange(30, 30 + n_lanes, dtype=np.int32)
    total = k + n1 + n2 + tail
    pk184 = _packets(enc, golden_dir, total, 184, 55)
    rx = _bursts(total, (3, 6), (30, 12), (k + n1 - 2, 5), (k + n1 + 20, 3))
    assert not rx[k] and not rx[k + n1], "both span calls start mid-burst"
    pb = _draw_sizes(np.random.default_rng(9), rx)
    rows = _rows_of(pk184, pb)
    cut = lambda d, a, b: {sid: d[a:b]}
    head = _twin_decode(ctx, cut(rows, 0, k), cut(pb, 0, k))
    want_head = _twin_decode(twin, cut(rows, 0, k), cut(pb, 0, k))
    off = _set_phase((ctx, twin), sid, "decoder", 3)
    want = _twin_decode(twin, cut(rows, k, total), cut(pb, k, total))
    F = k + n1 + n2
    d_rows = torch.from_numpy(np.ascontiguousarray(rows[:F])).to(dev)
    d_16, d_padded = torch.zeros((F, 320), dtype=torch.int16, device=dev), torch.zeros((F, EXT), dtype=torch.int16, device=dev)
    d_n, d_cn = torch.zeros(F, dtype=torch.int32, device=dev), torch.zeros(F, dtype=torch.int32, device=dev)
    d_flat = _filled(dev, 8 + n1 * 160 + 8, 1, np.int16).view(-1)
    ctx.decode_spans_lossy_packed_dev([(sid, k, n1)], d_rows, pb[:F], [8000], d_16, d_flat, lanes, d_is_noise=d_n,
                                      d_is_comfort_noise=d_cn, ext_offsets=[8])
    ctx.decode_spans_lossy_rates_dev([(sid, k + n1, n2)], d_rows, pb[:F], [8000], d_16, d_padded, lanes, d_is_noise=d_n,
                                     d_is_comfort_noise=d_cn)
    ctx.synchronize()
    flat, padded = d_flat.cpu().numpy(), d_padded.cpu().numpy()
    assert (flat[:8] == FILL16).all() and (flat[-8:] == FILL16).all(), "samples around the packed span were written"
    assert not padded[:k + n1].any() and not padded[:, 160:].any()
    mid = [d_16.cpu().numpy(), np.concatenate([flat[8:-8].reshape(n1, 160), padded[k + n1:, :160]]), d_n.cpu().numpy(),
           d_cn.cpu().numpy()]
    rest = _twin_decode(ctx, cut(rows, F, total), cut(pb, F, total))
    for q, name in enumerate(("pcm16", "pcm_ext", "is_noise", "is_comfort_noise")):
        assert q == 1 or not mid[q][:k].any(), name
        got = np.concatenate([mid[q] if q == 1 else mid[q][k:], rest[q][sid]])
        diff = np.flatnonzero((got.reshape(len(got), -1) != want[q][sid].reshape(len(got), -1)).any(axis=1))
        assert len(diff) == 0, (name, list(diff[:8]), len(diff))
        assert np.array_equal(head[q][sid], want_head[q][sid]), name
    assert want[3][sid][:n1].any() and not want[3][sid][:n1].all(), "the packed span has comfort noise and generated hops"
    _check_state("continued decode", ctx, twin, [sid], lanes)
    assert ctx.export_streams([sid])[0, off] == (3 + (n1 + n2 + tail) * 320) % 6


# ---- 5: the host-buffer forms -----------------------------------------------------------------------------------------------------
HOST_SPANS = [(7, 2, 9), (11, 11, 1), (3, 14, 0), (20, 14, 70), (5, 86, 5)]   # 70 frames run on lanes; F = 93


def _host_call(ctx, form, spans, lanes, rates, offsets, bufs, **kw):
    """one of the host-buffer forms through the C ABI on numpy buffers: the return code"""
    import lyra_amd.codec as codec
    sp, ln = codec._spans(spans), np.ascontiguousarray(lanes, np.int32)
    rt = np.ascontiguousarray(rates, np.int32)
    off = None if offsets is None else np.ascontiguousarray(offsets, np.int64)
    head = (ctx.h, sp.ctypes.data, sp.size, ln.ctypes.data, ln.size)
    p = lambda a: None if a is None else a.ctypes.data
    if form == "encode":
        return ctx.L.lyra_hip_encode_spans_packed(*head, p(bufs["ext"]), bufs["ext"].size, p(off), p(rt), p(bufs["bits"]),
                                                  kw.get("dtx", 0), p(bufs["pk"]), p(bufs["nb"]))
    if form == "lossy":
        return ctx.L.lyra_hip_decode_spans_lossy_packed(*head, p(bufs["rows"]), p(bufs["pb"]), p(rt), p(bufs.get("p16")),
                                                        p(bufs["ext"]), bufs["ext"].size, p(off), p(bufs.get("n")), p(bufs.get("cn")))
    return ctx.L.lyra_hip_decode_spans_packed(*head, p(bufs["rows"]), kw["num_bits"], p(rt), p(bufs.get("p16")), p(bufs["ext"]),
                                              bufs["ext"].size, p(off))


def test_host_forms_equal_the_dev_forms_and_write_nothing_else(golden_dir):
    """The three host-buffer forms against the `_dev` forms on a second context, on prefilled outputs: the spans' frames and
    samples equal, packet bytes behind a size and rows of noise frames zero, every byte outside the spans untouched; a call
    whose spans all have no frames does nothing; a large call behind a small one works."""
    import torch
    host, devc, enc = _ctx(), _ctx(), _ctx()
    dev = _dev()
    spans, F = HOST_SPANS, 93
    rates = _rates_of(spans)
    lanes = np.arange(40, 70, dtype=np.int32)
    offsets, total = _scattered(_frames_of(spans), rates, order=[3, 0, 4, 2, 1])
    rng = np.random.default_rng(23)
    ext = {i: _audio(golden_dir, n, RATE_OF[i], 700 + i) if n >= 60 else _pattern(golden_dir, "SSZZZZZSZ"[:n], RATE_OF[i], 700 + i)
           for i, _, n in spans}
    flat = _flat(spans, rates, ext, offsets, total)
    bits = rng.choice(BITS, F).astype(np.int32)
    # a small call first: the staging of the big one has to grow behind it
    small = dict(ext=flat[offsets[1]:offsets[1] + 160].copy(), bits=bits, pk=_filled(None, F, ROW, np.uint8),
                 nb=_filled(None, F, 1, np.int32).reshape(-1))
    assert _host_call(host, "encode", [(11, 11, 1)], lanes, [8000], None, small) == 0, host.last_error()
    d_p16, d_pk, d_nb = _filled(dev, F, 320, np.int16), _filled(dev, F, ROW, np.uint8), _filled(dev, F, 1, np.int32).view(-1)
    devc.encode_spans_packed_dev([(11, 11, 1)], torch.from_numpy(small["ext"]).to(dev), [8000], d_p16, bits, d_pk, d_nb, lanes)
    # encode with DTX
    out = dict(ext=flat.copy(), bits=bits, pk=_filled(None, F, ROW, np.uint8), nb=_filled(None, F, 1, np.int32).reshape(-1))
    assert _host_call(host, "encode", spans, lanes, rates, offsets, out, dtx=1) == 0, host.last_error()
    d_p16, d_pk, d_nb = _filled(dev, F, 320, np.int16), _filled(dev, F, ROW, np.uint8), _filled(dev, F, 1, np.int32).view(-1)
    devc.encode_spans_packed_dev(spans, torch.from_numpy(flat).to(dev), rates, d_p16, bits, d_pk, d_nb, lanes, dtx=True,
                                 ext_offsets=offsets)
    devc.synchronize()
    assert np.array_equal(out["ext"], flat), "the input was written"
    want_pk, want_nb = d_pk.cpu().numpy(), d_nb.cpu().numpy()
    inside = np.zeros(F, bool)
    for (_, first, n) in spans:
        inside[first:first + n] = True
    assert np.array_equal(out["nb"][inside], want_nb[inside]) and (out["nb"][inside] > 0).any()
    assert (out["nb"][~inside].view(np.uint8) == FILL).all() and (out["pk"][~inside] == FILL).all(), "rows outside the spans"
    for f in np.flatnonzero(inside):
        assert np.array_equal(out["pk"][f, :want_nb[f]], want_pk[f, :want_nb[f]]) and not out["pk"][f, want_nb[f]:].any(), f
    _check_state("host encode", host, devc, [i for i, _, _ in spans], lanes)
    # lossy decode: every output given, then the optional ones left out
    pk184 = {i: _packets(enc, golden_dir, n, 184, 800 + i) for i, _, n in spans}
    pb_by = {i: _draw_sizes(rng, _bursts(n, (n // 3, min(12, max(n // 4, 1))))) if n else np.zeros(0, np.int32)
             for i, _, n in spans}
    pb = _by_frame(spans, pb_by, F)
    rows = np.full((F, ROW), FILL, np.uint8)
    for (i, first, n) in spans:
        rows[first:first + n] = _rows_of(pk184[i], pb_by[i])
    out = dict(rows=rows.copy(), pb=pb, p16=_filled(None, F, 320, np.int16), ext=_filled(None, total, 1, np.int16).reshape(-1),
               n=_filled(None, F, 1, np.int32).reshape(-1), cn=_filled(None, F, 1, np.int32).reshape(-1))
    assert _host_call(host, "lossy", spans, lanes, rates, offsets, out) == 0, host.last_error()
    d_16, d_ext = _filled(dev, F, 320, np.int16), _filled(dev, total, 1, np.int16).view(-1)
    d_n, d_cn = _filled(dev, F, 1, np.int32).view(-1), _filled(dev, F, 1, np.int32).view(-1)
    devc.decode_spans_lossy_packed_dev(spans, torch.from_numpy(rows).to(dev), pb, rates, d_16, d_ext, lanes, d_is_noise=d_n,
                                       d_is_comfort_noise=d_cn, ext_offsets=offsets)
    devc.synchronize()
    for name, t in (("p16", d_16), ("ext", d_ext), ("n", d_n), ("cn", d_cn)):
        assert np.array_equal(out[name], t.cpu().numpy()), f"host lossy decode: {name} (the filler outside the spans included)"
    assert np.array_equal(out["rows"], rows) and d_cn.cpu().numpy()[inside].any()
    _check_state("host lossy decode", host, devc, [i for i, _, _ in spans], lanes)
    # plain decode without the optional 16 kHz output, back to back
    pk64 = {i: _packets(enc, golden_dir, n, 64, 900 + i) for i, _, n in spans}
    rows = np.full((F, 8), FILL, np.uint8)
    for (i, first, n) in spans:
        rows[first:first + n] = pk64[i]
    b2b, total2 = _back_to_back(_frames_of(spans), rates)
    out = dict(rows=rows.copy(), ext=_filled(None, total2 + 8, 1, np.int16).reshape(-1))
    assert _host_call(host, "plain", spans, lanes, rates, None, out, num_bits=64) == 0, host.last_error()
    d_16, d_ext = _filled(dev, F, 320, np.int16), _filled(dev, total2 + 8, 1, np.int16).view(-1)
    devc.decode_spans_packed_dev(spans, torch.from_numpy(rows).to(dev), 64, rates, d_16, d_ext, lanes)
    devc.synchronize()
    assert np.array_equal(out["ext"], d_ext.cpu().numpy()) and (out["ext"][total2:] == FILL16).all()
    _check_state("host plain decode", host, devc, [i for i, _, _ in spans], lanes)
    # spans without frames: nothing happens
    before = host.export_streams([7, 20])
    empty = [(7, 2, 0), (20, 50, 0)]
    out = dict(ext=_filled(None, 16, 1, np.int16).reshape(-1), bits=bits, pk=_filled(None, F, ROW, np.uint8),
               nb=_filled(None, F, 1, np.int32).reshape(-1))
    assert _host_call(host, "encode", empty, lanes, [48000, 8000], [0, 8], out) == 0, host.last_error()
    dec = dict(rows=_filled(None, F, ROW, np.uint8), pb=pb, p16=_filled(None, F, 320, np.int16),
               ext=_filled(None, 16, 1, np.int16).reshape(-1))
    assert _host_call(host, "lossy", empty, lanes, [48000, 8000], None, dec) == 0, host.last_error()
    assert _host_call(host, "plain", empty, lanes, [48000, 8000], None, dec, num_bits=184) == 0, host.last_error()
    for a in (out["ext"], out["pk"], out["nb"], dec["rows"], dec["p16"], dec["ext"]):
        assert (a.view(np.uint8) == FILL).all()
    assert np.array_equal(host.export_streams([7, 20]), before)


# ---- 6: all spans at 16000 ------------------------------------------------------------------------------------------------------
def test_all_packed_spans_at_16000_equal_the_mixed_span_calls(golden_dir):
    """Outputs and blobs equal encode_spans_mixed_dev (with DTX) / decode_spans_lossy_mixed_dev at 16000, the flat buffer carries
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
    offsets = [8 + 3 * 320 + 8, 8]     # the second span in front of the first
    total = offsets[0] + 70 * 320 + 8
    flat = _flat(spans, rates, {2: x[1:71], 6: x[71:74]}, offsets, total)
    t_pk, t_nb = _filled(dev, F, ROW, np.uint8), _filled(dev, F, 1, np.int32).view(-1)
    twin.encode_spans_mixed_dev(spans, torch.from_numpy(x).to(dev), bits, t_pk, t_nb, lanes, dtx=True)
    d_pk, d_nb, d_p16 = _filled(dev, F, ROW, np.uint8), _filled(dev, F, 1, np.int32).view(-1), _filled(dev, F, 320, np.int16)
    ctx.encode_spans_packed_dev(spans, torch.from_numpy(flat).to(dev), rates, d_p16, bits, d_pk, d_nb, lanes, dtx=True,
                                ext_offsets=offsets)
    ctx.synchronize(); twin.synchronize()
    nb = d_nb.cpu().numpy()
    assert np.array_equal(d_pk.cpu().numpy(), t_pk.cpu().numpy()) and np.array_equal(nb, t_nb.cpu().numpy())
    assert (nb[1:71] == 0).any() and (nb[1:71] > 0).any()
    p16 = d_p16.cpu().numpy()
    assert np.array_equal(p16[1:74], x[1:74]) and (p16[[0, 74, 75]] == FILL16).all(), "d_pcm16 holds the copy of the span rows"
    _check_state("16000 encode", ctx, twin, ids, lanes)
    pk184 = _packets(enc, golden_dir, 73, 184, 77)
    pb = np.full(F, 85, np.int32)
    pb[1:74] = _draw_sizes(rng, _bursts(73, (20, 10), (45, 2), (60, 9), (71, 1)))
    rows = np.full((F, ROW), FILL, np.uint8)
    rows[1:74] = _rows_of(pk184, pb[1:74])
    d_rows = torch.from_numpy(rows).to(dev)
    t = [_filled(dev, F, 320, np.int16), _filled(dev, F, 1, np.int32).view(-1), _filled(dev, F, 1, np.int32).view(-1)]
    twin.decode_spans_lossy_mixed_dev(spans, d_rows, pb, t[0], lanes, d_is_noise=t[1], d_is_comfort_noise=t[2])
    d = [_filled(dev, F, 320, np.int16), _filled(dev, F, 1, np.int32).view(-1), _filled(dev, F, 1, np.int32).view(-1)]
    d_ext = _filled(dev, total, 1, np.int16).view(-1)
    ctx.decode_spans_lossy_packed_dev(spans, d_rows, pb, rates, d[0], d_ext, lanes, d_is_noise=d[1], d_is_comfort_noise=d[2],
                                      ext_offsets=offsets)
    ctx.synchronize(); twin.synchronize()
    for a, b, name in zip(d, t, ("pcm16", "is_noise", "is_comfort_noise")):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy()), name
    p16 = d[0].cpu().numpy()
    _check_flat("16000 decode", d_ext.cpu().numpy(), spans, rates, offsets, {2: p16[1:71], 6: p16[71:74]})
    assert d[2].cpu().numpy()[1:74].any()
    _check_state("16000 decode", ctx, twin, ids, lanes)
    assert np.array_equal(ctx.export_streams(ids)[slots], dirtied[slots]), "a resampler slot changed"


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------------
def test_packed_refusals_change_nothing(golden_dir):
    """LYRA_HIP_EINVAL from each of the six forms before the first kernel: every buffer still holds the filler, the blobs and the
    three error counters are what they were; the valid call is then accepted."""
    import torch
    import lyra_amd.codec as codec
    ctx, enc = _ctx(), _ctx()
    dev = _dev()
    n, m, F = 20, 4, 30
    ok = [(7, 2, n), (20, 2 + n, m), (9, 2 + n + m, 0)]
    ok_rates, ok_off = [48000, 8000, 32000], [0, n * 960, 8]
    E = n * 960 + m * 160
    lanes = np.arange(40, 48, dtype=np.int32)
    ids = np.concatenate([[7, 20, 9], lanes])
    x = _plain(golden_dir, 4, 48000, 77)
    pk184 = _packets(enc, golden_dir, 4, 184, 8)
    _twin_encode(ctx, None, {7: x}, {7: [64, 120, 184, 8]})
    _twin_decode(ctx, {7: pk184}, {7: [23, 23, 0, 0]})
    before = ctx.export_streams(ids)
    counters = (ctx.rates_errors(), ctx.encode_mixed_errors(), ctx.decode_lossy_errors())
    bits_f, pb_f = np.full(F, 184, np.int32), np.full(F, 23, np.int32)
    bits_f[[0, 1, F - 2, F - 1]], pb_f[[0, 1, F - 2, F - 1]] = 186, 16   # outside the spans nobody looks
    D = dict(ext=_filled(dev, E, 1, np.int16).view(-1), rows=_filled(dev, F, ROW, np.uint8), p16=_filled(dev, F, 320, np.int16),
             pk=_filled(dev, F, ROW, np.uint8), nb=_filled(dev, F, 1, np.int32).view(-1), n=_filled(dev, F, 1, np.int32).view(-1),
             cn=_filled(dev, F, 1, np.int32).view(-1), odd=_filled(dev, E + 8, 1, np.int16).view(-1)[1:1 + E])
    assert D["odd"].data_ptr() % 16 == 2
    H = {k: _filled(None, *shape) for k, shape in dict(ext=(E, 1, np.int16), rows=(F, ROW, np.uint8), p16=(F, 320, np.int16),
                                                       pk=(F, ROW, np.uint8), nb=(F, 1, np.int32), n=(F, 1, np.int32),
                                                       cn=(F, 1, np.int32)).items()}
    NULL = "null"
    def with_at(v, at, value):
        out = v.copy()
        out[at] = value
        return out
    # the offset faults, a bad buffer, null or bad rates, and refusals of the rates twin's own
    common = [dict(off=[-8, n * 960, 8]), dict(off=[0, n * 960 + 4, 8]), dict(off=[0, n * 960, 4]), dict(off=[0, n * 960 + 8, 8]),
              dict(off=[8, n * 960, 8]), dict(off=[0, (n - 1) * 960, 8]), dict(off=[m * 160 - 8, 0, 8]), dict(n_ext=-1),
              dict(n_ext=E - 1), dict(off=NULL, n_ext=E - 8), dict(rates=[44100, 8000, 32000]), dict(rates=[48000, 8000, 0]),
              dict(off=NULL, rates=[48000, 44100, 32000]), dict(rates=NULL), dict(ext=NULL),
              dict(spans=[(7, 2, n), (20, 10, m), (9, 0, 0)]), dict(lanes=[7, 41]), dict(spans=[(MAX_STREAMS, 2, n), (20, 2 + n, m), (9, 0, 0)])]
    dev_only = [dict(ext="odd"), dict(p16=NULL)]
    held = []
    def call(form, host, case):
        B = H if host else D
        ptr = (lambda a: a.ctypes.data) if host else (lambda t: t.data_ptr())
        def buf(key, name=None):
            v = case.get(key, name or key)
            return None if v is NULL else ptr(B[v])
        def harr(key, default, dtype):
            v = case.get(key, default)
            if v is NULL:
                return None
            held.append(np.ascontiguousarray(v, dtype))
            return held[-1].ctypes.data
        sp = codec._spans(case.get("spans", ok))
        ln = np.asarray(case.get("lanes", lanes), np.int32)
        held.append((sp, ln))
        head = (ctx.h, sp.ctypes.data, sp.size, ln.ctypes.data, ln.size)
        rates, off = harr("rates", ok_rates, np.int32), harr("off", ok_off, np.int64)
        n_ext = case.get("n_ext", E)
        fn = getattr(ctx.L, {"encode": "lyra_hip_encode_spans_packed", "lossy": "lyra_hip_decode_spans_lossy_packed",
                             "plain": "lyra_hip_decode_spans_packed"}[form] + ("" if host else "_dev"))
        p16 = () if host and form == "encode" else (buf("p16"),)
        if form == "encode":
            return fn(*head, buf("ext"), n_ext, off, rates, *p16, harr("bits", bits_f, np.int32), case.get("dtx", 0), buf("pk"),
                      buf("d_nb", "nb"))
        if form == "lossy":
            return fn(*head, buf("rows"), harr("pb", pb_f, np.int32), rates, *p16, buf("ext"), n_ext, off, buf("n"), buf("cn"))
        return fn(*head, buf("rows"), case.get("num_bits", 184), rates, *p16, buf("ext"), n_ext, off)
    own = {"encode": [dict(bits=with_at(bits_f, 9, b)) for b in (0, 186)] + [dict(bits=NULL), dict(d_nb=NULL)],
           "lossy": [dict(pb=with_at(pb_f, 9, s)) for s in (16, -8)] + [dict(pb=NULL)],
           "plain": [dict(num_bits=b) for b in (0, 63)]}
    for form in ("encode", "lossy", "plain"):
        for host in (False, True):
            for case in common + own[form] + ([] if host else dev_only):
                if host and case.get("p16") is NULL:
                    continue
                rc = call(form, host, case)
                assert rc == EINVAL, (form, host, {k: v for k, v in case.items() if k != "bits" and k != "pb"}, rc)
    ctx.synchronize()
    assert np.array_equal(ctx.export_streams(ids), before)
    for t in D.values():
        assert (t.cpu().numpy().view(np.uint8) == FILL).all()
    for a in H.values():
        assert (a.view(np.uint8) == FILL).all()
    assert (ctx.rates_errors(), ctx.encode_mixed_errors(), ctx.decode_lossy_errors()) == counters
    for form in ("encode", "lossy", "plain"):   # and the valid call is accepted
        for host in (False, True):
            assert call(form, host, {}) == 0, (form, host, ctx.last_error())
    ctx.synchronize()


# ---- 8: archive_demo ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtx", [False, True])
def test_archive_demo_time_parallel_equals_hop_by_hop(golden_dir, tmp_path, dtx):
    """Four WAVs of golden speech at 8, 16, 32 and 48 kHz, 150 to 400 hops long, and one shorter than a hop, through archive_demo
    --lanes=64 with decode rates that differ from the encode rates: the time-parallel calls and the hop-by-hop classes agree on
    every packet and every sample; with --dtx on the half-silent signal."""
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "archive_demo")
    assert os.path.exists(demo), "lyra_amd/archive_demo not built (__graft_entry__.build())"
    files = [("a8", 8000, 400, 48000), ("b16", 16000, 150, 8000), ("c32", 32000, 230, 16000), ("d48", 48000, 310, 32000),
             ("tiny", 32000, 0, 48000)]
    wavs = []
    for k, (name, rate, hops, _) in enumerate(files):
        x = (_audio if dtx else _plain)(golden_dir, hops, rate, 40 + k).reshape(-1) if hops else np.zeros(0, np.int16)
        x = np.concatenate([x, np.full(rate // 50 - 1 if not hops else 37, 100, np.int16)])   # a tail that is no whole hop
        wavs.append(str(tmp_path / f"{name}.wav"))
        _write_wav(wavs[-1], x, rate)
    out = tmp_path / "out"
    out.mkdir()
    flags = ["--lanes=64", "--decode-rates=" + ",".join(str(f[3]) for f in files)] + (["--dtx"] if dtx else [])
    r = subprocess.run([demo] + flags + [lyra_amd.default_model_dir(), "6000", str(out)] + wavs, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert "encode equal decode equal" in r.stdout, r.stdout
    assert "8 kHz 400, 16 kHz 150, 32 kHz 230, 48 kHz 310" in r.stdout, r.stdout
    for name, rate, hops, decode_rate in files:
        dec = _read_wav(out / f"{name}_decoded.wav", decode_rate)
        assert dec.size == hops * (decode_rate // 50), name
        if dtx:
            assert not os.path.exists(out / f"{name}.lyra"), name
        else:
            assert os.path.getsize(out / f"{name}.lyra") == hops * 15, name
    if dtx:
        assert " 0 empty packets" not in r.stdout, r.stdout
