"""The staging path of the blocking span calls (spans_api.inc: the host-buffer forms stage frames 0 .. end - 1 on the device, run
the `_dev` form and read back the spans' own frames) at its corners: gaps between spans, a span of no frames, rows behind the
last span, calls with nothing to do, and a large call behind a small one on the same context.  The C functions are called
through ctx.L with the output arrays prefilled, so that a row the call must not write still holds the filler afterwards.  Every
row of a span is compared BIT FOR BIT with the hop-by-hop calls on a twin context (the twin helpers of
tests/span_cases.py), computed once per rate and shared."""
import numpy as np
import pytest

import gpu_plumbing
from gpu_plumbing import FILL, make_ctx
from signals import _audio_dtx, _audio_ext
from span_cases import _check_rows, _twin_decode_ext, _twin_encode_ext

pytestmark = pytest.mark.gpu
MAX_STREAMS = 96
BITS = 120
A, B, C = 5, 9, 2            # the spans' streams
LANES = np.array([40, 41], np.int32)
SMALL = 30                   # the stream of the small call in front (test_grow_after_small)
_WANT = {}


def _job(W):
    """spans A (7 frames at 3), B (none), C (2 W + 5 frames at 20) and the frames of the buffer: 4 more than the last span frame"""
    return [(A, 3, 7), (B, 12, 0), (C, 20, 2 * W + 5)], 20 + 2 * W + 5 + 4


def _buffer(rows_by_id, spans, frames):
    first = next(iter(rows_by_id.values()))
    buf = np.full((frames, first.shape[1] * first.dtype.itemsize), FILL, np.uint8).view(first.dtype)
    for (i, at, n) in spans:
        buf[at:at + n] = rows_by_id[i]
    return np.ascontiguousarray(buf)


def _filled(frames, width, dtype):
    return gpu_plumbing._filled(None, frames, width, dtype)


def _ctx(rate):
    return make_ctx(MAX_STREAMS, rate=rate)


def _want(golden_dir, rate):
    """What the hop-by-hop calls give for the streams of _job, in the order of _run: encode, decode, DTX encode, noise estimator
    of both sides; and the blobs of the spans' streams and the lanes behind each."""
    if rate in _WANT:
        return _WANT[rate]
    import lyra_amd.codec as codec
    W = codec.span_warmup_frames("encoder")
    assert W == codec.span_warmup_frames("decoder")
    spans, frames = _job(W)
    twin = _ctx(rate=rate)
    ids = np.concatenate([[A, B, C], LANES]).astype(np.int32)
    w = dict(spans=spans, frames=frames, blobs={})
    w["pcm"] = {i: _audio_ext(golden_dir, n, rate, 300 + i) for (i, _, n) in spans}
    if rate == 16000:
        w["pk"] = {i: np.stack([twin.encode(h[None], BITS, [i])[0] for h in v]) if len(v) else np.zeros((0, BITS // 8), np.uint8)
                   for i, v in w["pcm"].items()}
    else:
        w["pk"], _ = _twin_encode_ext(twin, w["pcm"], rate, BITS)
    w["blobs"]["encode"] = twin.export_streams(ids)
    if rate == 16000:
        w["out"] = {i: np.stack([twin.decode(p[None], BITS, [i])[0] for p in v]) if len(v) else np.zeros((0, 320), np.int16)
                    for i, v in w["pk"].items()}
    else:
        w["out"], _ = _twin_decode_ext(twin, w["pk"], rate, BITS)
    w["blobs"]["decode"] = twin.export_streams(ids)
    w["dtx_pcm"] = {i: _audio_dtx(golden_dir, n, rate, 400 + i) for (i, _, n) in spans}
    w["dtx_pk"], w["dtx_nb"], _ = _twin_encode_ext(twin, w["dtx_pcm"], rate, BITS, dtx=True)
    assert 5 <= (w["dtx_nb"][C] > 0).sum() <= len(w["dtx_nb"][C]) - 5, "the DTX input needs both kinds of hop"
    w["blobs"]["dtx"] = twin.export_streams(ids)
    w["noise_pcm"] = {i: _audio_dtx(golden_dir, n, 16000, 500 + i) for (i, _, n) in spans}
    for side in ("encoder", "decoder"):
        w["noise_" + side] = {i: np.array([twin.noise_receive(h[None], [i], side=side)[0] for h in v], np.int32).reshape(-1, 1)
                              for i, v in w["noise_pcm"].items()}
        w["blobs"]["noise_" + side] = twin.export_streams(ids)
    twin.close()
    _WANT[rate] = w
    return w


def _rows(where, got, spans, want_by_id, zero=None):
    """rows of the spans equal the twin's (zero[id]: those rows are zeros instead); every other row still holds the filler"""
    _check_rows(where, got, spans, want_by_id, None if zero is None else {i: ~z for i, z in zero.items()}, skipped=0)


def _span_args(spans, lanes):
    import lyra_amd.codec as codec
    sp = codec._spans(spans)
    ln = np.ascontiguousarray(lanes, np.int32)
    return sp, ln, (sp.ctypes.data, sp.size, ln.ctypes.data, ln.size)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _encode(ctx, spans, lanes, rate, pcm, out):
    sp, ln, a = _span_args(spans, lanes)
    if rate == 16000:
        return ctx.L.lyra_hip_encode_spans(ctx.h, *a, _ptr(pcm), BITS, _ptr(out))
    return ctx.L.lyra_hip_encode_spans_ext(ctx.h, *a, _ptr(pcm), rate, BITS, _ptr(out))


def _decode(ctx, spans, lanes, rate, pk, out):
    sp, ln, a = _span_args(spans, lanes)
    if rate == 16000:
        return ctx.L.lyra_hip_decode_spans(ctx.h, *a, _ptr(pk), BITS, _ptr(out))
    return ctx.L.lyra_hip_decode_spans_ext(ctx.h, *a, _ptr(pk), BITS, rate, _ptr(out))


def _encode_dtx(ctx, spans, lanes, rate, pcm, out, nbytes):
    sp, ln, a = _span_args(spans, lanes)
    return ctx.L.lyra_hip_encode_spans_dtx(ctx.h, *a, _ptr(pcm), rate, BITS, _ptr(out), _ptr(nbytes))


def _noise(ctx, spans, side, pcm, out):
    import lyra_amd.codec as codec
    sp = codec._spans(spans)
    return ctx.L.lyra_hip_noise_spans(ctx.h, codec.SIDES[side], sp.ctypes.data, sp.size, _ptr(pcm), _ptr(out))


def _run(where, ctx, w, rate):
    """the five host forms on the spans of _job, each against the twin's rows and blobs"""
    spans, F, hop, nb = w["spans"], w["frames"], rate // 50, BITS // 8
    ids = np.concatenate([[A, B, C], LANES]).astype(np.int32)

    def state(stage):
        assert np.array_equal(ctx.export_streams(ids), w["blobs"][stage]), f"{where}: blobs after {stage}"

    pk = _filled(F, nb, np.uint8)
    assert _encode(ctx, spans, LANES, rate, _buffer(w["pcm"], spans, F), pk) == 0, ctx.last_error()
    _rows(where + " encode_spans", pk, spans, w["pk"])
    state("encode")
    out = _filled(F, hop, np.int16)
    assert _decode(ctx, spans, LANES, rate, _buffer(w["pk"], spans, F), out) == 0, ctx.last_error()
    _rows(where + " decode_spans", out, spans, w["out"])
    state("decode")
    pk, nbytes = _filled(F, nb, np.uint8), _filled(F, 1, np.int32)
    assert _encode_dtx(ctx, spans, LANES, rate, _buffer(w["dtx_pcm"], spans, F), pk, nbytes) == 0, ctx.last_error()
    _rows(where + " encode_spans_dtx packet_bytes", nbytes, spans, w["dtx_nb"])
    _rows(where + " encode_spans_dtx packets", pk, spans, w["dtx_pk"], zero={i: v == 0 for i, v in w["dtx_nb"].items()})
    state("dtx")
    for side in ("encoder", "decoder"):
        flags = _filled(F, 1, np.int32)
        assert _noise(ctx, spans, side, _buffer(w["noise_pcm"], spans, F), flags) == 0, ctx.last_error()
        _rows(f"{where} noise_spans({side})", flags, spans, w["noise_" + side])
        state("noise_" + side)


@pytest.mark.parametrize("rate", [16000, 48000])
def test_gaps_and_sentinels(golden_dir, rate):
    """Three streams, two lanes, a span of no frames, gaps in front of, between and behind the spans: rows outside the spans keep
    the filler, rows inside equal the hop-by-hop calls."""
    ctx = _ctx(rate=rate)
    _run(f"{rate} Hz", ctx, _want(golden_dir, rate), rate)
    ctx.close()


@pytest.mark.parametrize("rate", [16000, 48000])
def test_grow_after_small(golden_dir, rate):
    """One span of 3 frames and no lanes through every form, then the call of test_gaps_and_sentinels on the same context: the
    scratch of the span calls grows and the result is that of a fresh context."""
    ctx = _ctx(rate=rate)
    hop, nb, small = rate // 50, BITS // 8, [(SMALL, 0, 3)]
    pcm = _audio_ext(golden_dir, 3, rate, 7)
    pk = np.zeros((3, nb), np.uint8)
    assert _encode(ctx, small, [], rate, pcm, pk) == 0, ctx.last_error()
    assert _decode(ctx, small, [], rate, pk, np.zeros((3, hop), np.int16)) == 0, ctx.last_error()
    assert _encode_dtx(ctx, small, [], rate, pcm, pk, np.zeros(3, np.int32)) == 0, ctx.last_error()
    for side in ("encoder", "decoder"):
        assert _noise(ctx, small, side, _audio_ext(golden_dir, 3, 16000, 8), np.zeros(3, np.int32)) == 0, ctx.last_error()
    _run(f"{rate} Hz behind a small call", ctx, _want(golden_dir, rate), rate)
    ctx.close()


def test_nothing_to_do(golden_dir):
    """Spans without frames through the host forms and the `_dev` forms, with buffers and with null data pointers: 0, nothing
    written, every stream's and lane's blob as before.  packet_bytes of the DTX calls is required even then."""
    import torch
    import lyra_amd.codec as codec
    rate = 48000
    ctx = _ctx(rate=rate)
    dev = torch.device("cuda", 0)
    ids = np.concatenate([[A, B, C], LANES]).astype(np.int32)
    x = _audio_ext(golden_dir, 4, rate, 11)
    for h in x:   # streams A and C are not in the reset state, on either side
        p = ctx.encode_dtx(ctx.resample(np.stack([h, h]), rate, 16000, [A, C], side="encoder"), BITS, [A, C])[0]
        ctx.resample(ctx.decode(p, BITS, [A, C]), 16000, rate, [A, C], side="decoder")
    before = ctx.export_streams(ids)
    F, nb = 4, BITS // 8
    side_of = codec.SIDES
    L, h = ctx.L, ctx.h
    for null in (False, True):
        # a span without frames still names its first frame: the data pointers may be null only where that is frame 0
        spans = [(A, 0, 0), (B, 0, 0), (C, 0, 0)] if null else [(A, 0, 0), (B, 2, 0), (C, 4, 0)]
        sp, ln, a = _span_args(spans, LANES)

        def host(width, dtype):
            return None if null else _filled(F, width, dtype)
        nbytes = _filled(F, 1, np.int32)
        bufs = [host(320, np.int16), host(960, np.int16), host(nb, np.uint8), host(1, np.int32)]
        p16, p48, pk, flags = bufs
        assert _encode(ctx, spans, LANES, 16000, p16, pk) == 0, ctx.last_error()
        assert _decode(ctx, spans, LANES, 16000, pk, p16) == 0, ctx.last_error()
        assert _encode(ctx, spans, LANES, rate, p48, pk) == 0, ctx.last_error()
        assert _decode(ctx, spans, LANES, rate, pk, p48) == 0, ctx.last_error()
        assert _encode_dtx(ctx, spans, LANES, rate, p48, pk, nbytes) == 0, ctx.last_error()
        assert _encode_dtx(ctx, spans, LANES, rate, p48, pk, None) == -1   # LYRA_HIP_EINVAL
        for side in ("encoder", "decoder"):
            assert _noise(ctx, spans, side, p16, flags) == 0, ctx.last_error()
        for b in bufs + [nbytes]:
            assert b is None or (b.view(np.uint8) == FILL).all()

        def device(width, dtype):
            return None if null else gpu_plumbing._filled(dev, F, width, dtype)
        d_nbytes = gpu_plumbing._filled(dev, F, 1, np.int32)
        d_bufs = [device(320, np.int16), device(960, np.int16), device(nb, np.uint8), device(1, np.int32)]
        d16, d48, dpk, dflags = (None if t is None else t.data_ptr() for t in d_bufs)
        assert L.lyra_hip_encode_spans_dev(h, *a, d16, BITS, dpk) == 0, ctx.last_error()
        assert L.lyra_hip_decode_spans_dev(h, *a, dpk, BITS, d16) == 0, ctx.last_error()
        assert L.lyra_hip_encode_spans_ext_dev(h, *a, d48, rate, d16, BITS, dpk) == 0, ctx.last_error()
        assert L.lyra_hip_decode_spans_ext_dev(h, *a, dpk, BITS, rate, d16, d48) == 0, ctx.last_error()
        assert L.lyra_hip_encode_spans_dtx_dev(h, *a, d48, rate, d16, BITS, dpk, d_nbytes.data_ptr()) == 0, ctx.last_error()
        assert L.lyra_hip_encode_spans_dtx_dev(h, *a, d48, rate, d16, BITS, dpk, None) == -1
        for side in ("encoder", "decoder"):
            assert L.lyra_hip_noise_spans_dev(h, side_of[side], sp.ctypes.data, sp.size, d16, dflags) == 0, ctx.last_error()
        ctx.synchronize()
        for t in d_bufs + [d_nbytes]:
            assert t is None or (t.cpu().numpy().view(np.uint8) == FILL).all()
    assert np.array_equal(ctx.export_streams(ids), before)
    ctx.close()
