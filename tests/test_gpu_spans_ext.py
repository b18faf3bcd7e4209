"""lyra_hip_encode_spans_ext / lyra_hip_decode_spans_ext on the GPU (include/lyra_hip.h "Time-parallel spans"): spans at 8, 32
and 48 kHz, the resampler as ONE pass over all frames in front of the chunked steps (encode) or behind them (decode).  Every
comparison is BIT FOR BIT against the hop-by-hop calls on a twin context fed the same streams -- lyra_hip_resample(ENCODER) +
lyra_hip_encode, lyra_hip_decode + lyra_hip_resample(DECODER): packets, external-rate PCM, the 16 kHz workspace, the span
streams' exported state (resampler slots included) and the lanes' state against a fresh stream's."""
import os
import subprocess
import wave

import numpy as np
import pytest

from gpu_plumbing import FILL, _filled, make_ctx
from signals import _audio_ext as _audio
from span_cases import (_check_rows, _check_state, _in_pos_offsets, _layout, _twin_decode_ext as _twin_decode,
                        _twin_encode_ext as _twin_encode)

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MAX_STREAMS = 96


def _ctx(mode="xnnpack"):
    return make_ctx(MAX_STREAMS, mode)


@pytest.mark.parametrize("rate,num_bits,mode", [(8000, 64, "xnnpack"), (32000, 120, "xnnpack"), (48000, 184, "xnnpack"),
                                                (48000, 120, "builtin_mixed")])
def test_spans_at_other_rates_equal_hop_by_hop_calls(golden_dir, rate, num_bits, mode):
    """Span lengths 0, 1, W, W + 18 and 350 in one call with 40 lanes; two pairs of spans touch in the buffer (frame 0 of the
    second must take its history from its stream's slot, not from the rows in front), the others lie behind filler rows."""
    import torch
    import lyra_amd.codec as codec
    W = codec.span_warmup_frames("encoder")
    ctx, twin = _ctx(mode), _ctx(mode)
    dev = torch.device("cuda", 0)
    hop, nb = rate // 50, (num_bits + 7) // 8
    lengths = {7: 350, 11: 1, 3: 0, 20: W, 5: W + 18}
    gaps = [2, 0, 3, 3, 0]
    ext = {i: _audio(golden_dir, n, rate, 100 + i) for i, n in lengths.items()}
    lanes = np.arange(24, 24 + 40, dtype=np.int32)
    where = f"{mode}/{rate}/{num_bits}"
    # encoder
    want_pk, want_e16 = _twin_encode(twin, ext, rate, num_bits)
    spans, buf = _layout(ext, gaps)
    F = len(buf)
    d_ext, d_p16, d_pk = torch.from_numpy(buf).to(dev), _filled(dev, F, 320, np.int16), _filled(dev, F, nb, np.uint8)
    ctx.encode_spans_dev(spans, d_ext, num_bits, d_pk, lanes, sample_rate_hz=rate, d_pcm16=d_p16)
    ctx.synchronize()
    _check_rows(where + " packets", d_pk.cpu().numpy(), spans, want_pk)
    _check_rows(where + " resampled input", d_p16.cpu().numpy(), spans, want_e16)
    assert np.array_equal(d_ext.cpu().numpy(), buf), f"{where}: the input buffer was written"
    _check_state(where + " after encode", ctx, twin, list(lengths), lanes)
    # decoder
    want_ext, want_d16 = _twin_decode(twin, want_pk, rate, num_bits)
    spans, buf = _layout(want_pk, gaps)
    d_pk, d_p16, d_out = torch.from_numpy(buf).to(dev), _filled(dev, F, 320, np.int16), _filled(dev, F, hop, np.int16)
    ctx.decode_spans_dev(spans, d_pk, num_bits, d_out, lanes, sample_rate_hz=rate, d_pcm16=d_p16)
    ctx.synchronize()
    _check_rows(where + " pcm", d_out.cpu().numpy(), spans, want_ext)
    _check_rows(where + " 16 kHz pcm", d_p16.cpu().numpy(), spans, want_d16)
    assert np.array_equal(d_pk.cpu().numpy(), buf), f"{where}: the packet buffer was written"
    _check_state(where + " after decode", ctx, twin, list(lengths), lanes)


def test_span_continues_a_live_stream_is_continued_and_keeps_a_decimation_phase(golden_dir):
    """48 kHz, host forms: k hops hop by hop, a span, more hops -- packets, PCM and blobs equal throughout.  Then the same
    stream with a decimation phase no call sequence reaches but a blob may carry (RS_IN_POS in 1..5, accepted by import):
    encoder 48 kHz -> 16 kHz with in_pos 4 (phase 1 of 3), decoder 16 kHz -> 8 kHz with in_pos 3 (phase 1 of 2)."""
    ctx, twin = _ctx(), _ctx()
    sid, k, n, tail, bits, rate = 13, 7, 300, 6, 120, 48000
    lanes = np.arange(30, 30 + 40, dtype=np.int32)
    x = _audio(golden_dir, k + n + tail, rate, 5)
    want_pk = _twin_encode(twin, {sid: x}, rate, bits)[0][sid]
    want_pcm = _twin_decode(twin, {sid: want_pk}, rate, bits)[0][sid]
    head = _twin_encode(ctx, {sid: x[:k]}, rate, bits)[0][sid]
    mid = ctx.encode_spans([(sid, k, n)], x, bits, lanes, sample_rate_hz=rate)
    assert not mid[:k].any() and not mid[k + n:].any()
    rest = _twin_encode(ctx, {sid: x[k + n:]}, rate, bits)[0][sid]
    got = np.concatenate([head, mid[k:k + n], rest])
    assert np.array_equal(got, want_pk), np.flatnonzero((got != want_pk).any(axis=1))[:8]
    head = _twin_decode(ctx, {sid: want_pk[:k]}, rate, bits)[0][sid]
    mid = ctx.decode_spans([(sid, k, n)], want_pk, bits, lanes, sample_rate_hz=rate)
    assert not mid[:k].any() and not mid[k + n:].any()
    rest = _twin_decode(ctx, {sid: want_pk[k + n:]}, rate, bits)[0][sid]
    got = np.concatenate([head, mid[k:k + n], rest])
    assert np.array_equal(got, want_pcm), np.flatnonzero((got != want_pcm).any(axis=1))[:8]
    _check_state("continued stream", ctx, twin, [sid], lanes)
    # a phase other than 0
    off_e, off_d = _in_pos_offsets(ctx, 90)
    blob = ctx.export_streams([sid])
    # so far only what hops leave: 960 in per hop is 0 mod 6 on the encoder, 320 in per hop is 2 mod 6 on the decoder
    assert blob[0, off_e] == 0 and blob[0, off_d] == (k + n + tail) * 320 % 6
    blob[0, off_e], blob[0, off_d] = 4, 3
    for c in (ctx, twin):
        c.import_streams([sid], blob)
    n = 120
    y = _audio(golden_dir, n + 2, rate, 6)
    want_pk = _twin_encode(twin, {sid: y}, rate, bits)[0][sid]
    got = np.concatenate([ctx.encode_spans([(sid, 0, n)], y[:n], bits, lanes, sample_rate_hz=rate),
                          _twin_encode(ctx, {sid: y[n:]}, rate, bits)[0][sid]])
    assert np.array_equal(got, want_pk), np.flatnonzero((got != want_pk).any(axis=1))[:8]
    want_pcm = _twin_decode(twin, {sid: want_pk}, 8000, bits)[0][sid]
    got = np.concatenate([ctx.decode_spans([(sid, 0, n)], want_pk[:n], bits, lanes, sample_rate_hz=8000),
                          _twin_decode(ctx, {sid: want_pk[n:]}, 8000, bits)[0][sid]])
    assert np.array_equal(got, want_pcm), np.flatnonzero((got != want_pcm).any(axis=1))[:8]
    after = ctx.export_streams([sid])
    assert after[0, off_e] == (4 + (n + 2) * 960) % 6 and after[0, off_d] == (3 + (n + 2) * 320) % 6
    _check_state("non-zero phase", ctx, twin, [sid], lanes)


def test_16000_through_the_ext_calls_is_the_plain_span_call(golden_dir):
    """rate 16000: no 16 kHz buffer (NULL), no resampler slot read or written -- they are dirtied first, alike on both."""
    import lyra_amd.codec as codec
    ctx, twin = _ctx(), _ctx()
    bits, lanes = 184, np.arange(40, 60, dtype=np.int32)
    x = _audio(golden_dir, 200, 16000, 9)
    for c in (ctx, twin):
        c.resample(_audio(golden_dir, 1, 48000, 3), 48000, 16000, [2], side="encoder")
        c.resample(x[:1], 16000, 32000, [2], side="decoder")
    sp = codec._spans([(2, 1, 199)])
    want_pk = twin.encode_spans(sp, x, bits, lanes)
    pk = np.zeros_like(want_pk)
    ctx._chk(ctx.L.lyra_hip_encode_spans_ext(ctx.h, sp.ctypes.data, sp.size, lanes.ctypes.data, lanes.size, x.ctypes.data, 16000,
                                             bits, pk.ctypes.data))
    assert np.array_equal(pk, want_pk)
    want = twin.decode_spans(sp, want_pk, bits, lanes)
    out = np.zeros_like(want)
    ctx._chk(ctx.L.lyra_hip_decode_spans_ext(ctx.h, sp.ctypes.data, sp.size, lanes.ctypes.data, lanes.size, pk.ctypes.data, bits,
                                             16000, out.ctypes.data))
    assert np.array_equal(out, want)
    _check_state("16000", ctx, twin, [2], lanes)
    # and the Python forms pick the plain call themselves
    assert np.array_equal(ctx.encode_spans([(2, 0, 1)], x[:1], bits, (), sample_rate_hz=16000), twin.encode_spans([(2, 0, 1)], x[:1], bits))


def test_dev_form_refusals_change_nothing(golden_dir):
    """LYRA_HIP_EINVAL with nothing enqueued: a rate that is no codec rate, a missing or misaligned 16 kHz buffer at 48 kHz,
    id sets the planner refuses."""
    import torch
    import lyra_amd.codec as codec
    ctx = _ctx()
    dev = torch.device("cuda", 0)
    F, rate, bits = 60, 48000, 184
    lanes = np.arange(1, 9, dtype=np.int32)
    d_ext = torch.from_numpy(_audio(golden_dir, F, rate, 8)).to(dev)
    d_cd = _filled(dev, F, 882, np.int16)   # rows of 44100 / 50 samples
    d_p16, d_pk, d_out = _filled(dev, F, 320, np.int16), _filled(dev, F, 23, np.uint8), _filled(dev, F, 960, np.int16)
    d_odd = _filled(dev, F + 1, 320, np.int16).view(-1)[1:1 + F * 320].view(F, 320)   # 2 bytes off a 16-byte boundary
    assert d_odd.data_ptr() % 16 == 2 and d_odd.is_contiguous()
    ctx.resample(_audio(golden_dir, 1, rate, 2), rate, 16000, [0], side="encoder")   # a slot that is not the reset state
    before = ctx.export_streams(np.arange(0, 9))
    ok = [(0, 0, F)]
    cases = [(ok, d_cd, 44100, d_p16, d_cd, lanes), (ok, d_ext, rate, None, d_out, lanes), (ok, d_ext, rate, d_odd, d_out, lanes),
             (ok, d_ext, rate, d_p16, d_out, [0]), (ok, d_ext, rate, d_p16, d_out, [5, 5]),
             ([(0, 0, F), (0, 0, 10)], d_ext, rate, d_p16, d_out, lanes), ([(MAX_STREAMS, 0, F)], d_ext, rate, d_p16, d_out, lanes)]
    for spans, d_in, r, p16, d_o, ln in cases:
        with pytest.raises(codec.LyraHipError):
            ctx.encode_spans_dev(spans, d_in, bits, d_pk, ln, sample_rate_hz=r, d_pcm16=p16)
        with pytest.raises(codec.LyraHipError):
            ctx.decode_spans_dev(spans, d_pk, bits, d_o, ln, sample_rate_hz=r, d_pcm16=p16)
    ctx.synchronize()
    assert np.array_equal(ctx.export_streams(np.arange(0, 9)), before)
    for t in (d_p16, d_pk, d_out, d_cd, d_odd):
        assert (t.cpu().numpy().view(np.uint8) == FILL).all()


def test_file_functions_give_the_same_bytes_at_48_khz(golden_dir, tmp_path):
    """file_demo on 48 kHz WAVs, decoded at 48 kHz: --time-parallel=64 against hop by hop."""
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "file_demo")
    assert os.path.exists(demo), "lyra_amd/file_demo not built (__graft_entry__.build())"
    files = {"long": 1900 * 960 + 17, "short": 40 * 960, "tiny": 100, "mid": 611 * 960 + 957}
    wavs = []
    for k, (name, n) in enumerate(files.items()):
        pcm = _audio(golden_dir, n // 960 + 1, 48000, 40 + k).reshape(-1)[:n]
        with wave.open(str(tmp_path / f"{name}.wav"), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(48000)
            w.writeframes(pcm.tobytes())
        wavs.append(str(tmp_path / f"{name}.wav"))
    outs = {}
    for flag in ((), ("--time-parallel=64",)):
        out_dir = tmp_path / ("tp" if flag else "seq")
        out_dir.mkdir()
        r = subprocess.run([demo, *flag, "--decode-rate=48000", lyra_amd.default_model_dir(), "6000", str(out_dir)] + wavs,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (flag, r.returncode, r.stderr[-2000:])
        outs[bool(flag)] = out_dir
    for name, n in files.items():
        for suffix in (".lyra", "_decoded.wav"):
            a = (outs[False] / (name + suffix)).read_bytes()
            b = (outs[True] / (name + suffix)).read_bytes()
            assert a == b, (name, suffix, len(a), len(b))
        assert len((outs[True] / (name + ".lyra")).read_bytes()) == (n // 960) * 15
        with wave.open(str(outs[True] / (name + "_decoded.wav")), "rb") as w:
            assert w.getframerate() == 48000 and w.getnframes() == (n // 960) * 960
