"""lyra_hip_encode_spans_dtx / lyra_hip_noise_spans on the GPU (include/lyra_hip.h "Time-parallel spans", DTX): the encoder's
NoiseEstimator over whole spans in front of the chunked steps, the steps on the compacted list of non-noise hops.  Every
comparison is BIT FOR BIT against the hop-by-hop calls on a twin context fed the same streams -- lyra_hip_resample(ENCODER) +
lyra_hip_encode_dtx, lyra_hip_noise_receive: packets, packet sizes, the 16 kHz workspace, the span streams' exported state
(estimator and resampler slots included) and the lanes' state against a fresh stream's.

The input is golden speech with stretches zeroed and stretches of low-level noise, so the non-noise hops are not contiguous.
What the tests need of it is asserted on the TWIN's output before anything is compared (_assert_input): every span longer
than W has at least 20 empty packets and at least 4 noise <-> non-noise transitions; every span that can hold them (n >= 20 +
hops_per_update + 10 -- the 350-frame span; W + 18 = 43 frames cannot hold 20 empty and hops_per_update + 10 >= 35 non-empty
packets at any rate) has at least hops_per_update + 10 non-empty packets, the shorter ones at least 15; and in the 350-frame
span a transition lies inside a lane chunk's warm-up."""
import os
import subprocess
import wave

import numpy as np
import pytest

from gpu_plumbing import FILL, _filled, make_ctx
import span_cases
from signals import _audio_dtx as _audio
from span_cases import _check_rows, _check_state, _layout

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MAX_STREAMS = 96


def _ctx(mode="xnnpack", rate=16000):
    return make_ctx(MAX_STREAMS, mode, rate)


def _twin_encode(twin, ext_by_id, rate, num_bits):
    return span_cases._twin_encode_ext(twin, ext_by_id, rate, num_bits, dtx=True)


def _assert_input(where, sizes_by_id, W, rate, long_id, lanes):
    """the conditions on the input (module docstring), on the twin's packet sizes"""
    import lyra_amd.codec as codec
    hpu = round(rate / 320)
    for i, nb in sizes_by_id.items():
        n, active = len(nb), nb > 0
        if n <= W:
            continue
        trans = int(np.count_nonzero(active[1:] != active[:-1]))
        need = hpu + 10 if n >= 20 + hpu + 10 else 15
        assert n - active.sum() >= 20 and active.sum() >= need and trans >= 4, (where, i, n, int(active.sum()), trans)
    region, compact = 0, []   # what the call hands its planner: the spans' non-noise hops, a region per span
    for i, nb in sizes_by_id.items():
        compact.append((i, region, int((nb > 0).sum())))
        region += len(nb)
    chunks, _ = codec.spans_plan("encoder", compact, lanes, MAX_STREAMS)
    k = list(sizes_by_id).index(long_id)
    at = np.flatnonzero(sizes_by_id[long_id] > 0)   # compacted index -> frame of the span
    first = [int(c["first_frame"]) - compact[k][1] for c in chunks if c["span"] == k and c["n_warmup"] > 0]
    assert first, (where, "the long span is not cut")
    # a warm-up of W compacted hops that is not W consecutive frames holds a noise stretch, i.e. two transitions
    assert any(at[f] - at[f - W] > W for f in first), (where, "no transition in a warm-up")


@pytest.mark.parametrize("rate,num_bits,mode", [(16000, 184, "xnnpack"), (8000, 64, "xnnpack"), (48000, 120, "xnnpack"),
                                                (16000, 120, "builtin_mixed")])
def test_one_call_of_mixed_span_lengths_equals_hop_by_hop_dtx(golden_dir, rate, num_bits, mode):
    """Span lengths 0, 1, 2, W, W + 18 and 350 in one call with 40 lanes; two pairs of spans touch in the buffer; the span of
    2 frames is silence on a stream whose estimator already knows silence: no active frame, no chunk."""
    import torch
    import lyra_amd.codec as codec
    W = codec.span_warmup_frames("encoder")
    ctx, twin = _ctx(mode, rate), _ctx(mode, rate)
    dev = torch.device("cuda", 0)
    hop, nb = rate // 50, (num_bits + 7) // 8
    lengths = {7: 350, 11: 1, 3: 0, 20: W, 5: W + 18, 9: 2}
    gaps = [2, 0, 3, 3, 0, 1]
    ext = {i: _audio(golden_dir, n, rate, 200 + i) for i, n in lengths.items()}
    ext[9][:] = 0
    silence = np.zeros((3, hop), np.int16)
    for c in (ctx, twin):   # stream 9 has heard three hops of silence
        _twin_encode(c, {9: silence}, rate, num_bits)
    lanes = np.arange(24, 24 + 40, dtype=np.int32)
    where = f"{mode}/{rate}/{num_bits}"
    want_pk, want_nb, want_e16 = _twin_encode(twin, ext, rate, num_bits)
    _assert_input(where, want_nb, W, rate, 7, lanes)
    assert not want_nb[9].any(), (where, "the silent span has active frames")
    if rate == 48000:
        assert (want_nb[7] > 0).sum() > 150
    spans, buf = _layout(ext, gaps)
    F = len(buf)
    d_ext, d_p16 = torch.from_numpy(buf).to(dev), _filled(dev, F, 320, np.int16)
    d_pk, d_nb = _filled(dev, F, nb, np.uint8), _filled(dev, F, 1, np.int32).view(-1)
    ctx.encode_spans_dtx_dev(spans, d_ext, num_bits, d_pk, d_nb, lanes, sample_rate_hz=rate,
                             d_pcm16=d_p16 if rate != 16000 else None)
    ctx.synchronize()
    _check_rows(where + " packet_bytes", d_nb.cpu().numpy().reshape(F, 1), spans, want_nb)
    _check_rows(where + " packets", d_pk.cpu().numpy(), spans, want_pk, written={i: v > 0 for i, v in want_nb.items()})
    if rate != 16000:
        _check_rows(where + " resampled input", d_p16.cpu().numpy(), spans, want_e16)
    else:
        assert (d_p16.cpu().numpy().view(np.uint8) == FILL).all()
    assert np.array_equal(d_ext.cpu().numpy(), buf), f"{where}: the input buffer was written"
    _check_state(where, ctx, twin, list(lengths), lanes)
    if (rate, num_bits, mode) == (16000, 184, "xnnpack"):   # and the CPU restatement of LyraEncoder with DTX
        from oracle import lyra_oracle
        from oracle.lyra_codec_model import RefLyraEncoder
        lyra_oracle.build()
        O = lyra_oracle.Oracle(mode=mode)
        got = d_pk.cpu().numpy()
        for (i, first, n) in spans:
            if i not in (5, 20):   # fresh streams; the long span is held to the twin, which test_gpu_parity holds to the oracle
                continue
            enc = RefLyraEncoder(O, rate, num_bits, enable_dtx=True)
            for h in range(n):
                p = enc.Encode(ext[i][h])
                assert p.size == want_nb[i][h], (i, h, p.size)
                assert p.size == 0 or np.array_equal(p, got[first + h]), (i, h)


@pytest.mark.parametrize("n_lanes", [40, 0])
def test_span_continues_a_live_dtx_stream_and_is_continued(golden_dir, n_lanes):
    """37 hops hop by hop with DTX (estimator initialised, hops mid-period), a span of 200, 30 more hops hop by hop: all equal
    the twin that went hop by hop throughout.  n_lanes = 0: the sequential fallback."""
    ctx, twin = _ctx(), _ctx()
    sid, k, n, tail, bits = 13, 37, 200, 30, 120
    lanes = np.arange(30, 30 + n_lanes, dtype=np.int32)
    x = _audio(golden_dir, k + n + tail, 16000, 5)
    want_pk, want_nb, _ = _twin_encode(twin, {sid: x}, 16000, bits)
    assert 20 <= (want_nb[sid][k:k + n] > 0).sum() <= n - 20
    head = _twin_encode(ctx, {sid: x[:k]}, 16000, bits)
    mid_pk, mid_nb = ctx.encode_spans_dtx([(sid, k, n)], x, bits, lanes)
    assert not mid_pk[:k].any() and not mid_pk[k + n:].any() and not mid_nb[:k].any() and not mid_nb[k + n:].any()
    rest = _twin_encode(ctx, {sid: x[k + n:]}, 16000, bits)
    got_pk = np.concatenate([head[0][sid], mid_pk[k:k + n], rest[0][sid]])
    got_nb = np.concatenate([head[1][sid], mid_nb[k:k + n], rest[1][sid]])
    assert np.array_equal(got_nb, want_nb[sid]), np.flatnonzero(got_nb != want_nb[sid])[:8]
    assert np.array_equal(got_pk, want_pk[sid]), np.flatnonzero((got_pk != want_pk[sid]).any(axis=1))[:8]
    _check_state("continued stream", ctx, twin, [sid], lanes)


@pytest.mark.parametrize("side,enc_rate", [("encoder", 32000), ("decoder", 16000)])
def test_noise_spans_equals_noise_receive_per_hop(golden_dir, side, enc_rate):
    """Lengths 1, 2, 3 and 120, two spans touch; the encoder side with the constants and filterbank of a 32 kHz encoder."""
    ctx, twin = _ctx(rate=enc_rate), _ctx(rate=enc_rate)
    pcm = {4: _audio(golden_dir, 120, 16000, 31), 8: _audio(golden_dir, 1, 16000, 32), 2: _audio(golden_dir, 2, 16000, 33),
           17: _audio(golden_dir, 3, 16000, 34)}
    spans, buf = _layout(pcm, [1, 0, 2, 0])
    want = {i: np.array([twin.noise_receive(h[None], [i], side=side)[0] for h in v], np.int32) for i, v in pcm.items()}
    assert 10 <= want[4].sum() <= 110   # both kinds of hop
    got = ctx.noise_spans(spans, buf, side=side)
    covered = np.zeros(len(buf), bool)
    for (i, first, n) in spans:
        covered[first:first + n] = True
        assert np.array_equal(got[first:first + n], want[i]), (side, i, np.flatnonzero(got[first:first + n] != want[i])[:8])
    assert not got[~covered].any()
    ids = list(pcm)
    assert np.array_equal(ctx.noise_estimate(ids, side=side).view(np.uint32), twin.noise_estimate(ids, side=side).view(np.uint32))
    assert np.array_equal(ctx.export_streams(ids), twin.export_streams(ids))


def test_refusals_change_nothing(golden_dir):
    """LYRA_HIP_EINVAL before the first kernel: the estimator slots, like everything else, stay as they were."""
    import torch
    import lyra_amd.codec as codec
    ctx, twin = _ctx(rate=48000), _ctx(rate=48000)
    dev = torch.device("cuda", 0)
    F, rate, bits = 60, 48000, 184
    lanes = np.arange(1, 9, dtype=np.int32)
    x = _audio(golden_dir, F, rate, 8)
    d_ext = torch.from_numpy(x).to(dev)
    d_p16, d_pk, d_nb = _filled(dev, F, 320, np.int16), _filled(dev, F, 23, np.uint8), _filled(dev, F, 1, np.int32).view(-1)
    d_odd = _filled(dev, F + 1, 960, np.int16).view(-1)[1:1 + F * 960].view(F, 960)   # 2 bytes off a 16-byte boundary
    assert d_odd.data_ptr() % 16 == 2 and d_odd.is_contiguous()
    for c in (ctx, twin):   # slots that are not the reset state
        _twin_encode(c, {0: x[:3]}, rate, bits)
    before = ctx.export_streams(np.arange(0, 9))
    ok = [(0, 0, F)]
    d_16 = _filled(dev, F, 320, np.int16)
    # null d_packet_bytes | rate != encoder rate | bad bit counts | overlapping spans | a lane that is also a span id | misaligned PCM
    cases = [dict(d_nb=None), dict(rate=16000, d_in=d_16), dict(bits=186), dict(bits=0), dict(spans=[(0, 0, F), (9, 10, 5)]),
             dict(lanes=[0, 1]), dict(d_in=d_odd)]
    for case in cases:
        sp = codec._spans(case.get("spans", ok))
        ln = np.asarray(case.get("lanes", lanes), np.int32)
        nb_t = case.get("d_nb", d_nb)
        rc = ctx.L.lyra_hip_encode_spans_dtx_dev(ctx.h, sp.ctypes.data, sp.size, ln.ctypes.data, ln.size,
                                                 case.get("d_in", d_ext).data_ptr(), case.get("rate", rate), d_p16.data_ptr(),
                                                 case.get("bits", bits), d_pk.data_ptr(), nb_t.data_ptr() if nb_t is not None else None)
        assert rc == -1, (case.keys(), rc)   # LYRA_HIP_EINVAL
    ctx.synchronize()
    assert np.array_equal(ctx.export_streams(np.arange(0, 9)), before)
    for t in (d_p16, d_pk, d_nb, d_16):
        assert (t.cpu().numpy().view(np.uint8) == FILL).all()
    want_pk, want_nb, want_e16 = _twin_encode(twin, {0: x}, rate, bits)
    ctx.encode_spans_dtx_dev(ok, d_ext, bits, d_pk, d_nb, lanes, sample_rate_hz=rate, d_pcm16=d_p16)
    ctx.synchronize()
    assert np.array_equal(d_nb.cpu().numpy(), want_nb[0])
    on = want_nb[0] > 0
    assert np.array_equal(d_pk.cpu().numpy()[on], want_pk[0][on]) and np.array_equal(d_p16.cpu().numpy(), want_e16[0])
    _check_state("after the refusals", ctx, twin, [0], lanes)


def _file_demo(tmp_path, golden_dir, rate, seconds):
    """file_demo --dtx hop by hop and --time-parallel=64 on one WAV: (wav path, the two .lyra files' bytes)"""
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "file_demo")
    assert os.path.exists(demo), "lyra_amd/file_demo not built (__graft_entry__.build())"
    n = seconds * rate + 37
    pcm = _audio(golden_dir, n // (rate // 50) + 1, rate, 77).reshape(-1)[:n]
    wav = str(tmp_path / "talk.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(pcm.tobytes())
    out = []
    for flag in ((), ("--time-parallel=64",)):
        out_dir = tmp_path / ("tp" if flag else "seq")
        out_dir.mkdir()
        r = subprocess.run([demo, *flag, "--dtx", lyra_amd.default_model_dir(), "6000", str(out_dir), wav],
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (flag, r.returncode, r.stderr[-2000:])
        assert not (out_dir / "talk_decoded.wav").exists()
        out.append((out_dir / "talk.lyra").read_bytes())
    return wav, out[0], out[1]


@pytest.mark.parametrize("rate", [16000, 48000])
def test_file_demo_dtx_time_parallel_and_hop_by_hop_write_the_same_file(golden_dir, tmp_path, rate):
    """12 s: the files are byte-identical, a whole number of packets, and shorter than without DTX but not empty."""
    _, seq, tp = _file_demo(tmp_path, golden_dir, rate, 12)
    assert seq == tp, (len(seq), len(tp))
    assert len(seq) % 15 == 0 and 100 * 15 <= len(seq) <= (12 * 50 - 100) * 15, len(seq)


def test_file_demo_dtx_equals_the_reference_encode_file(golden_dir, tmp_path, oracle_default):
    """16 kHz: the reference's own EncodeFile with enable_dtx (oracle/_ref, where it is built)."""
    from oracle import lyra_ref
    if not lyra_ref.available():
        pytest.skip("oracle/_ref/liblyra_ref.so not built (needs /root/reference at build time)")
    lyra_ref.load(oracle_default)
    wav, seq, tp = _file_demo(tmp_path, golden_dir, 16000, 12)
    model_dir = lyra_ref.make_model_dir(str(tmp_path / "model"))
    ref_out = str(tmp_path / "ref.lyra")
    assert lyra_ref.encode_file(oracle_default, wav, ref_out, 6000, model_dir, enable_dtx=True)
    ref = open(ref_out, "rb").read()
    assert tp == ref and seq == ref, (len(tp), len(seq), len(ref))
