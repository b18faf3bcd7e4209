"""lyra_hip_encode_spans / lyra_hip_decode_spans on the GPU (include/lyra_hip.h "Time-parallel spans"): long spans cut into
chunks that run side by side behind a discarded warm-up.  Every comparison is BIT FOR BIT against the hop-by-hop calls
lyra_hip_encode / lyra_hip_decode on a twin context fed the same streams: packets, PCM, the span streams' exported state,
and the lanes' state against a freshly reset stream's.  One case holds the packets against the CPU oracle directly, one the
whole-file functions against EncodeFiles / DecodeFiles.

Stream kind: the contexts here (96 streams) run on the CU-masked streams the library picks up to 1,024 streams, which are
blocking streams with respect to the NULL stream; the case with streams="plain" runs on hipStreamNonBlocking streams, the kind
of a 4,096-stream context (tests/gpu_plumbing.py make_ctx)."""
import os
import subprocess
import wave

import numpy as np
import pytest

from gpu_plumbing import make_ctx, stream_cases
from signals import _audio_spans as _audio
import span_cases
from span_cases import _check_state, _sequential

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MAX_STREAMS = 96


def _ctx(mode="xnnpack", max_streams=MAX_STREAMS, streams=None):
    return make_ctx(max_streams, mode, streams=streams)


def _layout(rows_by_id, gap=3):
    return span_cases._layout(rows_by_id, gap, tail=0)


def _round_trip(where, ctx, twin, pcm_by_id, num_bits, lanes, lanes_dirty=False):
    """encode spans, decode spans from the produced packets, against the twin hop by hop; state checks after each side
    (lanes that came in dirty on both sides are whole again only after both calls)"""
    ids = list(pcm_by_id)
    want_pk = _sequential(twin, pcm_by_id, num_bits, True)
    spans, buf = _layout(pcm_by_id)
    pk = ctx.encode_spans(spans, buf, num_bits, lanes)
    for (i, first, n) in spans:
        got = pk[first:first + n]
        diff = np.flatnonzero((got != want_pk[i]).any(axis=1)) if n else []
        assert len(diff) == 0, f"{where}: packets of stream {i} differ at hops {list(diff[:8])} of {n}"
    _check_state(where + " after encode", ctx, twin, ids, [] if lanes_dirty else lanes)
    want_pcm = _sequential(twin, want_pk, num_bits, False)
    spans, buf = _layout(want_pk)
    out = ctx.decode_spans(spans, buf, num_bits, lanes)
    for (i, first, n) in spans:
        got = out[first:first + n]
        diff = np.flatnonzero((got != want_pcm[i]).any(axis=1)) if n else []
        assert len(diff) == 0, f"{where}: PCM of stream {i} differs at hops {list(diff[:8])} of {n}"
    covered = np.zeros(len(out), bool)
    for (_, first, n) in spans:
        covered[first:first + n] = True
    assert not out[~covered].any(), f"{where}: rows outside every span were written"
    _check_state(where + " after decode", ctx, twin, ids, lanes)
    return want_pk, want_pcm


@pytest.mark.parametrize("num_bits", [64, 120, 184])
@pytest.mark.parametrize("mode", ["exact", "gemmlowp_double", "xnnpack", "builtin_mixed"])
def test_spans_equal_hop_by_hop_calls(golden_dir, mode, num_bits):
    """Span lengths 0, 1, W, W + 18 and a few thousand with a ragged last chunk, all in ONE call with many lanes."""
    import lyra_amd.codec as codec
    W = codec.span_warmup_frames("encoder")
    assert W == codec.span_warmup_frames("decoder")
    ctx, twin = _ctx(mode), _ctx(mode)
    lengths = {7: 2611, 3: 0, 11: 1, 20: W, 5: W + 18, 1: 333}
    pcm = {i: _audio(golden_dir, n, 100 + i) for i, n in lengths.items()}
    lanes = np.array([i for i in range(24, 24 + 61)], np.int32)
    chunks, steps = codec.spans_plan("encoder", _layout(pcm)[0], lanes, MAX_STREAMS)
    assert steps < 120 and len(set(int(c["n_frames"]) for c in chunks if c["n_warmup"])) > 1, "ragged chunks wanted"
    _round_trip(f"{mode}/{num_bits}", ctx, twin, pcm, num_bits, lanes)


@pytest.mark.parametrize("n_lanes,streams", stream_cases([0, 1, 37], plain=37))
def test_lane_counts(golden_dir, n_lanes, streams):
    """n_lanes = 0 runs the spans sequentially on their own ids; 1 and many cut them.  The lanes come in DIRTY."""
    ctx, twin = _ctx(streams=streams), _ctx(streams=streams)
    pcm = {4: _audio(golden_dir, 700, 1), 9: _audio(golden_dir, 410, 2)}
    lanes = np.arange(40, 40 + n_lanes, dtype=np.int32)
    if n_lanes:   # whatever a lane held is lost: run some hops on them first, on both sides
        junk = _audio(golden_dir, 5, 77)
        for h in range(5):
            pk = ctx.encode(np.repeat(junk[h][None], n_lanes, 0), 184, lanes)
            ctx.decode(pk, 184, lanes)
    _round_trip(f"lanes={n_lanes}", ctx, twin, pcm, 184, lanes, lanes_dirty=True)


def test_span_continues_a_live_stream_and_is_continued(golden_dir):
    """k sequential hops, a span, more sequential hops: packets and PCM stay equal throughout, the exported state is
    byte-identical, and the regions that are not the codec's (log-mel history, both noise estimators, both resamplers,
    comfort noise) keep what they held -- they are dirtied first, the same way on both contexts."""
    ctx, twin = _ctx(), _ctx()
    sid, k, n, tail, bits = 13, 31, 1500, 20, 120
    x = _audio(golden_dir, k + n + tail, 5)
    lanes = np.arange(30, 30 + 50, dtype=np.int32)
    for c in (ctx, twin):
        c.logmel(x[:1], [sid])
        c.noise_receive(x[1:2], [sid], side="encoder")
        c.noise_receive(x[2:3], [sid], side="decoder")
        c.resample(np.tile(x[3], 3)[None], 48000, 16000, [sid], side="encoder")
        c.resample(x[4:5], 16000, 48000, [sid], side="decoder")
    want_pk = _sequential(twin, {sid: x}, bits, True)[sid]
    want_pcm = _sequential(twin, {sid: want_pk}, bits, False)[sid]
    # encoder
    head = _sequential(ctx, {sid: x[:k]}, bits, True)[sid]
    mid = ctx.encode_spans([(sid, k, n)], x, bits, lanes)[k:k + n]
    rest = _sequential(ctx, {sid: x[k + n:]}, bits, True)[sid]
    got = np.concatenate([head, mid, rest])
    assert np.array_equal(got, want_pk), np.flatnonzero((got != want_pk).any(axis=1))[:8]
    # decoder
    head = _sequential(ctx, {sid: want_pk[:k]}, bits, False)[sid]
    mid = ctx.decode_spans([(sid, k, n)], want_pk, bits, lanes)[k:k + n]
    rest = _sequential(ctx, {sid: want_pk[k + n:]}, bits, False)[sid]
    got = np.concatenate([head, mid, rest])
    assert np.array_equal(got, want_pcm), np.flatnonzero((got != want_pcm).any(axis=1))[:8]
    _check_state("continued stream", ctx, twin, [sid], lanes)


def test_dev_form_and_refusals(golden_dir):
    """The `_dev` forms on torch buffers (no synchronisation inside; encode -> decode ordered by the library), and
    LYRA_HIP_EINVAL with nothing changed for id sets the planner refuses."""
    import torch
    import lyra_amd.codec as codec
    ctx, twin = _ctx(), _ctx()
    dev = torch.device("cuda", 0)
    x = _audio(golden_dir, 900, 8)
    lanes = np.arange(1, 33, dtype=np.int32)
    d_pcm = torch.from_numpy(x).to(dev)
    d_pk = torch.zeros((900, 23), dtype=torch.uint8, device=dev)
    d_out = torch.zeros((900, 320), dtype=torch.int16, device=dev)
    before = ctx.export_streams([0, 1, 2])
    for spans, ln in [([(0, 0, 900), (0, 0, 10)], lanes), ([(0, 0, 900)], [0]), ([(0, 0, 900)], [5, 5]),
                      ([(0, 0, 900)], [MAX_STREAMS]), ([(MAX_STREAMS, 0, 900)], lanes)]:
        with pytest.raises(codec.LyraHipError):
            ctx.encode_spans_dev(spans, d_pcm, 184, d_pk, ln)
        with pytest.raises(codec.LyraHipError):
            ctx.decode_spans_dev(spans, d_pk, 184, d_out, ln)
    ctx.synchronize()
    assert np.array_equal(ctx.export_streams([0, 1, 2]), before) and not d_pk.any().item()
    ctx.encode_spans_dev([(0, 0, 900)], d_pcm, 184, d_pk, lanes)
    ctx.decode_spans_dev([(0, 0, 900)], d_pk, 184, d_out, lanes)
    ctx.synchronize()
    want_pk = _sequential(twin, {0: x}, 184, True)[0]
    want_pcm = _sequential(twin, {0: want_pk}, 184, False)[0]
    assert np.array_equal(d_pk.cpu().numpy(), want_pk) and np.array_equal(d_out.cpu().numpy(), want_pcm)
    _check_state("dev form", ctx, twin, [0], lanes)


def test_sample1_packets_equal_the_oracle(speech_sample1, oracle_default):
    """Against the CPU oracle directly: Stream.encode + rvq_encode + pack, and the decoded PCM of its packets."""
    from oracle import lyra_oracle
    hops = speech_sample1.size // 320
    x = np.ascontiguousarray(speech_sample1[:hops * 320]).reshape(hops, 320)
    ctx = _ctx()
    lanes = np.arange(1, 1 + 8, dtype=np.int32)
    pk = ctx.encode_spans([(0, 0, hops)], x, 184, lanes)
    s = lyra_oracle.Stream(oracle_default)
    feats = np.stack([s.encode(h) for h in x])
    want = oracle_default.pack(oracle_default.rvq_encode_batch(feats, 46), 46)
    assert np.array_equal(pk, want), np.flatnonzero((pk != want).any(axis=1))[:8]
    ref = lyra_oracle.run_batch(oracle_default, x[:, None, :], 46, do_decode=True)
    out = ctx.decode_spans([(0, 0, hops)], pk, 184, lanes)
    assert np.array_equal(out, ref["pcm"][:, 0]), np.flatnonzero((out != ref["pcm"][:, 0]).any(axis=1))[:8]


def test_file_functions_give_the_same_bytes(golden_dir, tmp_path):
    """EncodeFilesTimeParallel / DecodeFilesTimeParallel (file_demo --time-parallel) against EncodeFiles / DecodeFiles."""
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "file_demo")
    assert os.path.exists(demo), "lyra_amd/file_demo not built (__graft_entry__.build())"
    files = {"long": 1900 * 320 + 17, "short": 40 * 320, "tiny": 100, "mid": 611 * 320 + 319}
    wavs = []
    for k, (name, n) in enumerate(files.items()):
        pcm = _audio(golden_dir, n // 320 + 1, 40 + k).reshape(-1)[:n]
        with wave.open(str(tmp_path / f"{name}.wav"), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes(pcm.tobytes())
        wavs.append(str(tmp_path / f"{name}.wav"))
    outs = {}
    for flag in ((), ("--time-parallel=64",)):
        out_dir = tmp_path / ("tp" if flag else "seq")
        out_dir.mkdir()
        r = subprocess.run([demo, *flag, lyra_amd.default_model_dir(), "6000", str(out_dir)] + wavs,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (flag, r.returncode, r.stderr[-2000:])
        outs[bool(flag)] = out_dir
    for name, n in files.items():
        for suffix in (".lyra", "_decoded.wav"):
            a = (outs[False] / (name + suffix)).read_bytes()
            b = (outs[True] / (name + suffix)).read_bytes()
            assert a == b, (name, suffix, len(a), len(b))
        assert len((outs[True] / (name + ".lyra")).read_bytes()) == (n // 320) * 15
