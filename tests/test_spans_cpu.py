"""CPU: the two foundations of the time-parallel span calls (include/lyra_hip.h "Time-parallel spans").

1. The warm-up bound.  lyra_hip_span_warmup_frames is derived from the graphs' kernel sizes, strides and dilations
   (lyra_amd/csrc/spans_plan.h); here the CPU oracle is held to it: a fresh stream restarted W hops in front of
   hop r equals the stream that ran from hop 0, bit for bit, on every hop from r on -- features, and float PCM from lossy
   features -- in all four arithmetic modes, on noise and on the two recordings of tests/golden/sample_wavs.npz.
2. The planner (lyra_hip_spans_plan, a pure function): over random span and lane sets every frame is produced exactly once,
   every lane chunk warms up on frames of its own span, the running lanes of every step are a prefix of the lane rows, the
   last chunk's ring phase is the sequential stream's, and bad id sets are refused.
"""
import os

import numpy as np
import pytest

from lyra_amd import codec

from abi_loading import load_library

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MEASURED = {"encoder": 23, "decoder": 25}   # last differing hop after a restart, CPU oracle, 140 hops of noise (the issue)
N_HOPS = 84
RESTARTS = (26, 33, 41, 52)                 # >= W: the restarted stream begins at hop r - W


@pytest.fixture(scope="module")
def lib():
    return load_library()


def test_warmup_frames_cover_the_measured_restarts(lib):
    for side, measured in MEASURED.items():
        assert codec.span_warmup_frames(side, lib) >= measured, side
    assert lib.lyra_hip_span_warmup_frames(2) < 0


def _signals():
    rng = np.random.default_rng(11)
    wavs = np.load(os.path.join(GOLDEN, "sample_wavs.npz"))
    out = {"noise": rng.integers(-32768, 32768, N_HOPS * 320).astype(np.int16)}
    for name in wavs.files[:2]:
        w = wavs[name]
        start = min(16000, max(0, w.size - N_HOPS * 320))   # past the leading silence where the file allows
        out[name] = np.ascontiguousarray(w[start:start + N_HOPS * 320])
    assert len(out) == 3 and all(v.size == N_HOPS * 320 for v in out.values())
    return out


@pytest.mark.parametrize("mode", ["exact", "gemmlowp_double", "xnnpack", "builtin_mixed"])
def test_oracle_stream_restarted_w_hops_early_is_bit_identical(lib, mode):
    from oracle import lyra_oracle
    lyra_oracle.build()
    O = lyra_oracle.Oracle(mode=mode)
    w_enc, w_dec = codec.span_warmup_frames("encoder", lib), codec.span_warmup_frames("decoder", lib)
    for name, pcm in _signals().items():
        hops = pcm.reshape(N_HOPS, 320)
        s = lyra_oracle.Stream(O)
        feats = np.stack([s.encode(h) for h in hops])
        lossy = O.rvq_decode(O.rvq_encode_batch(feats, 46))
        d = lyra_oracle.Stream(O)
        pf = np.stack([d.decode(f, want_float=True)[1] for f in lossy])
        for r in RESTARTS:
            e2 = lyra_oracle.Stream(O)
            got = np.stack([e2.encode(h) for h in hops[r - w_enc:]])[w_enc:]
            assert np.array_equal(got.view(np.uint32), feats[r:].view(np.uint32)), (mode, name, r, "features")
            d2 = lyra_oracle.Stream(O)
            got = np.stack([d2.decode(f, want_float=True)[1] for f in lossy[r - w_dec:]])[w_dec:]
            assert np.array_equal(got.view(np.uint32), pf[r:].view(np.uint32)), (mode, name, r, "float pcm")


def _random_case(rng):
    max_streams = int(rng.integers(2, 200))
    n_spans = int(rng.integers(1, min(6, max_streams) + 1))
    n_lanes = int(rng.integers(0, max_streams - n_spans + 1))
    ids = rng.permutation(max_streams)[:n_spans + n_lanes].astype(np.int32)
    spans, at = [], int(rng.integers(0, 50))
    for s in range(n_spans):
        n = int(rng.choice([0, 1, 25, 26, 43, int(rng.integers(0, 400)), int(rng.integers(0, 20000))]))
        spans.append((int(ids[s]), at, n))
        at += n + int(rng.integers(0, 40))
    order = rng.permutation(n_spans)   # spans need not be listed in buffer order
    return max_streams, [spans[i] for i in order], ids[n_spans:]


@pytest.mark.parametrize("side", ["encoder", "decoder"])
def test_planner_properties_over_random_span_and_lane_sets(lib, side):
    rng = np.random.default_rng(2024)
    W = codec.span_warmup_frames(side, lib)
    cut = 0
    for _ in range(300):
        max_streams, spans, lanes = _random_case(rng)
        chunks, steps = codec.spans_plan(side, spans, lanes, max_streams, lib)
        total = sum(s[2] for s in spans)
        # every frame of every span is produced exactly once, nothing else is
        produced = {}
        for c in chunks:
            for f in range(int(c["first_frame"]), int(c["first_frame"]) + int(c["n_frames"])):
                assert f not in produced, (spans, c)
                produced[f] = int(c["span"])
        assert len(produced) == total
        for i, (sid, first, n) in enumerate(spans):
            assert all(produced[f] == i for f in range(first, first + n))
        # rows: a span's first chunk on its own id without warm-up, the others on distinct lanes behind W hops of the SAME span
        own = [c for c in chunks if c["n_warmup"] == 0]
        lane_rows = [c for c in chunks if c["n_warmup"] != 0]
        assert list(chunks[:len(own)]) == own, "own rows first"
        assert sorted(int(c["span"]) for c in own) == [i for i, s in enumerate(spans) if s[2] > 0]
        used = [int(c["stream_id"]) for c in lane_rows]
        assert len(set(used)) == len(used) and set(used) <= set(int(v) for v in lanes)
        for c in own:
            sid, first, n = spans[int(c["span"])]
            assert int(c["stream_id"]) == sid and int(c["first_frame"]) == first and c["n_frames"] >= 1
        for c in lane_rows:
            sid, first, n = spans[int(c["span"])]
            assert c["n_warmup"] >= W and c["n_frames"] >= 1
            assert int(c["first_frame"]) - int(c["n_warmup"]) >= first, "warm-up frames inside its own span"
            assert int(c["phase_offset"]) == (int(c["first_frame"]) - int(c["n_warmup"]) - first) % 18
        # the running lanes of every step are a prefix of the lane rows (and so are the running own rows)
        for rows in (own, lane_rows):
            n_steps = [int(c["n_warmup"]) + int(c["n_frames"]) for c in rows]
            assert n_steps == sorted(n_steps, reverse=True)
        assert steps == max([int(c["n_warmup"]) + int(c["n_frames"]) for c in chunks], default=0)
        # phase congruence: the last chunk ends with the ring phase of the stream that ran the whole span
        for i, (sid, first, n) in enumerate(spans):
            mine = [c for c in lane_rows if int(c["span"]) == i]
            assert sum(int(c["last"]) for c in mine) == (1 if mine else 0)
            for c in mine:
                if c["last"]:
                    assert int(c["first_frame"]) + int(c["n_frames"]) == first + n
                    assert (int(c["phase_offset"]) + int(c["n_warmup"]) + int(c["n_frames"])) % 18 == n % 18
        # the step count is what the lanes allow: no lanes -> the longest span; never worse than that
        longest = max(s[2] for s in spans)
        assert steps <= longest
        if len(lanes) == 0:
            assert steps == longest and not lane_rows
        cut += bool(lane_rows)
    assert cut > 100, "the random cases must exercise cutting"


def test_planner_cuts_the_one_hour_recording(lib):
    """180,000 hops on 4096 lanes: every lane is worth its warm-up, the call is under a hundred steps."""
    W = codec.span_warmup_frames("encoder", lib)
    chunks, steps = codec.spans_plan("encoder", [(0, 0, 180000)], np.arange(1, 4097), 4097, lib)
    assert len(chunks) > 4000 and steps < 100
    L = steps - W
    assert int(chunks["n_frames"].sum()) == 180000 and (L + W) / L < 1.7


def test_planner_refuses_bad_id_sets(lib):
    ok = [(0, 0, 100), (1, 100, 100)]
    codec.spans_plan("encoder", ok, [2, 3], 8, lib)
    for spans, lanes, max_streams in [
            ([(0, 0, 100), (0, 100, 100)], [2], 8),       # a span id twice
            (ok, [2, 2], 8),                              # a lane twice
            (ok, [1], 8),                                 # a lane that is a span's stream
            (ok, [8], 8), (ok, [-1], 8),                  # ids outside the context
            ([(9, 0, 10)], [], 8),
            ([(0, 0, 100), (1, 50, 100)], [2], 8),        # overlapping frame ranges
            ([(0, -1, 10)], [], 8), ([(0, 0, -1)], [], 8)]:
        with pytest.raises(codec.LyraHipError):
            codec.spans_plan("encoder", spans, lanes, max_streams, lib)
