"""CPU: what lyra_hip_encode_spans_dtx rests on (include/lyra_hip.h "Time-parallel spans", DTX).

1. The header, the ctypes prototypes of lyra_amd/codec.py and the built library agree on the four new symbols.
2. On the CPU model of LyraEncoder with DTX (oracle/lyra_codec_model.py): the estimator's decisions are the same whether or not
   the encoder runs, and an encoder fed ONLY the non-noise hops of the session, restarted W non-noise hops early, gives the
   sequential packets from the W-th of them on -- the compacted list of non-noise hops is a stream of its own.
"""
import os
import re

import numpy as np
import pytest

from lyra_amd import codec

from abi_loading import load_library

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = {"lyra_hip_encode_spans_dtx_dev": 11, "lyra_hip_encode_spans_dtx": 10, "lyra_hip_noise_spans_dev": 6,
       "lyra_hip_noise_spans": 6}
N_HOPS, BITS = 150, 64


@pytest.fixture(scope="module")
def lib():
    return load_library()


def test_header_ctypes_and_library_agree_on_the_new_symbols(lib):
    hdr = open(os.path.join(ROOT, "include", "lyra_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(lyra_hip_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)}
    for name, n_args in NEW.items():
        assert name in protos, f"{name} is not declared in include/lyra_hip.h"
        args = [a.strip() for a in protos[name].split(",")]
        assert len(args) == n_args, (name, args)
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name} is not exported by {codec.library_path()}"
        assert fn.argtypes is not None and len(fn.argtypes) == n_args, (name, fn.argtypes)
        for a, t in zip(args, fn.argtypes):   # pointers as void pointers, everything else an int
            assert ("*" in a) == (t is codec.C.c_void_p), (name, a, t)
    # a null context is refused, not dereferenced
    assert lib.lyra_hip_encode_spans_dtx_dev(None, None, 0, None, 0, None, 16000, None, 64, None, None) < 0
    assert lib.lyra_hip_noise_spans(None, 0, None, 0, None, None) < 0


def _session():
    """150 hops at 16 kHz: speech, digital silence and +-12 noise in turns"""
    rng = np.random.default_rng(3)
    w = np.load(os.path.join(GOLDEN, "sample_wavs.npz"))
    src = np.concatenate([w["sample1_16kHz"], w["sample2_16kHz"]]).astype(np.int32)
    x = (src[(20000 + np.arange(N_HOPS * 320)) % src.size] * 3).reshape(N_HOPS, 320)
    at = k = 0
    while at < N_HOPS:
        kind = "SZNZ"[k % 4]
        n = int(rng.integers(8, 15) if kind == "S" else rng.integers(4, 9))
        if kind == "Z":
            x[at:at + n] = 0
        elif kind == "N":
            x[at:at + n] = rng.integers(-12, 13, x[at:at + n].shape)
        at += n; k += 1
    return np.clip(x, -32768, 32767).astype(np.int16)


def test_compacted_non_noise_hops_are_a_stream_of_their_own(lib):
    from oracle import lyra_oracle
    from oracle.lyra_codec_model import RefLyraEncoder
    lyra_oracle.build()
    O = lyra_oracle.Oracle(mode="xnnpack")
    W = codec.span_warmup_frames("encoder", lib)
    hops = _session()
    enc = RefLyraEncoder(O, 16000, BITS, enable_dtx=True)
    packets = [enc.Encode(h) for h in hops]
    active = np.array([p.size > 0 for p in packets])
    assert active.sum() >= 2 * W + 20 and (~active).sum() >= 20 and np.count_nonzero(active[1:] != active[:-1]) >= 8
    # the decisions do not need the encoder
    est = lyra_oracle.NoiseEstimator(O, sample_rate_hz=16000)
    alone = np.array([not est.ReceiveSamples(h)[0] for h in hops])
    assert np.array_equal(alone, active)
    # ... and the encoder does not need the noise hops: restarted W non-noise hops early it is the sequential one
    at = np.flatnonzero(active)
    for r in (W, W + 7, int(active.sum()) - 12):
        s = lyra_oracle.Stream(O)
        for c in range(r - W, at.size):
            feat = s.encode(hops[at[c]])
            if c < r:
                continue
            got = O.pack(O.rvq_encode(feat, BITS // 4), BITS // 4)[0]
            assert np.array_equal(got, packets[at[c]]), (r, c, int(at[c]))
