"""CPU-side checks of per-stream bitrates on the device path (lyra_hip_encode_mixed_dev, lyra_hip_decode_lossy_mixed_dev,
LYRA_HIP_STEP_MIXED_BITRATE): the library exports the calls, the Python mirror's lyra_hip_steps has the C layout, and the
invariant the mixed quantizer rests on -- the RVQ is greedy, so a frame quantised at n stages is the first n stages of the
same frame at 46 -- holds for the oracle on the golden vectors and on a few thousand more drawn the same way."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from abi_loading import load_library

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def lib():
    return load_library(raw=True)


def test_mixed_calls_are_exported(lib):
    for name in ("lyra_hip_encode_mixed_dev", "lyra_hip_encode_mixed_errors", "lyra_hip_decode_lossy_mixed_dev"):
        assert hasattr(lib, name), name


def test_steps_desc_matches_c_layout(tmp_path):
    """codec.StepsDesc against offsetof / sizeof of lyra_hip_steps, compiled from include/lyra_hip.h."""
    from lyra_amd import codec
    fields = [f[0] for f in codec.StepsDesc._fields_]
    src = tmp_path / "offsets.cc"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "lyra_hip.h"\nint main() {\n'
                   '  std::printf("sizeof %zu\\n", sizeof(lyra_hip_steps));\n' +
                   "".join(f'  std::printf("{f} %zu\\n", offsetof(lyra_hip_steps, {f}));\n' for f in fields) + "}\n")
    exe = tmp_path / "offsets"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got.pop("sizeof")) == ctypes.sizeof(codec.StepsDesc)
    for f in fields:
        assert int(got[f]) == getattr(codec.StepsDesc, f).offset, f
    assert fields[-2:] == ["d_bits_ring", "n_bits_ring"]
    assert codec.STEP_MIXED_BITRATE == 32 and codec.MAX_PACKET_BYTES == codec.packet_size(184) == 23


def _vectors(golden_dir):
    g = np.load(os.path.join(golden_dir, "rvq.npz"))
    rng = np.random.Generator(np.random.PCG64(0x6D6978))   # drawn like make_golden.py's `rnd`: on the encoder's grid + off it
    more = np.concatenate([(rng.integers(-128, 128, size=(2048, 64)) - 20) * np.float32(0.26349151134490967),
                           rng.normal(0, 3, size=(2048, 64))]).astype(np.float32)
    return np.concatenate([g["fixture"].reshape(1, 64), g["rnd"], more]).astype(np.float32)


def test_rvq_stage_prefix_invariant(oracle_exact, golden_dir):
    """rvq_encode_batch(feat, n) == the first n columns of rvq_encode_batch(feat, 46), -1 after them, for every n; the
    packed form agrees as a prefix at every even n (the oracle's pack writes num_stages // 2 bytes)."""
    o = oracle_exact
    feat = _vectors(golden_dir)
    full = o.rvq_encode_batch(feat, 46)
    assert (full >= 0).all() and (full < 16).all()
    packed46 = o.pack(full, 46)
    for n in range(1, 47):
        idx = o.rvq_encode_batch(feat, n)
        assert np.array_equal(idx[:, :n], full[:, :n]), n
        assert (idx[:, n:] == -1).all(), n
        if n % 2 == 0:
            assert np.array_equal(o.pack(idx, n), packed46[:, :n // 2]), n
