"""CPU-side checks of per-stream sample rates on the device path (lyra_hip_encode_rates_dev,
lyra_hip_decode_lossy_rates_dev, LYRA_HIP_STEP_MIXED_RATE): the library exports the calls, the Python mirror's
lyra_hip_steps has the C layout, and what rows of a fixed stride rest on -- hop by hop the codec's resamplers turn one hop
into exactly one hop, nothing carries over -- holds for the oracle."""
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


def test_rates_calls_are_exported(lib):
    for name in ("lyra_hip_encode_rates_dev", "lyra_hip_decode_lossy_rates_dev", "lyra_hip_rates_errors"):
        assert hasattr(lib, name), name


def test_steps_desc_matches_c_layout(tmp_path):
    """codec.StepsDescRates against offsetof / sizeof of lyra_hip_steps_rates, compiled from include/lyra_hip.h: the first
    member is lyra_hip_steps, unchanged, and d_rates -- the last field -- lies where a field appended to it would."""
    import lyra_amd
    from lyra_amd import codec
    fields = ["steps." + f[0] for f in codec.StepsDesc._fields_] + ["d_rates"]
    src = tmp_path / "offsets.cc"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "lyra_hip.h"\nint main() {\n'
                   '  std::printf("sizeof %zu\\n", sizeof(lyra_hip_steps_rates));\n'
                   '  std::printf("inner %zu\\n", sizeof(lyra_hip_steps));\n'
                   '  std::printf("flag %u\\n", LYRA_HIP_STEP_MIXED_RATE);\n'
                   '  std::printf("hop %d\\n", LYRA_HIP_MAX_EXT_HOP);\n' +
                   "".join(f'  std::printf("{f} %zu\\n", offsetof(lyra_hip_steps_rates, {f}));\n' for f in fields) + "}\n")
    exe = tmp_path / "offsets"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got.pop("sizeof")) == ctypes.sizeof(codec.StepsDescRates)
    inner = int(got.pop("inner"))
    assert inner == ctypes.sizeof(codec.StepsDesc) == int(got["d_rates"]) == codec.StepsDescRates.d_rates.offset
    assert int(got.pop("flag")) == codec.STEP_MIXED_RATE == lyra_amd.STEP_MIXED_RATE == 64
    assert int(got.pop("hop")) == codec.MAX_EXT_HOP == lyra_amd.MAX_EXT_HOP == 960
    for f in fields[:-1]:
        assert int(got[f]) == getattr(codec.StepsDesc, f.split(".")[1]).offset, f
    assert [f[0] for f in codec.StepsDescRates._fields_] == ["steps", "d_rates"]


@pytest.mark.parametrize("rate", [8000, 32000, 48000])
def test_oracle_resampler_turns_one_hop_into_one_hop(oracle_exact, rate):
    """200 hops of random int16 audio, fed one hop after another: rate -> 16 kHz gives exactly 320 samples for rate / 50,
    16 kHz -> rate exactly rate / 50 for 320, on every hop."""
    from oracle import lyra_oracle
    rng = np.random.default_rng(rate)
    down, up = lyra_oracle.Resampler(rate, 16000), lyra_oracle.Resampler(16000, rate)
    for _ in range(200):
        assert down.Resample(rng.integers(-32768, 32768, size=rate // 50).astype(np.int16)).size == 320
        assert up.Resample(rng.integers(-32768, 32768, size=320).astype(np.int16)).size == rate // 50


def test_reference_model_at_16k_holds_no_resampler(oracle_exact):
    from oracle import lyra_codec_model as M
    enc = M.RefLyraEncoder(oracle_exact, 16000, 184, False)
    dec = M.RefLyraDecoder(oracle_exact, 16000, 1)
    assert enc.resampler is None and dec.resampler is None
