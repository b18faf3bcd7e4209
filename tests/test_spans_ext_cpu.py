"""CPU: the span calls and the whole-file functions at 8, 32 and 48 kHz (include/lyra_hip.h "Time-parallel spans", the `_ext`
forms; lyra_amd/host/lyra_file_codec.h).

1. EncodeFiles / DecodeFiles over the fake C ABI at 48 and 8 kHz: WAVs of unequal lengths, one shorter than a hop, a decode
   rate that differs from the encode rate; every .lyra and every decoded WAV is what the reference model with the same fake
   components gives for that file alone.
2. The property the one-pass span resampler rests on, held on the CPU oracle: the resampler fed a whole signal in one call
   equals the same signal fed in 20 ms hops, for all six rate pairs -- its state is the input's recent past, nothing else.
3. The four new symbols are exported by the library and declared in the header.
"""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from lyra_amd import codec

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW_SYMBOLS = ("lyra_hip_encode_spans_ext_dev", "lyra_hip_decode_spans_ext_dev", "lyra_hip_encode_spans_ext",
               "lyra_hip_decode_spans_ext")


@pytest.fixture(scope="module")
def fake_file_demo(tmp_path_factory):
    """file_demo + the file and batch codecs against tests/host_stub/fake_lyra_hip_codec.cc (no GPU, no product library)"""
    host = os.path.join(ROOT, "lyra_amd", "host")
    exe = str(tmp_path_factory.mktemp("fake_demo") / "file_demo_fake")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + host, "-I" + os.path.join(host, "shims"), "-I" + ROOT, "-o", exe,
                           os.path.join(host, "file_demo.cc"), os.path.join(host, "lyra_file_codec.cc"),
                           os.path.join(host, "lyra_batch_codec.cc"),
                           os.path.join(ROOT, "tests", "host_stub", "fake_lyra_hip_codec.cc")])
    return exe


@pytest.mark.parametrize("rate,decode_rate,bitrate", [(48000, 48000, 9200), (8000, 32000, 6000), (48000, 16000, 3200)])
def test_file_functions_at_other_rates_against_fake_abi(fake_file_demo, tmp_path, rate, decode_rate, bitrate):
    sys.path.insert(0, os.path.join(ROOT, "tests", "host_stub"))
    from fake_kit import FakeKit
    from oracle import lyra_codec_model as M
    hop, out_hop = rate // 50, decode_rate // 50
    bits, nbytes = {3200: (64, 8), 6000: (120, 15), 9200: (184, 23)}[bitrate]
    rng = np.random.default_rng(rate + bitrate)
    lengths = {"a": hop * 17 + hop // 3, "b": hop * 5, "c": hop * 6, "d": hop * 11 - 7, "tiny": hop - 1, "e": hop * 17}
    files = {k: rng.integers(-9000, 9000, n).astype(np.int16) for k, n in lengths.items()}
    wavs = []
    for name, pcm in files.items():
        with wave.open(str(tmp_path / f"{name}.wav"), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
            w.writeframes(pcm.tobytes())
        wavs.append(str(tmp_path / f"{name}.wav"))
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    r = subprocess.run([fake_file_demo, f"--decode-rate={decode_rate}", "unused_model_dir", str(bitrate), str(out_dir)] + wavs,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    for name, pcm in files.items():
        hops = len(pcm) // hop
        enc = np.fromfile(out_dir / f"{name}.lyra", np.uint8)
        with wave.open(str(out_dir / f"{name}_decoded.wav"), "rb") as w:
            assert w.getnchannels() == 1 and w.getframerate() == decode_rate, name
            dec = np.frombuffer(w.readframes(w.getnframes()), np.int16)
        assert enc.size == hops * nbytes and dec.size == hops * out_hop, name
        e = M.RefLyraEncoder(None, rate, bits, False, kit=FakeKit())
        d = M.RefLyraDecoder(None, decode_rate, cng_seed=0, kit=FakeKit())
        for h in range(hops):
            p = e.Encode(pcm[h * hop:(h + 1) * hop])
            assert np.array_equal(enc[h * nbytes:(h + 1) * nbytes], p), (name, h)
            d.SetEncodedPacket(p)
            assert np.array_equal(dec[h * out_hop:(h + 1) * out_hop], d.DecodeSamples(out_hop)), (name, h)


def test_file_demo_refuses_unknown_rates(fake_file_demo, tmp_path):
    """44.1 kHz is no codec rate (exit 4: the encode is refused), and a bad --decode-rate fails the decode (exit 5)."""
    pcm = np.arange(3000, dtype=np.int16)
    for name, rate in (("cd", 44100), ("ok", 16000)):
        with wave.open(str(tmp_path / f"{name}.wav"), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
            w.writeframes(pcm.tobytes())
    r = subprocess.run([fake_file_demo, "m", "6000", str(tmp_path), str(tmp_path / "cd.wav")], capture_output=True, timeout=60)
    assert r.returncode == 4
    r = subprocess.run([fake_file_demo, "--decode-rate=44100", "m", "6000", str(tmp_path), str(tmp_path / "ok.wav")],
                       capture_output=True, timeout=60)
    assert r.returncode == 5


@pytest.mark.parametrize("in_rate,out_rate", [(8000, 16000), (32000, 16000), (48000, 16000),
                                              (16000, 8000), (16000, 32000), (16000, 48000)])
def test_oracle_resampler_whole_signal_equals_hops(in_rate, out_rate):
    from oracle import lyra_oracle
    lyra_oracle.build()
    hop = in_rate // 50
    n_hops = min(23, 8192 // hop)   # (the oracle takes at most 8192 input samples per call)
    rng = np.random.default_rng(in_rate + out_rate)
    x = rng.integers(-32768, 32768, hop * n_hops).astype(np.int16)   # full scale: the clip is part of the property
    whole = lyra_oracle.Resampler(in_rate, out_rate).Resample(x)
    by_hop = lyra_oracle.Resampler(in_rate, out_rate)
    parts = np.concatenate([by_hop.Resample(x[h * hop:(h + 1) * hop]) for h in range(n_hops)])
    assert whole.size == n_hops * (out_rate // 50)
    assert np.array_equal(whole, parts)


def test_new_symbols_exported_and_declared():
    if not os.path.isfile(codec.library_path()):
        codec.build_library()
    lib = codec._load()
    header = open(os.path.join(ROOT, "include", "lyra_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by {codec.library_path()}"
        assert f"int {name}(lyra_hip_ctx* ctx," in header, f"{name} is not declared in include/lyra_hip.h"
