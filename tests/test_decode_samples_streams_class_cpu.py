"""MixedAnySizeDeviceLyraDecoder (lyra_amd/host/lyra_mixed_device_decoder.cc) without a GPU:
tests/decode_samples_streams/mixed_any_decoder_test.cc, a program of its own linked against a fake of the three calls of
include/lyra_hip_decode_samples_streams.h (tests/decode_samples_streams/fake_decode_samples_streams_abi.cc) next to the unchanged
fakes of tests/decode_samples_any and tests/host_stub, built with -fsanitize=address,undefined and run as a program: the mirror's
leftover count and DsState per stream against the integers the fake device keeps over a script with four rates and changing
sizes, the refusals, the class blob round trip to and from AnySizeDeviceLyraDecoder.  And: the older classes' objects reference
nothing of the new call."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HOST = os.path.join(ROOT, "lyra_amd", "host")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")


def test_mixed_any_size_decoder_host_logic_under_sanitizers(tmp_path):
    here = os.path.join(ROOT, "tests", "decode_samples_streams")
    exe = str(tmp_path / "mixed_any_decoder_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + HOST, "-I" + os.path.join(HOST, "shims"), "-I" + ROOT,
                           "-o", exe, os.path.join(here, "mixed_any_decoder_test.cc"),
                           os.path.join(here, "fake_decode_samples_streams_abi.cc"),
                           os.path.join(ROOT, "tests", "decode_samples_any", "fake_decode_samples_any_abi.cc"),
                           os.path.join(HOST, "lyra_mixed_device_decoder.cc"), os.path.join(HOST, "lyra_device_decoder_any.cc"),
                           os.path.join(ROOT, "tests", "host_stub", "fake_lyra_hip_codec.cc")], timeout=600)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("mixed any decoder ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_the_older_classes_do_not_reference_the_new_call(tmp_path):
    for name in ("lyra_stream_state.cc", "lyra_batch_codec.cc", "lyra_device_decoder.cc", "lyra_device_decoder_any.cc",
                 "lyra_mixed_decoder.cc", "lyra_mixed_encoder.cc"):
        obj = str(tmp_path / (name + ".o"))
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + HOST, "-I" + os.path.join(HOST, "shims"), "-I" + ROOT, "-c",
                               os.path.join(HOST, name), "-o", obj], timeout=600)
        syms = subprocess.check_output(["nm", "-C", "--undefined-only", obj], text=True)
        assert "decode_samples_streams" not in syms and "MixedAnySizeDeviceLyraDecoder" not in syms, name
    obj = str(tmp_path / "new.o")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + HOST, "-I" + os.path.join(HOST, "shims"), "-I" + ROOT, "-c",
                           os.path.join(HOST, "lyra_mixed_device_decoder.cc"), "-o", obj], timeout=600)
    syms = subprocess.check_output(["nm", "-C", "--undefined-only", obj], text=True)
    assert "lyra_hip_decode_samples_streams_begin" in syms and "lyra_hip_decode_samples_streams_end" in syms
    assert "decode_samples_any" not in syms     # (and the new class goes through the new calls only)
