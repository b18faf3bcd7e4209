"""Encoders of any rate, bitrate and DTX setting in one batch, the parts that need no GPU
(include/lyra_hip_encode_streams.h, lyra_amd/host/lyra_mixed_encoder.cc):
1. the header, the fourth ctypes table of lyra_amd/codec.py (_SIGNATURES_ENCODE_STREAMS) and the built library agree on the
   three symbols; a null context is refused; LyraHip has the three methods; the two new kernels are in the library's gfx950
   code object; the older headers and tables are what they were;
2. the host logic of MixedBatchLyraEncoder: tests/encode_streams/mixed_encoder_test.cc, a program of its own linked against a
   fake of the three calls (tests/encode_streams/fake_encode_streams_abi.cc) next to the unchanged fake of tests/host_stub,
   built with -fsanitize=address,undefined and run as a program."""
import os
import re
import subprocess

import pytest

from lyra_amd import codec

from abi_loading import _protos, load_library

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NEW = {"lyra_hip_encode_streams_dev": 11, "lyra_hip_encode_streams_begin": 7, "lyra_hip_encode_streams_end": 3}


@pytest.fixture(scope="module")
def lib():
    return load_library()


def test_header_fourth_table_and_library_agree_on_the_three_symbols(lib):
    protos = _protos("lyra_hip_encode_streams.h")
    assert set(protos) == set(NEW) == set(codec._SIGNATURES_ENCODE_STREAMS)
    for name, n_args in NEW.items():
        args = [a.strip() for a in protos[name].split(",")]
        assert len(args) == n_args, (name, args)
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name} is not exported by {codec.library_path()}"
        restype, argtypes = codec._SIGNATURES_ENCODE_STREAMS[name]
        assert restype is codec.C.c_int and fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert len(argtypes) == n_args, (name, argtypes)
        for a, t in zip(args, argtypes):   # pointers as void pointers, `long` as a long, everything else an int
            want = codec.C.c_void_p if "*" in a else codec.C.c_long if a.startswith("long ") else codec.C.c_int
            assert t is want, (name, a, t)


def test_a_null_context_is_refused_by_all_three(lib):
    for name in NEW:
        args = [None if t is codec.C.c_void_p else 0 for t in codec._SIGNATURES_ENCODE_STREAMS[name][1]]
        assert getattr(lib, name)(*args) < 0, name


def test_lyrahip_has_the_three_methods():
    for name in NEW:
        assert callable(getattr(codec.LyraHip, name[len("lyra_hip_"):], None)), name


def test_the_two_kernels_are_in_the_gfx950_code_object():
    """A kernel descriptor symbol (<mangled name>.kd) exists only in a device code object; the library bundles one target."""
    image = open(codec.library_path(), "rb").read()
    assert set(re.findall(rb"hip[v\d]*-amdgcn-amd-amdhsa--(gfx\w+)", image)) == {b"gfx950"}
    for kernel in (b"logmel_streams_kernel", b"resample_streams_kernel"):
        assert re.search(rb"_ZN4lyra\d+" + kernel + rb"\w*\.kd", image), kernel
    # (their siblings are still there)
    for kernel in (b"logmel_rates_kernel", b"resample_rates_kernel"):
        assert re.search(rb"_ZN4lyra\d+" + kernel + rb"\w*\.kd", image), kernel


def test_the_older_headers_and_tables_are_what_they_were():
    inc = os.path.join(ROOT, "include")
    for header in ("lyra_hip.h", "lyra_hip_spans_mixed.h", "lyra_hip_spans_rates.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, header)).read(), flags=re.S)
        assert "lyra_hip_encode_streams" not in text, header   # (lyra_hip.h points to the new header in a comment only)
    assert "lyra_hip_encode_streams.h" in open(os.path.join(inc, "lyra_hip.h")).read()
    assert "#include \"lyra_hip.h\"" in open(os.path.join(inc, "lyra_hip_encode_streams.h")).read()
    assert len(codec._SIGNATURES) == 88 and len(codec._SIGNATURES_SPANS_MIXED) == 5 and len(codec._SIGNATURES_SPANS_RATES) == 3
    others = set(codec._SIGNATURES) | set(codec._SIGNATURES_SPANS_MIXED) | set(codec._SIGNATURES_SPANS_RATES)
    assert not set(NEW) & others


def test_mixed_batch_encoder_host_logic_under_sanitizers(tmp_path):
    host = os.path.join(ROOT, "lyra_amd", "host")
    here = os.path.join(ROOT, "tests", "encode_streams")
    exe = str(tmp_path / "mixed_encoder_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + host, "-I" + os.path.join(host, "shims"), "-I" + ROOT,
                           "-I" + here, "-o", exe, os.path.join(here, "mixed_encoder_test.cc"),
                           os.path.join(here, "fake_encode_streams_abi.cc"), os.path.join(host, "lyra_mixed_encoder.cc"),
                           os.path.join(host, "lyra_batch_codec.cc"),
                           os.path.join(ROOT, "tests", "host_stub", "fake_lyra_hip_codec.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
