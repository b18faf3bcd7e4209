"""The conference bridge, the parts that need no GPU (include/lyra_hip_bridge.h):
1. the header, the ctypes table of lyra_amd/codec.py (_SIGNATURES_BRIDGE, with a loader of its own) and the built library agree
   on the symbols and argument counts; a null context is refused; LyraHip has the methods; bridge_mix_kernel is in the library's
   gfx950 code object; the older headers and tables are what they were;
2. the planner: tests/bridge/bridge_plan_test.cc, a program of its own over lyra_amd/csrc/bridge_plan.h built with
   -fsanitize=address,undefined and run as a program, against the numpy restatement of tests/bridge_models.py -- and the
   library's lyra_hip_bridge_plan against the same; and the staging layout of begin() / end():
   tests/bridge/bridge_staging_test.cc over lyra_amd/csrc/bridge_staging.h, built and run the same way;
3. the host logic of LyraConferenceBridge: tests/bridge/bridge_class_test.cc, linked against a fake of the new calls
   (tests/bridge/fake_bridge_abi.cc) next to the unchanged fake of tests/host_stub, built with the same flags and run as a
   program; the older classes' objects reference nothing of the new calls."""
import os
import re
import subprocess

import numpy as np
import pytest

from lyra_amd import codec

from abi_loading import _protos, load_library
from bridge_models import MAX_ROOM, np_bridge_plan

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HOST = os.path.join(ROOT, "lyra_amd", "host")
HERE = os.path.join(ROOT, "tests", "bridge")
NEW = {"lyra_hip_bridge_plan": 6, "lyra_hip_bridge_mix_dev": 10, "lyra_hip_bridge_tick_dev": 2, "lyra_hip_bridge_begin": 10,
       "lyra_hip_bridge_end": 5}
SAN = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")


@pytest.fixture(scope="module")
def lib():
    return load_library()


def test_header_table_and_library_agree_on_the_symbols(lib):
    protos = _protos("lyra_hip_bridge.h")
    assert set(protos) == set(NEW) and set(codec._SIGNATURES_BRIDGE) == set(NEW) | {"lyra_hip_bridge_errors"}
    for name, n_args in NEW.items():
        args = [a.strip() for a in protos[name].split(",")]
        assert len(args) == n_args, (name, args)
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name} is not exported by {codec.library_path()}"
        restype, argtypes = codec._SIGNATURES_BRIDGE[name]
        assert restype is codec.C.c_int and fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert len(argtypes) == n_args, (name, argtypes)
        for a, t in zip(args, argtypes):   # pointers as void pointers, `unsigned` as one, everything else an int
            want = codec.C.c_void_p if "*" in a else codec.C.c_uint if a.startswith("unsigned ") else codec.C.c_int
            assert t is want, (name, a, t)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lyra_hip_bridge.h")).read(), flags=re.S)
    assert re.search(r"\blong\s+lyra_hip_bridge_errors\s*\(\s*lyra_hip_ctx\s*\*\s*ctx\s*,\s*int\s+clear\s*\)\s*;", hdr)
    restype, argtypes = codec._SIGNATURES_BRIDGE["lyra_hip_bridge_errors"]
    assert restype is codec.C.c_long and list(argtypes) == [codec.C.c_void_p, codec.C.c_int]
    assert lib.lyra_hip_bridge_errors.restype is codec.C.c_long


def test_the_tick_struct_is_the_headers():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lyra_hip_bridge.h")).read(), flags=re.S)
    body = re.search(r"typedef struct lyra_hip_bridge_tick \{(.*?)\} lyra_hip_bridge_tick;", hdr, flags=re.S).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert [re.split(r"[\s*]+", f)[-1] for f in fields] == [n for n, _ in codec.BridgeTick._fields_]
    for f, (name, t) in zip(fields, codec.BridgeTick._fields_):
        want = codec.C.c_void_p if "*" in f else codec.C.c_uint if f.startswith("unsigned ") else codec.C.c_int
        assert t is want, (f, t)
    assert codec.BRIDGE_MAX_ROOM == MAX_ROOM == int(re.search(r"#define LYRA_HIP_BRIDGE_MAX_ROOM (\d+)", hdr).group(1))
    assert codec.BRIDGE_SKIP_COMFORT_NOISE == int(re.search(r"#define LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE (\d+)u", hdr).group(1))


def test_a_null_context_is_refused(lib):
    for name in set(NEW) - {"lyra_hip_bridge_plan"}:
        args = [None if t is codec.C.c_void_p else 0 for t in codec._SIGNATURES_BRIDGE[name][1]]
        assert getattr(lib, name)(*args) < 0, name
    assert lib.lyra_hip_bridge_errors(None, 0) < 0
    assert lib.lyra_hip_bridge_plan(None, 4, None, None, None, None) < 0      # (no context: null arrays are refused)


def test_lyrahip_has_the_methods():
    for name in ("bridge_mix_dev", "bridge_tick_dev", "bridge_begin", "bridge_end", "bridge_errors"):
        assert callable(getattr(codec.LyraHip, name, None)), name
    assert callable(codec.bridge_plan)


def test_the_kernel_is_in_the_gfx950_code_object():
    """A kernel descriptor symbol (<mangled name>.kd) exists only in a device code object; the library bundles one target."""
    image = open(codec.library_path(), "rb").read()
    assert set(re.findall(rb"hip[v\d]*-amdgcn-amd-amdhsa--(gfx\w+)", image)) == {b"gfx950"}
    for kernel in (b"bridge_mix_kernel", b"lossy_mix_kernel"):
        assert re.search(rb"_ZN4lyra\d+" + kernel + rb"E\w*\.kd", image), kernel


def test_the_older_headers_and_tables_are_what_they_were():
    inc = os.path.join(ROOT, "include")
    for header in sorted(os.listdir(inc)):
        if header == "lyra_hip_bridge.h":
            continue
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, header)).read(), flags=re.S)
        assert "lyra_hip_bridge" not in text, header   # (lyra_hip.h points to the new header in a comment only)
    assert "lyra_hip_bridge.h" in open(os.path.join(inc, "lyra_hip.h")).read()
    assert "#include \"lyra_hip.h\"" in open(os.path.join(inc, "lyra_hip_bridge.h")).read()
    tables = (codec._SIGNATURES, codec._SIGNATURES_SPANS_MIXED, codec._SIGNATURES_SPANS_RATES, codec._SIGNATURES_SPANS_PACKED,
              codec._SIGNATURES_ENCODE_STREAMS, codec._SIGNATURES_DECODE_STREAMS, codec._SIGNATURES_DECODE_SAMPLES_ANY,
              codec._SIGNATURES_DECODE_SAMPLES_STREAMS)
    assert [len(t) for t in tables[:2]] + [len(t) for t in tables[2:]] == [88, 5, 3, len(codec._SIGNATURES_SPANS_PACKED), 3, 3, 3, 3]
    assert not any(set(codec._SIGNATURES_BRIDGE) & set(t) for t in tables)


# ---- 2. the planner ---------------------------------------------------------------------------------------------------------

def _plan_cases():
    rng = np.random.default_rng(4)
    one_big = np.concatenate([np.full(MAX_ROOM, 5), [-1, 9, 9]])
    too_big = np.concatenate([[2], np.full(MAX_ROOM + 1, 5), [-3]])
    return {"random labels": rng.integers(-2, 9, 500), "one room": np.full(64, 3), "all negative": np.full(33, -1),
            "B = 1": np.array([0]), "B = 1, in no room": np.array([-7]),
            "non-contiguous labels": rng.choice([0, 7, 1000, 2 ** 31 - 1, 12], 200),
            "a room of 32767": rng.permutation(one_big), "a room of 32768": rng.permutation(too_big)}


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bridge_plan") / "bridge_plan_test")
    subprocess.check_call(SAN + ["-I" + os.path.join(ROOT, "lyra_amd", "csrc"), "-o", exe, os.path.join(HERE, "bridge_plan_test.cc")])
    return exe


@pytest.mark.parametrize("case", list(_plan_cases()))
def test_planner_program_under_sanitizers_equals_the_restatement(plan_exe, tmp_path, case, lib):
    rooms = np.asarray(_plan_cases()[case], np.int32)
    path = str(tmp_path / "rooms.bin")
    rooms.tofile(path)
    r = subprocess.run([plan_exe, path], capture_output=True, text=True, timeout=120, env=SAN_ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    want = np_bridge_plan(rooms)
    lines = r.stdout.split("\n")
    if want is None:
        assert case == "a room of 32768" and lines[0] == "-1"
        with pytest.raises(codec.LyraHipError):
            codec.bridge_plan(rooms)
        return
    assert case != "a room of 32768"
    order, start = want
    assert lines[0].split() == ["0", str(start.size - 1), str(order.size)] and lines[3] == "ok"
    assert np.array_equal(np.array(lines[1].split(), np.int64), order) and np.array_equal(np.array(lines[2].split(), np.int64), start)
    got = codec.bridge_plan(rooms)       # the library's function is the same header
    assert np.array_equal(got[0], order) and np.array_equal(got[1], start)
    # what the index promises: rooms in ascending label order, rows ascending inside a room, negative labels left out
    labels = [int(rooms[order[start[i]]]) for i in range(start.size - 1)]
    assert labels == sorted(set(int(v) for v in rooms if v >= 0))
    for i in range(start.size - 1):
        m = order[start[i]:start[i + 1]]
        assert (np.diff(m) > 0).all() and (rooms[m] == labels[i]).all()


def test_staging_layout_program_under_sanitizers(tmp_path):
    """tests/bridge/bridge_staging_test.cc over lyra_amd/csrc/bridge_staging.h: where the arrays of every kind of tick lie in
    the two staging slots of begin() / end() -- no overlap, the alignments, the bytes moved, the room in a slot."""
    exe = str(tmp_path / "bridge_staging_test")
    subprocess.check_call(SAN + ["-I" + os.path.join(ROOT, "lyra_amd", "csrc"), "-o", exe, os.path.join(HERE, "bridge_staging_test.cc")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=SAN_ENV)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


# ---- 3. the class -----------------------------------------------------------------------------------------------------------

def test_conference_bridge_host_logic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bridge_class_test")
    subprocess.check_call(SAN + ["-I" + HOST, "-I" + os.path.join(HOST, "shims"), "-I" + ROOT, "-I" + HERE, "-o", exe,
                                 os.path.join(HERE, "bridge_class_test.cc"), os.path.join(HERE, "fake_bridge_abi.cc"),
                                 os.path.join(HOST, "lyra_conference_bridge.cc"),
                                 os.path.join(ROOT, "tests", "host_stub", "fake_lyra_hip_codec.cc")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=SAN_ENV)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def _undefined(tmp_path, name):
    obj = str(tmp_path / (name + ".o"))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + HOST, "-I" + os.path.join(HOST, "shims"), "-I" + ROOT, "-c",
                           os.path.join(HOST, name), "-o", obj], timeout=600)
    return subprocess.check_output(["nm", "-C", "--undefined-only", obj], text=True)


def test_the_older_classes_do_not_reference_the_new_calls(tmp_path):
    for name in ("lyra_stream_state.cc", "lyra_batch_codec.cc", "lyra_device_decoder.cc", "lyra_device_decoder_any.cc",
                 "lyra_mixed_device_decoder.cc", "lyra_mixed_decoder.cc", "lyra_mixed_encoder.cc"):
        syms = _undefined(tmp_path, name)
        assert "lyra_hip_bridge" not in syms and "LyraConferenceBridge" not in syms, name
    syms = _undefined(tmp_path, "lyra_conference_bridge.cc")
    assert "lyra_hip_bridge_begin" in syms and "lyra_hip_bridge_end" in syms and "lyra_hip_reset_streams" in syms
    assert "decode_streams" not in syms and "encode_streams" not in syms   # (the class goes through the new calls only)
