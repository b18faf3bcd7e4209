"""The conference bridge with loudest-N selection, the parts that need no GPU (include/lyra_hip_speakers.h):
1. the header, the ctypes table of lyra_amd/codec.py (_SIGNATURES_SPEAKERS, with a loader of its own) and the built library agree
   on the symbols, argument counts and types; the tick struct is SpeakersTick; a null context is refused; LyraHip has the
   methods; the three kernels are in the library's gfx950 code object; the header does not name the full-mix bridge's symbols;
2. the numpy restatement of tests/speaker_models.py holds its own properties: nobody left out = the full mix, the tie rule, and
   the kernel case's own assertions;
3. the host logic of LyraSpeakerBridge: tests/speakers/speaker_class_test.cc, linked against a fake of the new calls
   (tests/speakers/fake_speakers_abi.cc) next to the unchanged fakes, built with -fsanitize=address,undefined and run as a
   program; lyra_conference_bridge.cc references nothing of the new calls."""
import os
import re
import subprocess

import numpy as np
import pytest

from lyra_amd import codec

from abi_loading import _protos, load_library
from bridge_models import bridge_kernel_case, np_bridge_mix, np_bridge_plan
from speaker_models import SPEAKERS_MAX, np_levels, np_select, np_speakers_mix, speakers_kernel_case, threshold_case

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HOST = os.path.join(ROOT, "lyra_amd", "host")
HERE = os.path.join(ROOT, "tests", "speakers")
NEW = {"lyra_hip_speakers_mix_dev": 13, "lyra_hip_speakers_tick_dev": 2, "lyra_hip_speakers_begin": 11, "lyra_hip_speakers_end": 7}
SAN = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")


@pytest.fixture(scope="module")
def lib():
    return load_library()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lyra_hip_speakers.h")).read(), flags=re.S)


def _ctype(decl):
    """pointers as void pointers, `unsigned` as one, everything else an int"""
    return codec.C.c_void_p if "*" in decl else codec.C.c_uint if decl.startswith("unsigned ") else codec.C.c_int


# ---- 1. the ABI -------------------------------------------------------------------------------------------------------------

def test_header_table_and_library_agree_on_the_symbols(lib):
    protos = _protos("lyra_hip_speakers.h")
    assert set(protos) == set(NEW) == set(codec._SIGNATURES_SPEAKERS)
    for name, n_args in NEW.items():
        args = [a.strip() for a in protos[name].split(",")]
        assert len(args) == n_args, (name, args)
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name} is not exported by {codec.library_path()}"
        restype, argtypes = codec._SIGNATURES_SPEAKERS[name]
        assert restype is codec.C.c_int and fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert [_ctype(a) for a in args] == list(argtypes), (name, args)
    # the arguments of the stateless helper and of begin() are the full-mix bridge's with the selection's added
    bridge = _protos("lyra_hip_bridge.h")
    names = lambda text: [re.split(r"[\s*]+", a.strip())[-1] for a in text.split(",")]   # noqa: E731
    assert names(protos["lyra_hip_speakers_begin"]) == names(bridge["lyra_hip_bridge_begin"]) + ["max_speakers"]
    assert names(protos["lyra_hip_speakers_end"]) == names(bridge["lyra_hip_bridge_end"]) + ["levels", "is_speaker"]
    mix = names(bridge["lyra_hip_bridge_mix_dev"])
    assert names(protos["lyra_hip_speakers_mix_dev"]) == mix[:-1] + ["max_speakers", "d_mix", "d_levels", "d_is_speaker"]


def test_the_tick_struct_is_the_headers_and_extends_the_bridges():
    hdr = _header()
    body = re.search(r"typedef struct lyra_hip_speakers_tick \{(.*?)\} lyra_hip_speakers_tick;", hdr, flags=re.S).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert [re.split(r"[\s*]+", f)[-1] for f in fields] == [n for n, _ in codec.SpeakersTick._fields_]
    for f, (name, t) in zip(fields, codec.SpeakersTick._fields_):
        assert t is _ctype(f), (f, t)
    # the fields of lyra_hip_bridge_tick in the same order, with the same declarations, then the three new ones
    old = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lyra_hip_bridge.h")).read(), flags=re.S)
    old_body = re.search(r"typedef struct lyra_hip_bridge_tick \{(.*?)\} lyra_hip_bridge_tick;", old, flags=re.S).group(1)
    old_fields = [" ".join(f.split()) for f in old_body.split(";") if f.strip()]
    assert [" ".join(f.split()) for f in fields] == old_fields + ["int max_speakers", "int64_t* d_levels", "int32_t* d_is_speaker"]
    assert codec.SpeakersTick._fields_[:len(old_fields)] == codec.BridgeTick._fields_
    assert codec.SPEAKERS_MAX == SPEAKERS_MAX == int(re.search(r"#define LYRA_HIP_SPEAKERS_MAX (\d+)", hdr).group(1)) == 8
    assert codec.SPEAKERS_SKIP_COMFORT_NOISE == int(re.search(r"#define LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE (\d+)u", hdr).group(1))
    assert codec.SPEAKERS_SKIP_COMFORT_NOISE == codec.BRIDGE_SKIP_COMFORT_NOISE


def test_a_null_context_is_refused(lib):
    for name in NEW:
        args = [None if t is codec.C.c_void_p else 0 for t in codec._SIGNATURES_SPEAKERS[name][1]]
        assert getattr(lib, name)(*args) < 0, name


def test_lyrahip_has_the_methods():
    for name in ("speakers_mix_dev", "speakers_tick_dev", "speakers_begin", "speakers_end"):
        assert callable(getattr(codec.LyraHip, name, None)), name


def test_the_kernels_are_in_the_gfx950_code_object():
    """A kernel descriptor symbol (<mangled name>.kd) exists only in a device code object; the library bundles one target."""
    image = open(codec.library_path(), "rb").read()
    assert set(re.findall(rb"hip[v\d]*-amdgcn-amd-amdhsa--(gfx\w+)", image)) == {b"gfx950"}
    for kernel in (b"speakers_level_kernel", b"speakers_select_kernel", b"speakers_mix_kernel"):
        assert re.search(rb"_ZN4lyra\d+" + kernel + rb"E\w*\.kd", image), kernel


def test_the_header_stands_beside_the_bridges_and_the_tables_do_not_overlap():
    hdr = _header()
    assert "lyra_hip_bridge" not in hdr                  # (comments may point to it; the declarations are self-contained)
    assert re.findall(r"#include\s+\"([^\"]+)\"", hdr) == ["lyra_hip.h"]
    assert "lyra_hip_speakers.h" in open(os.path.join(ROOT, "include", "lyra_hip.h")).read()
    assert "lyra_hip_speakers" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lyra_hip.h")).read(), flags=re.S)
    tables = (codec._SIGNATURES, codec._SIGNATURES_SPANS_MIXED, codec._SIGNATURES_SPANS_RATES, codec._SIGNATURES_SPANS_PACKED,
              codec._SIGNATURES_ENCODE_STREAMS, codec._SIGNATURES_DECODE_STREAMS, codec._SIGNATURES_DECODE_SAMPLES_ANY,
              codec._SIGNATURES_DECODE_SAMPLES_STREAMS, codec._SIGNATURES_BRIDGE)
    assert not any(set(codec._SIGNATURES_SPEAKERS) & set(t) for t in tables)


# ---- 2. the model's own properties ------------------------------------------------------------------------------------------

def test_model_with_nobody_left_out_is_the_full_mix():
    x, rooms, muted, is_cn = bridge_kernel_case()
    small = np.where(np.isin(rooms, (0, 1, 2, 3)), rooms, -1).astype(np.int32)
    rest = np.flatnonzero(small < 0)
    small[rest] = 10 + np.arange(rest.size) // 8          # every room has at most 8 members
    order, start = np_bridge_plan(small)
    mix, levels, spk = np_speakers_mix(x, order, start, 8, muted, is_cn)
    assert np.array_equal(mix, np_bridge_mix(x, order, start, muted, is_cn))
    assert np.array_equal(levels, np_levels(x)) and levels.dtype == np.int64 and levels.max() == 320 * 2 ** 30
    source = (muted == 0) & (is_cn == 0)
    assert np.array_equal(spk != 0, source & (levels > 0) & (small >= 0))   # every candidate speaks
    # ... and with N = 1 in rooms of several sources it is not
    assert not np.array_equal(np_speakers_mix(x, order, start, 1, muted, is_cn)[0], mix)


def test_model_tie_rule_and_candidates():
    levels = np.array([5, 9, 9, 0, 9, 7, 9], np.int64)
    order, start = np.array([6, 1, 3, 4, 2, 0, 5], np.int32), np.array([0, 5, 7], np.int32)
    source = np.array([1, 1, 1, 1, 1, 1, 0], bool)       # row 6, first in the room's order, is muted
    speakers, flags = np_select(levels, order, start, source, 2)
    assert speakers == [[1, 4], [5, 0]]                  # equal levels: positions 1 and 3 beat position 4 (row 2)
    assert flags.tolist() == [1, 1, 0, 0, 1, 1, 0]
    speakers, flags = np_select(levels, order, start, source, 8)
    assert speakers == [[1, 4, 2], [5, 0]] and flags[3] == 0      # a zero-level row is never a speaker
    x = np.zeros((7, 320), np.int16)
    x[:, 0] = [1, 3, 3, 0, 3, 2, 3]
    mix, lv, spk = np_speakers_mix(x, order, start, 2, (~source).astype(np.int32))
    assert lv.tolist() == [1, 9, 9, 0, 9, 4, 9] and spk.tolist() == [1, 1, 0, 0, 1, 1, 0]
    assert mix[:, 0].tolist() == [2, 3, 6, 6, 3, 1, 6] and not mix[:, 1:].any()


def test_the_kernel_cases_hold_their_own_assertions():
    x, rooms, muted, is_cn, order, start = speakers_kernel_case()
    assert x.shape == (330, 320) and sorted(np.diff(start).tolist()) == [1, 2, 3, 8, 9, 16, 17, 257]
    plain = np_bridge_plan(rooms)[0]
    assert sorted(order.tolist()) == sorted(plain.tolist()) and not np.array_equal(order, plain)
    x, rooms, muted, order, start = threshold_case()
    assert np.diff(start).tolist() == [63, 64, 65, 129] and np.unique(np_levels(x)).size == 4


# ---- 3. the class -----------------------------------------------------------------------------------------------------------

def test_speaker_bridge_host_logic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "speaker_class_test")
    subprocess.check_call(SAN + ["-I" + HOST, "-I" + os.path.join(HOST, "shims"), "-I" + ROOT, "-I" + HERE,
                                 "-I" + os.path.join(ROOT, "tests", "bridge"), "-o", exe,
                                 os.path.join(HERE, "speaker_class_test.cc"), os.path.join(HERE, "fake_speakers_abi.cc"),
                                 os.path.join(ROOT, "tests", "bridge", "fake_bridge_abi.cc"),
                                 os.path.join(HOST, "lyra_speaker_bridge.cc"), os.path.join(HOST, "lyra_conference_bridge.cc"),
                                 os.path.join(ROOT, "tests", "host_stub", "fake_lyra_hip_codec.cc")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=SAN_ENV)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_each_bridge_class_references_its_own_calls_only(tmp_path):
    syms = {}
    for name in ("lyra_conference_bridge", "lyra_speaker_bridge"):
        obj = str(tmp_path / (name + ".o"))
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + HOST, "-I" + os.path.join(HOST, "shims"), "-I" + ROOT, "-c",
                               os.path.join(HOST, name + ".cc"), "-o", obj], timeout=600)
        syms[name] = subprocess.check_output(["nm", "-C", "--undefined-only", obj], text=True)
    old, new = syms["lyra_conference_bridge"], syms["lyra_speaker_bridge"]
    assert "lyra_hip_speakers" not in old and "LyraSpeakerBridge" not in old
    assert "lyra_hip_speakers_begin" in new and "lyra_hip_speakers_end" in new
    assert "lyra_hip_bridge" not in new and "decode_streams" not in new and "encode_streams" not in new
