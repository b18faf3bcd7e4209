"""A meeting recording through the bridge, the parts that need no GPU (include/lyra_hip_bridge_spans.h):
1. the header, the ctypes table of lyra_amd/codec.py (_SIGNATURES_BRIDGE_SPANS, with a loader of its own), the call struct and
   the built library agree; a null context is refused; LyraHip has the methods; the pass's kernels are in the library's gfx950
   code object; the tick calls' header is still the only one that declares names starting with lyra_hip_bridge;
2. the planner: lyra_hip_spans_bridge_plan against the numpy restatement of tests/bridge_models.py, what it refuses, T = 0, and
   the bound on a room's size;
3. the Python binding refuses shapes that do not fit before it calls the library;
4. the host-only parts -- lyra_amd/csrc/bridge_spans_plan.h and the segment cutting of BridgeRecordingTimeParallel
   (lyra_amd/host/lyra_bridge_recording.h) -- through tests/bridge/bridge_recording_test.cc, a program of its own built with
   -fsanitize=address,undefined and run as a program."""
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
NEW = {"lyra_hip_spans_bridge_plan": 8, "lyra_hip_spans_bridge_mix_dev": 11, "lyra_hip_spans_bridge_dev": 2,
       "lyra_hip_spans_bridge": 21}
SAN = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return load_library()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lyra_hip_bridge_spans.h")).read(), flags=re.S)


def test_header_table_and_library_agree_on_the_four_symbols(lib):
    protos = _protos("lyra_hip_bridge_spans.h")
    assert set(protos) == set(NEW) == set(codec._SIGNATURES_BRIDGE_SPANS)
    for name, n_args in NEW.items():
        args = [a.strip() for a in protos[name].split(",")]
        assert len(args) == n_args, (name, args)
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name} is not exported by {codec.library_path()}"
        restype, argtypes = codec._SIGNATURES_BRIDGE_SPANS[name]
        assert restype is codec.C.c_int and fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        for a, t in zip(args, argtypes):   # pointers as void pointers, `unsigned` as one, everything else an int
            want = codec.C.c_void_p if "*" in a else codec.C.c_uint if a.startswith("unsigned ") else codec.C.c_int
            assert t is want, (name, a, t)
    others = (codec._SIGNATURES, codec._SIGNATURES_SPANS_MIXED, codec._SIGNATURES_SPANS_RATES, codec._SIGNATURES_SPANS_PACKED,
              codec._SIGNATURES_BRIDGE, codec._SIGNATURES_SPEAKERS, codec._SIGNATURES_SHARED)
    assert not any(set(NEW) & set(t) for t in others)


def test_the_call_struct_is_the_headers():
    body = re.search(r"typedef struct lyra_hip_spans_bridge_call \{(.*?)\} lyra_hip_spans_bridge_call;", _header(), flags=re.S).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert [re.split(r"[\s*]+", f)[-1] for f in fields] == [n for n, _ in codec.BridgeSpansCall._fields_]
    for f, (name, t) in zip(fields, codec.BridgeSpansCall._fields_):
        want = codec.C.c_void_p if "*" in f else codec.C.c_uint if f.startswith("unsigned ") else codec.C.c_int
        assert t is want, (f, t)


def test_the_header_builds_on_the_selection_and_the_span_headers():
    text = open(os.path.join(ROOT, "include", "lyra_hip_bridge_spans.h")).read()
    assert '#include "lyra_hip_speakers.h"' in text and '#include "lyra_hip_spans_mixed.h"' in text
    # the older headers say nothing of the new calls outside comments, and the tick calls' header keeps its prefix to itself
    inc = os.path.join(ROOT, "include")
    for header in sorted(os.listdir(inc)):
        stripped = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, header)).read(), flags=re.S)
        if header != "lyra_hip_bridge_spans.h":
            assert "spans_bridge" not in stripped, header
        if header != "lyra_hip_bridge.h":
            assert "lyra_hip_bridge" not in stripped, header
    assert codec.SPEAKERS_SKIP_COMFORT_NOISE == codec.BRIDGE_SKIP_COMFORT_NOISE


def test_a_null_context_is_refused(lib):
    for name in set(NEW) - {"lyra_hip_spans_bridge_plan"}:
        args = [None if t is codec.C.c_void_p else 0 for t in codec._SIGNATURES_BRIDGE_SPANS[name][1]]
        assert getattr(lib, name)(*args) < 0, name


def test_lyrahip_has_the_methods():
    for name in ("bridge_spans_mix_dev", "bridge_spans_dev", "bridge_spans", "bridge_spans_plan"):
        assert callable(getattr(codec.LyraHip, name, None)), name
    assert callable(codec.bridge_spans_plan)


def test_the_kernels_are_in_the_gfx950_code_object():
    image = open(codec.library_path(), "rb").read()
    assert set(re.findall(rb"hip[v\d]*-amdgcn-amd-amdhsa--(gfx\w+)", image)) == {b"gfx950"}
    for kernel in (b"bridge_spans_mix_kernel", b"bridge_spans_zero_kernel", b"bridge_spans_level_kernel",
                   b"bridge_spans_select_kernel", b"bridge_spans_speakers_mix_kernel"):
        assert re.search(rb"_ZN4lyra\d+" + kernel + rb"E\w*\.kd", image), kernel


# ---- 2. the planner ---------------------------------------------------------------------------------------------------------

def _rooms_case():
    """rooms of 1, 2, 3, 8, 9 and 17 members under non-contiguous labels, the 17 scattered over the participants, some in no room"""
    rng = np.random.default_rng(5)
    P = 48
    rooms = np.full(P, -1, np.int32)
    free = rng.permutation(P)
    rooms[free[:17]] = 1000
    rest = np.sort(free[17:])
    at = 0
    for label, n in ((3, 1), (70, 2), (5, 3), (2 ** 31 - 1, 8), (12, 9)):
        rooms[rest[at:at + n]] = label
        at += n
    rooms[rest[at]] = -9
    assert (rooms < 0).sum() == P - 40
    return rooms


def _spans_for(P, T, gap=2):
    return [(100 + p, p * (T + gap), T) for p in range(P)]


def _plan_raw(lib, spans, rooms, P=None, null=()):
    sp = codec._spans(spans)
    rooms = np.ascontiguousarray(rooms, np.int32)
    P = sp.size if P is None else P
    order, start = np.zeros(max(P, 1), np.int32), np.zeros(max(P, 0) + 1, np.int32)
    n_rooms, n_members, n_ticks = codec.C.c_int(-5), codec.C.c_int(-5), codec.C.c_int64(-5)
    args = dict(spans=sp.ctypes.data, rooms=rooms.ctypes.data, order=order.ctypes.data, start=start.ctypes.data,
                n_rooms=codec.C.addressof(n_rooms), n_members=codec.C.addressof(n_members), n_ticks=codec.C.addressof(n_ticks))
    for k in null:
        args[k] = None
    rc = lib.lyra_hip_spans_bridge_plan(args["spans"], P, args["rooms"], args["order"], args["start"], args["n_rooms"],
                                        args["n_members"], args["n_ticks"])
    return rc, order, start, n_rooms.value, n_members.value, n_ticks.value


def test_planner_equals_the_restatement(lib):
    rooms = _rooms_case()
    order, start = np_bridge_plan(rooms)
    assert sorted(np.diff(start).tolist()) == [1, 2, 3, 8, 9, 17]
    assert (np.diff(order[start[-2]:start[-1]]) > 1).any(), "the 17-room (the largest label but one) is scattered"
    for T in (0, 1, 250):
        got = codec.bridge_spans_plan(_spans_for(rooms.size, T), rooms)
        assert np.array_equal(got[0], order) and np.array_equal(got[1], start) and got[2] == T, T
    rc, o, s, n_rooms, n_members, n_ticks = _plan_raw(lib, _spans_for(rooms.size, 7), rooms)
    assert (rc, n_rooms, n_members, n_ticks) == (0, 6, 40, 7)
    # everybody in no room; one participant
    got = codec.bridge_spans_plan(_spans_for(5, 3), np.full(5, -1))
    assert got[0].size == 0 and got[1].tolist() == [0] and got[2] == 3
    got = codec.bridge_spans_plan([(7, 11, 4)], [6])
    assert got[0].tolist() == [0] and got[1].tolist() == [0, 1] and got[2] == 4


def test_an_empty_recording_is_accepted_and_yields_its_plan(lib):
    rooms = np.array([2, 2, -1, 0], np.int32)
    spans = [(9, 0, 0), (3, 0, 0), (4, 5, 0), (1, 5, 0)]       # no frames: the ranges name nothing and cannot overlap
    rc, order, start, n_rooms, n_members, n_ticks = _plan_raw(lib, spans, rooms)
    assert (rc, n_rooms, n_members, n_ticks) == (0, 2, 3, 0)
    assert order[:3].tolist() == [3, 0, 1] and start[:3].tolist() == [0, 1, 3]


def test_planner_refusals(lib):
    rooms = np.array([0, 0, 1, -1], np.int32)
    good = [(5, 0, 10), (6, 10, 10), (2, 25, 10), (9, 40, 10)]
    assert _plan_raw(lib, good, rooms)[0] == 0
    bad = {"unequal n_frames": [(5, 0, 10), (6, 10, 9), (2, 25, 10), (9, 40, 10)],
           "overlapping spans": [(5, 0, 10), (6, 9, 10), (2, 25, 10), (9, 40, 10)],
           "a duplicate id": [(5, 0, 10), (6, 10, 10), (5, 25, 10), (9, 40, 10)],
           "a negative first frame": [(5, -1, 10), (6, 10, 10), (2, 25, 10), (9, 40, 10)],
           "a negative n_frames": [(5, 0, -1), (6, 10, -1), (2, 25, -1), (9, 40, -1)],
           "a negative id": [(5, 0, 10), (-6, 10, 10), (2, 25, 10), (9, 40, 10)]}
    for what, spans in bad.items():
        assert _plan_raw(lib, spans, rooms)[0] == EINVAL, what
        with pytest.raises(codec.LyraHipError):
            codec.bridge_spans_plan(spans, rooms)
    for k in ("spans", "rooms", "order", "start", "n_rooms", "n_members", "n_ticks"):
        assert _plan_raw(lib, good, rooms, null=(k,))[0] == EINVAL, f"null {k}"
    assert _plan_raw(lib, good, rooms, P=0)[0] == EINVAL and _plan_raw(lib, good, rooms, P=-1)[0] == EINVAL
    # more span frames than one call takes: 2^30 - 1 in all
    assert _plan_raw(lib, [(0, 0, 2 ** 29), (1, 2 ** 29, 2 ** 29)], [0, 0])[0] == EINVAL
    assert _plan_raw(lib, [(0, 0, 2 ** 29 - 1), (1, 2 ** 29, 2 ** 29 - 1)], [0, 0])[0] == 0


def test_planner_holds_the_bound_on_a_rooms_size(lib):
    P = MAX_ROOM + 2
    spans = np.zeros(P, codec.SPAN_DTYPE)
    spans["stream_id"], spans["first_frame"], spans["n_frames"] = np.arange(P), np.arange(P) * 2, 2
    rooms = np.full(P, 4, np.int32)
    assert _plan_raw(lib, spans, rooms)[0] == EINVAL
    rooms[[0, P - 1]] = -1
    rc, order, start, n_rooms, n_members, _ = _plan_raw(lib, spans, rooms)
    assert (rc, n_rooms, n_members) == (0, 1, MAX_ROOM) and np.array_equal(order[:MAX_ROOM], np.arange(1, P - 1))


# ---- 3. the binding ---------------------------------------------------------------------------------------------------------

class _NoLibrary:
    """stands in for the library handle: any call of it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the binding called {name} with arguments whose shapes do not fit")


def test_the_binding_raises_on_bad_shapes_before_calling_the_library():
    h = object.__new__(codec.LyraHip)          # no context: the checks below come before any use of one
    h.L, h.h, h.device, h.torch_order = _NoLibrary(), None, 0, False
    packets = np.zeros((30, 23), np.uint8)
    sizes, bits = np.zeros(30, np.int32), np.full(30, 64, np.int32)
    good = [(0, 0, 10), (1, 10, 10), (2, 20, 10)]
    cases = {"rooms of another length": dict(spans=good, rooms=[0, 0]),
             "no participants": dict(spans=[], rooms=[]),
             "unequal n_frames": dict(spans=[(0, 0, 10), (1, 10, 9), (2, 20, 10)], rooms=[0, 0, 0]),
             "a span outside the buffer": dict(spans=[(0, 0, 10), (1, 10, 10), (2, 21, 10)], rooms=[0, 0, 0]),
             "packet_bytes of another length": dict(spans=good, rooms=[0, 0, 0], packet_bytes=sizes[:29]),
             "num_bits of another length": dict(spans=good, rooms=[0, 0, 0], num_bits=bits[:7]),
             "muted of another length": dict(spans=good, rooms=[0, 0, 0], muted=np.zeros(31, np.int32)),
             "dtx of another length": dict(spans=good, rooms=[0, 0, 0], dtx=[1, 0])}
    for what, kw in cases.items():
        args = dict(spans=good, rooms=[0, 0, 0], packets=packets, packet_bytes=sizes, num_bits=bits)
        args.update(kw)
        with pytest.raises((codec.LyraHipError, ValueError)):
            h.bridge_spans(**args)
    for what in ("rooms of another length", "no participants", "unequal n_frames"):
        with pytest.raises(codec.LyraHipError):
            codec.bridge_spans_plan(cases[what]["spans"], cases[what]["rooms"], _NoLibrary())


# ---- 4. the host-only parts, as a program under the sanitizers ----------------------------------------------------------------

@pytest.fixture(scope="module")
def recording_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bridge_recording") / "bridge_recording_test")
    subprocess.check_call(SAN + ["-I" + os.path.join(ROOT, "lyra_amd", "csrc"), "-I" + HOST, "-I" + os.path.join(HOST, "shims"),
                                 "-I" + ROOT, "-o", exe, os.path.join(ROOT, "tests", "bridge", "bridge_recording_test.cc")])
    return exe


def _np_segment_starts(script):
    rooms = np.where(script[:, :, 0] < 0, -1, script[:, :, 0])
    return [0] + [t for t in range(1, len(rooms)) if (rooms[t] != rooms[t - 1]).any()] if len(rooms) else []


def _scripts():
    rng = np.random.default_rng(9)
    T, n, k = 40, 7, 23

    def base():
        s = np.zeros((T, n, 3), np.int32)
        s[:, :, 0] = (np.arange(n) // 3)[None, :]
        s[:, :, 1] = rng.random((T, n)) < 0.3          # mutes and bitrates change all the time: they cut nothing
        s[:, :, 2] = rng.choice([3200, 6000, 9200], (T, n))
        return s
    none = base()
    changes = base()
    changes[1:, 2, 0] = 5                               # tick 0 is a segment's first whatever happens; a change right behind it,
    changes[k:, 4, 0] = -1                              # one at tick k
    changes[T - 1:, 0, 0] = 9                           # and one at the last tick
    no_room = base()
    no_room[:, 6, 0] = -1
    no_room[10:, 6, 0] = -4                             # two negative labels are the same "no room": no cut
    return {"no change": (none, [0]), "changes at 1, k and T - 1": (changes, [0, 1, k, T - 1]), "another negative label": (no_room, [0]),
            "one tick": (base()[:1], [0]), "no tick": (base()[:0], [])}


@pytest.mark.parametrize("case", list(_scripts()))
def test_segment_cutting_program_under_sanitizers(recording_exe, tmp_path, case):
    script, want = _scripts()[case]
    assert _np_segment_starts(script) == want
    path = str(tmp_path / "script.i32")
    script.tofile(path)
    r = subprocess.run([recording_exe, path, str(script.shape[1])], capture_output=True, text=True, timeout=120, env=SAN_ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    lines = r.stdout.split("\n")
    assert [int(v) for v in lines[0].split()] == want and lines[1] == "ok"
