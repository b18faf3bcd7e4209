"""A meeting with a schedule through the bridge, the parts that need no GPU (include/lyra_hip_spans_meeting.h):
1. the header, the ctypes table of lyra_amd/codec.py (_SIGNATURES_SPANS_MEETING, with a loader of its own), the two structs and
   the built library agree; no older table names the calls; the header keeps clear of the other conference headers' names; a
   null context is refused; LyraHip has the methods; the pass's kernels are in the library's gfx950 code object;
2. the planner: lyra_hip_spans_meeting_plan against the numpy restatement of tests/meeting_cases.py on drawn schedules and on
   the named shapes (epochs of one tick, a room that empties, a room that appears, a gap, no stay, T = 0), and every refusal;
3. lyra_amd/csrc/meeting_plan.h through tests/meeting/meeting_plan_test.cc, a program of its own built with
   -fsanitize=address,undefined and run as a program."""
import os
import re
import subprocess

import numpy as np
import pytest

from lyra_amd import codec

from abi_loading import _protos, load_library
from bridge_models import MAX_ROOM
from meeting_cases import as_stays, draw_schedule, np_meeting_plan, present_ticks

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HEADER = "lyra_hip_spans_meeting.h"
NEW = {"lyra_hip_spans_meeting_plan": 11, "lyra_hip_spans_meeting_mix_dev": 12, "lyra_hip_spans_meeting_dev": 2,
       "lyra_hip_spans_meeting": 22}
SAN = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return load_library()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)


def _ctype_of(decl):
    return codec.C.c_void_p if "*" in decl else codec.C.c_uint if decl.startswith("unsigned ") else codec.C.c_int


# ---- 1. header, table, structs, library -------------------------------------------------------------------------------------

def test_header_table_and_library_agree_on_the_four_symbols(lib):
    protos = _protos(HEADER)
    assert set(protos) == set(NEW) == set(codec._SIGNATURES_SPANS_MEETING)
    for name, n_args in NEW.items():
        args = [a.strip() for a in protos[name].split(",")]
        assert len(args) == n_args, (name, args)
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name} is not exported by {codec.library_path()}"
        restype, argtypes = codec._SIGNATURES_SPANS_MEETING[name]
        assert restype is codec.C.c_int and fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        for a, t in zip(args, argtypes):
            assert t is _ctype_of(a), (name, a, t)
    others = (codec._SIGNATURES, codec._SIGNATURES_SPANS_MIXED, codec._SIGNATURES_SPANS_RATES, codec._SIGNATURES_SPANS_PACKED,
              codec._SIGNATURES_ENCODE_STREAMS, codec._SIGNATURES_DECODE_STREAMS, codec._SIGNATURES_DECODE_SAMPLES_ANY,
              codec._SIGNATURES_DECODE_SAMPLES_STREAMS, codec._SIGNATURES_BRIDGE, codec._SIGNATURES_SPEAKERS, codec._SIGNATURES_SHARED,
              codec._SIGNATURES_BRIDGE_SPANS)
    assert not any(set(NEW) & set(t) for t in others)
    assert len(codec._SIGNATURES_BRIDGE_SPANS) == 4, "the recording call's table keeps its four"


def test_the_structs_are_the_headers():
    body = re.search(r"typedef struct lyra_hip_spans_meeting_call \{(.*?)\} lyra_hip_spans_meeting_call;", _header(), flags=re.S).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert [re.split(r"[\s*]+", f)[-1] for f in fields] == [n for n, _ in codec.MeetingSpansCall._fields_]
    for f, (name, t) in zip(fields, codec.MeetingSpansCall._fields_):
        assert t is _ctype_of(f), (f, t)
    assert "stays" in dict(codec.MeetingSpansCall._fields_) and "rooms" not in dict(codec.MeetingSpansCall._fields_)
    body = re.search(r"typedef struct lyra_hip_meeting_stay \{(.*?)\} lyra_hip_meeting_stay;", _header(), flags=re.S).group(1)
    fields = [f.strip().split() for f in body.split(";") if f.strip()]
    widths = {"int32_t": 4, "int64_t": 8}
    dt = codec.MEETING_STAY_DTYPE
    assert [f[1] for f in fields] == list(dt.names)
    assert [widths[f[0]] for f in fields] == [dt[n].itemsize for n in dt.names]
    assert dt.itemsize == 24 and [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 16]
    m = re.search(r"#define LYRA_HIP_MEETING_MAX_ENTRIES \(1 << (\d+)\)", _header())
    assert m and 1 << int(m.group(1)) == codec.MEETING_MAX_ENTRIES


def test_the_header_keeps_clear_of_the_other_conference_names():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "lyra_hip_speakers.h"' in text and '#include "lyra_hip_spans_mixed.h"' in text
    stripped = _header()
    assert "spans_bridge" not in stripped and "lyra_hip_bridge" not in stripped
    assert len(re.findall(r"#include", stripped)) == 2
    # the older headers say nothing of the new calls outside comments
    inc = os.path.join(ROOT, "include")
    for header in sorted(os.listdir(inc)):
        if header != HEADER:
            assert "spans_meeting" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, header)).read(), flags=re.S), header
    assert set(_protos("lyra_hip_bridge_spans.h")) == set(codec._SIGNATURES_BRIDGE_SPANS)


def test_a_null_context_is_refused(lib):
    for name in set(NEW) - {"lyra_hip_spans_meeting_plan"}:
        args = [None if t is codec.C.c_void_p else 0 for t in codec._SIGNATURES_SPANS_MEETING[name][1]]
        assert getattr(lib, name)(*args) < 0, name


def test_lyrahip_has_the_methods():
    for name in ("meeting_spans_mix_dev", "meeting_spans_dev", "meeting_spans", "meeting_plan"):
        assert callable(getattr(codec.LyraHip, name, None)), name
    assert callable(codec.meeting_plan)


def test_the_kernels_are_in_the_gfx950_code_object():
    image = open(codec.library_path(), "rb").read()
    assert set(re.findall(rb"hip[v\d]*-amdgcn-amd-amdhsa--(gfx\w+)", image)) == {b"gfx950"}
    for kernel in (b"meeting_mix_kernel", b"meeting_zero_kernel", b"meeting_level_kernel", b"meeting_select_kernel",
                   b"meeting_speakers_mix_kernel"):
        assert re.search(rb"_ZN4lyra\d+" + kernel + rb"E\w*\.kd", image), kernel


# ---- 2. the planner ---------------------------------------------------------------------------------------------------------

def _spans_for(stays, P, gap=2, ids=None):
    at, spans = 0, []
    for p in range(P):
        n = len(present_ticks(stays, p))
        spans.append((100 + p if ids is None else ids[p], at, n))
        at += n + gap
    return spans


def _plan_raw(lib, spans, stays, P=None, n_stays=None, null=(), sized=None):
    """the C call -> (rc, n_epochs, n_entries, n_ticks, arrays); the four arrays are sized by `sized` = (epochs, entries)"""
    sp = codec._spans(spans)
    st = stays if isinstance(stays, np.ndarray) else np.array([tuple(s) for s in stays], codec.MEETING_STAY_DTYPE).reshape(-1)
    P = sp.size if P is None else P
    n_stays = st.size if n_stays is None else n_stays
    E, N = sized or (2 * st.size + 1, 0)
    arrays = dict(epoch_tick=np.full(E + 1, -7, np.int64), epoch_entry=np.full(E + 1, -7, np.int64),
                  entry_participant=np.full(max(N, 1), -7, np.int32), entry_room=np.full(max(N, 1), -7, np.int32))
    counts = [codec.C.c_int64(-5) for _ in range(3)]
    args = dict(spans=sp.ctypes.data, stays=st.ctypes.data if st.size else None, n_epochs=codec.C.addressof(counts[0]),
                n_entries=codec.C.addressof(counts[1]), n_ticks=codec.C.addressof(counts[2]))
    args.update({k: v.ctypes.data if sized else None for k, v in arrays.items()})
    for k in null:
        args[k] = None
    rc = lib.lyra_hip_spans_meeting_plan(args["spans"], P, args["stays"], n_stays, args["n_epochs"], args["n_entries"], args["n_ticks"],
                                         args["epoch_tick"], args["epoch_entry"], args["entry_participant"], args["entry_room"])
    return (rc, *[c.value for c in counts], arrays)


def _assert_plan(got, want, what):
    assert got["n_ticks"] == want["n_ticks"], what
    for k in ("epoch_tick", "epoch_entry", "entry_participant", "entry_room"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k][:40], want[k][:40])


def _named_schedules():
    """P = 6; participant 5 never shows up"""
    return {
        # three epochs of one tick each: every tick somebody comes or goes
        "epochs of one tick": [(0, 4, 0, 3), (1, 4, 1, 2), (2, 9, 0, 2), (3, -1, 2, 1)],
        # room 9 holds 2 and 3 until tick 5 and is empty afterwards; room 1 does not exist before tick 7
        "a room empties, a room appears": [(0, 4, 0, 10), (1, 4, 0, 10), (2, 9, 0, 5), (3, 9, 0, 5), (4, 1, 7, 3)],
        # participant 1 is away for ticks 3 .. 5 and comes back into another room; 2 moves rooms at tick 4 without a gap
        "a gap and a move": [(0, 4, 0, 8), (1, 4, 0, 3), (1, 2, 6, 2), (2, 4, 0, 4), (2, 2, 4, 4), (3, -3, 1, 6)],
        # nobody is present on ticks 2 .. 3: an epoch without entries; the meeting starts at tick 1
        "an empty stretch": [(0, 4, 1, 1), (1, 4, 1, 1), (0, 4, 4, 2), (2, 0, 4, 1)],
    }


def test_planner_equals_the_restatement_on_named_schedules(lib):
    for what, stays in _named_schedules().items():
        stays = as_stays(stays)
        spans = _spans_for(stays, 6)
        want = np_meeting_plan(spans, stays)
        _assert_plan(codec.meeting_plan(spans, stays), want, what)
        rc, n_epochs, n_entries, n_ticks, _ = _plan_raw(lib, spans, stays)       # the sizing call writes no array
        assert (rc, n_epochs, n_entries, n_ticks) == (0, len(want["epoch_tick"]) - 1, len(want["entry_participant"]), want["n_ticks"]), what
    want = np_meeting_plan(_spans_for(as_stays(_named_schedules()["epochs of one tick"]), 6), as_stays(_named_schedules()["epochs of one tick"]))
    assert want["epoch_tick"].tolist() == [0, 1, 2, 3] and want["epoch_entry"].tolist() == [0, 2, 5, 8]
    assert want["entry_participant"].tolist() == [0, 2, 0, 1, 2, 0, 1, 3]
    assert want["entry_room"].tolist() == [0, 1, 0, 0, 1, 0, 0, -1]
    want = np_meeting_plan(_spans_for(as_stays(_named_schedules()["an empty stretch"]), 6), as_stays(_named_schedules()["an empty stretch"]))
    assert want["epoch_tick"].tolist() == [1, 2, 4, 5, 6] and want["epoch_entry"].tolist() == [0, 2, 2, 4, 5] and want["n_ticks"] == 6


@pytest.mark.parametrize("seed", range(6))
def test_planner_equals_the_restatement_on_drawn_schedules(seed):
    rng = np.random.default_rng(300 + seed)
    P, T = int(rng.integers(3, 40)), int(rng.integers(2, 60))
    stays = draw_schedule(rng, P, T, n_rooms=int(rng.integers(1, 5)), events=int(rng.integers(0, 40)), no_room=0.2)
    spans = _spans_for(stays, P, ids=rng.permutation(500)[:P].tolist())
    assert any(n == 0 for (_, _, n) in spans), "a participant with no stay"
    _assert_plan(codec.meeting_plan(spans, stays), np_meeting_plan(spans, stays), seed)


def test_an_empty_meeting_is_accepted(lib):
    spans = [(9, 0, 0), (3, 0, 0), (4, 5, 0)]
    rc, n_epochs, n_entries, n_ticks, arrays = _plan_raw(lib, spans, [], sized=(0, 0))
    assert (rc, n_epochs, n_entries, n_ticks) == (0, 0, 0, 0)
    assert arrays["epoch_tick"].tolist() == [0] and arrays["epoch_entry"].tolist() == [0]
    got = codec.meeting_plan(spans, [])
    assert got["n_ticks"] == 0 and got["entry_participant"].size == 0


def test_planner_refusals(lib):
    good_stays = [(0, 0, 0, 10), (1, 0, 2, 4), (1, 1, 6, 3), (2, -1, 5, 5)]
    good = [(5, 0, 10), (6, 10, 7), (2, 25, 5), (9, 40, 0)]
    assert _plan_raw(lib, good, good_stays)[0] == 0
    bad_spans = {"overlapping spans": [(5, 0, 10), (6, 9, 7), (2, 25, 5), (9, 40, 0)],
                 "a duplicate id": [(5, 0, 10), (6, 10, 7), (5, 25, 5), (9, 40, 0)],
                 "a duplicate id of a participant with no stay": [(5, 0, 10), (6, 10, 7), (2, 25, 5), (6, 40, 0)],
                 "a negative first frame": [(5, -1, 10), (6, 10, 7), (2, 25, 5), (9, 40, 0)],
                 "a negative n_frames": [(5, 0, 10), (6, 10, 7), (2, 25, 5), (9, 40, -1)],
                 "a negative id": [(5, 0, 10), (-6, 10, 7), (2, 25, 5), (9, 40, 0)],
                 "n_frames above the stays' sum": [(5, 0, 10), (6, 10, 8), (2, 25, 5), (9, 40, 0)],
                 "n_frames below the stays' sum": [(5, 0, 9), (6, 10, 7), (2, 25, 5), (9, 40, 0)],
                 "frames without a stay": [(5, 0, 10), (6, 10, 7), (2, 25, 5), (9, 40, 1)]}
    for what, spans in bad_spans.items():
        assert _plan_raw(lib, spans, good_stays)[0] == EINVAL, what
    bad_stays = {"unsorted participants": [(1, 0, 2, 4), (0, 0, 0, 10), (1, 1, 6, 3), (2, -1, 5, 5)],
                 "unsorted ticks": [(0, 0, 0, 10), (1, 1, 6, 3), (1, 0, 2, 4), (2, -1, 5, 5)],
                 "overlapping stays": [(0, 0, 0, 10), (1, 0, 2, 5), (1, 1, 6, 2), (2, -1, 5, 5)],
                 "n_ticks 0": [(0, 0, 0, 10), (1, 0, 2, 7), (1, 1, 9, 0), (2, -1, 5, 5)],
                 "a negative n_ticks": [(0, 0, 0, 10), (1, 0, 2, 8), (1, 1, 10, -1), (2, -1, 5, 5)],
                 "a negative first_tick": [(0, 0, -1, 10), (1, 0, 2, 4), (1, 1, 6, 3), (2, -1, 5, 5)],
                 "a participant out of range": [(0, 0, 0, 10), (1, 0, 2, 4), (1, 1, 6, 3), (4, -1, 5, 5)],
                 "a negative participant": [(-1, 0, 0, 10), (1, 0, 2, 4), (1, 1, 6, 3), (2, -1, 5, 5)]}
    for what, stays in bad_stays.items():
        assert _plan_raw(lib, good, stays)[0] == EINVAL, what
    for what in ("unsorted participants", "overlapping stays"):
        with pytest.raises(codec.LyraHipError):
            codec.meeting_plan(good, bad_stays[what])
    for k in ("spans", "stays", "n_epochs", "n_entries", "n_ticks"):
        assert _plan_raw(lib, good, good_stays, null=(k,))[0] == EINVAL, f"null {k}"
    assert _plan_raw(lib, good, good_stays, P=0)[0] == EINVAL and _plan_raw(lib, good, good_stays, P=-1)[0] == EINVAL
    assert _plan_raw(lib, good, good_stays, n_stays=-1)[0] == EINVAL
    # more span frames than one call takes: 2^30 - 1 in all
    assert _plan_raw(lib, [(0, 0, 2 ** 29), (1, 2 ** 29, 2 ** 29)], [(0, 0, 0, 2 ** 29), (1, 0, 0, 2 ** 29)])[0] == EINVAL
    assert _plan_raw(lib, [(0, 0, 2 ** 29 - 1), (1, 2 ** 29, 2 ** 29)], [(0, 0, 0, 2 ** 29 - 1), (1, 0, 0, 2 ** 29)])[0] == 0


def test_planner_holds_the_bound_on_a_rooms_size_in_one_epoch_only(lib):
    """MAX_ROOM members throughout; one more is in the room for one tick in the middle: that epoch alone is too large"""
    P = MAX_ROOM + 1
    stays = np.zeros(P, codec.MEETING_STAY_DTYPE)
    stays["participant"], stays["room"], stays["first_tick"], stays["n_ticks"] = np.arange(P), 4, 0, 3
    stays[P - 1] = (P - 1, 4, 1, 1)
    spans = np.zeros(P, codec.SPAN_DTYPE)
    spans["stream_id"], spans["first_frame"], spans["n_frames"] = np.arange(P), np.arange(P) * 3, stays["n_ticks"]
    assert _plan_raw(lib, spans, stays)[0] == EINVAL
    stays["room"][P - 1] = 5                          # next door it fits
    rc, n_epochs, n_entries, n_ticks, _ = _plan_raw(lib, spans, stays)
    assert (rc, n_epochs, n_entries, n_ticks) == (0, 3, 3 * MAX_ROOM + 1, 3)
    stays["room"][P - 1] = -1                         # and so it does in no room
    assert _plan_raw(lib, spans, stays)[0] == 0


def test_planner_refuses_one_entry_above_the_bound(lib):
    """2048 participants present throughout 2047 epochs of one tick, which a flickering participant cuts (present on every other
    tick: 1024 entries), and one more who is present for the first m ticks: 2048 * 2047 + 1024 + m entries"""
    A, k = 2048, 1024
    T = 2 * k - 1
    for m, want in ((1024, 0), (1025, EINVAL)):
        stays = [(p, p % 5, 0, T) for p in range(A)] + [(A, 1, 2 * i, 1) for i in range(k)] + [(A + 1, 2, 0, m)]
        n = [T] * A + [k, m]
        spans = np.zeros(A + 2, codec.SPAN_DTYPE)
        spans["stream_id"], spans["n_frames"] = np.arange(A + 2), n
        spans["first_frame"] = np.concatenate([[0], np.cumsum(n)[:-1]])
        rc, n_epochs, n_entries, _, _ = _plan_raw(lib, spans, stays)
        assert rc == want, m
        if not want:
            assert (n_epochs, n_entries) == (T, codec.MEETING_MAX_ENTRIES)


# ---- 3. the host-only planner, as a program under the sanitizers ---------------------------------------------------------------

@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("meeting_plan") / "meeting_plan_test")
    subprocess.check_call(SAN + ["-I" + os.path.join(ROOT, "lyra_amd", "csrc"), "-o", exe,
                                 os.path.join(ROOT, "tests", "meeting", "meeting_plan_test.cc")])
    return exe


def _run_plan(exe, tmp_path, spans, stays):
    flat = [len(spans), len(stays)] + [v for s in spans for v in s] + [v for s in stays for v in s]
    path = str(tmp_path / "in.i64")
    np.array(flat, np.int64).tofile(path)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120, env=SAN_ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-4000:])
    return r.stdout.split("\n")


def _drawn(seed):
    rng = np.random.default_rng(400 + seed)
    P, T = 17, 30
    stays = draw_schedule(rng, P, T, n_rooms=3, events=25, no_room=0.2)
    return _spans_for(stays, P), stays


@pytest.mark.parametrize("case", list(_named_schedules()) + ["drawn 0", "drawn 1", "no stays"])
def test_planner_program_under_sanitizers(plan_exe, tmp_path, case):
    if case in _named_schedules():
        stays = as_stays(_named_schedules()[case])
        spans = _spans_for(stays, 6)
    elif case == "no stays":
        spans, stays = [(1, 0, 0), (2, 0, 0)], []
    else:
        spans, stays = _drawn(int(case.split()[1]))
    want = np_meeting_plan(spans, stays)
    lines = _run_plan(plan_exe, tmp_path, spans, stays)
    assert lines[0] != "refused", case
    assert int(lines[0]) == want["n_ticks"]
    for k, text in zip(("epoch_tick", "epoch_entry", "entry_participant", "entry_room"), lines[1:5]):
        assert [int(v) for v in text.split()] == want[k].tolist(), (case, k)
    # the frame base of an entry: on the epoch's first tick it names the participant's frame of that tick
    base = [int(v) for v in lines[5].split()]
    for e in range(len(want["epoch_tick"]) - 1):
        t0 = int(want["epoch_tick"][e])
        for i in range(int(want["epoch_entry"][e]), int(want["epoch_entry"][e + 1])):
            p = int(want["entry_participant"][i])
            k = int(np.flatnonzero(present_ticks(stays, p) == t0)[0])
            assert base[i] + t0 == spans[p][1] + k, (case, e, i)


def test_planner_program_refuses_under_sanitizers(plan_exe, tmp_path):
    spans = [(5, 0, 10), (6, 10, 7)]
    assert _run_plan(plan_exe, tmp_path, spans, [(0, 0, 0, 10), (1, 0, 2, 4), (1, 1, 6, 3)])[0] != "refused"
    for stays in ([(0, 0, 0, 10), (1, 0, 2, 5), (1, 1, 6, 2)], [(0, 0, 0, 10), (1, 0, 2, 4), (1, 1, 6, 2)],
                  [(1, 0, 2, 4), (1, 1, 6, 3), (0, 0, 0, 10)], [(0, 0, 0, 10), (1, 0, 2, 4), (2, 1, 6, 3)]):
        assert _run_plan(plan_exe, tmp_path, spans, stays)[0] == "refused", stays
