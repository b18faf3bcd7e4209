"""The loudest-N bridge with shared encoders, the parts that need no GPU (include/lyra_hip_shared_bridge.h):
1. the header, the ctypes table of lyra_amd/codec.py (_SIGNATURES_SHARED, with a loader of its own) and the built library agree on
   the symbols, argument counts and types; the tick struct is SharedTick; a null context is refused; LyraHip has the methods; the
   three new kernels are in the library's gfx950 code object and use no scratch (the code object's metadata);
2. the numpy model of tests/shared_bridge_models.py: the slot rule on hand-made rows, and the scripted conference, which must
   show every slot event it was written for;
3. the planner-side check of room_labels (lyra_amd/csrc/shared_bridge_plan.h) as a program, and against the model's own;
4. the host logic of LyraSharedBridge: tests/shared_bridge/shared_class_test.cc, linked against a fake of the new calls
   (tests/shared_bridge/fake_shared_abi.cc) next to the unchanged fakes, built with -fsanitize=address,undefined and run as a
   program; the two other bridge classes reference nothing of the new calls."""
import os
import re
import subprocess

import numpy as np
import pytest

from lyra_amd import codec

from abi_loading import _protos, load_library
from bridge_models import np_bridge_plan
from shared_bridge_models import (EVENTS, SLOTS, check_labels, np_fanout, np_shared_mix, np_slot_update, run_slot_script,
                                  slot_script)
from speaker_models import np_speakers_mix

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HOST = os.path.join(ROOT, "lyra_amd", "host")
CSRC = os.path.join(ROOT, "lyra_amd", "csrc")
HERE = os.path.join(ROOT, "tests", "shared_bridge")
NEW = {"lyra_hip_shared_mix_dev": 18, "lyra_hip_shared_tick_dev": 2, "lyra_hip_shared_begin": 14, "lyra_hip_shared_end": 8,
       "lyra_hip_shared_reset_rooms": 3}
KERNELS = ("shared_slots_kernel", "shared_mix_kernel", "shared_fanout_kernel")
SAN = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")


@pytest.fixture(scope="module")
def lib():
    return load_library()


def _c_type(decl):
    """a pointer is a void pointer, `unsigned` is one, anything else an int"""
    decl = decl.strip()
    return codec.C.c_void_p if "*" in decl else codec.C.c_uint if decl.startswith("unsigned") else codec.C.c_int


def _stripped(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)


def _struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _stripped(header), flags=re.S).group(1)
    return [" ".join(f.split()) for f in body.split(";") if f.strip()]


# ---- 1. the ABI -------------------------------------------------------------------------------------------------------------

def test_header_table_and_library_agree_on_the_symbols(lib):
    protos = _protos("lyra_hip_shared_bridge.h")
    assert set(protos) == set(NEW) == set(codec._SIGNATURES_SHARED)
    for name, n_args in NEW.items():
        args = protos[name].split(",")
        assert len(args) == n_args, (name, args)
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name} is not exported by {codec.library_path()}"
        restype, argtypes = codec._SIGNATURES_SHARED[name]
        assert restype is codec.C.c_int and fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert [_c_type(a) for a in args] == list(argtypes), (name, args)
    tables = (codec._SIGNATURES, codec._SIGNATURES_BRIDGE, codec._SIGNATURES_SPEAKERS, codec._SIGNATURES_ENCODE_STREAMS,
              codec._SIGNATURES_DECODE_STREAMS)
    assert not any(set(codec._SIGNATURES_SHARED) & set(t) for t in tables)
    assert "lyra_hip_shared_bridge.h" in open(os.path.join(ROOT, "include", "lyra_hip.h")).read()


def test_the_tick_struct_is_the_headers():
    fields = _struct_fields("lyra_hip_shared_bridge.h", "lyra_hip_shared_tick")
    assert [re.split(r"[\s*]+", f)[-1] for f in fields] == [n for n, _ in codec.SharedTick._fields_]
    for f, (name, t) in zip(fields, codec.SharedTick._fields_):
        assert t is _c_type(f), (f, t)
    # the loudest-N tick's fields without the per-listener bit counts, DTX flags and mix, in its order; then the new ones
    old = [f for f in _struct_fields("lyra_hip_speakers.h", "lyra_hip_speakers_tick")
           if re.split(r"[\s*]+", f)[-1] not in ("d_num_bits", "d_dtx", "d_mix")]
    assert fields[:len(old)] == old and len(fields) == len(old) + 10
    hdr = _stripped("lyra_hip_shared_bridge.h")
    assert codec.SHARED_SLOTS == SLOTS == int(re.search(r"#define LYRA_HIP_SHARED_SLOTS (\d+)", hdr).group(1)) == codec.SPEAKERS_MAX


def test_a_null_context_is_refused(lib):
    for name in NEW:
        args = [None if t is codec.C.c_void_p else 0 for t in codec._SIGNATURES_SHARED[name][1]]
        assert getattr(lib, name)(*args) < 0, name


def test_lyrahip_has_the_methods():
    for name in ("shared_mix_dev", "shared_tick_dev", "shared_begin", "shared_end", "shared_reset_rooms"):
        assert callable(getattr(codec.LyraHip, name, None)), name


def test_the_kernels_are_in_the_gfx950_code_object_and_use_no_scratch():
    """A kernel descriptor symbol (<mangled name>.kd) exists only in a device code object.  Registers and scratch are read from
    the amdhsa.kernels notes of the kernels' final ISA (the same build flags as the library's), not from its instructions."""
    image = open(codec.library_path(), "rb").read()
    assert set(re.findall(rb"hip[v\d]*-amdgcn-amd-amdhsa--(gfx\w+)", image)) == {b"gfx950"}
    for kernel in KERNELS:
        assert re.search(rb"_ZN4lyra\d+" + kernel.encode() + rb"E\w*\.kd", image), kernel
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not present")
    r = subprocess.run(["make", "-C", CSRC, "-j4", "ODIR=obj_asm", "obj_asm/shared_bridge_kernels.s", "obj_asm/speakers_kernels.s"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    notes = {}
    for f in ("shared_bridge_kernels.s", "speakers_kernels.s"):
        for block in open(os.path.join(CSRC, "obj_asm", f)).read().split("\n  - .agpr_count:")[1:]:
            block = block.split("amdhsa.target")[0]
            name = re.search(r"\.name:\s+_ZN4lyra\d+([a-z0-9_]+_kernel)E", block).group(1)
            notes[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
                           for k in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    for kernel in KERNELS + ("speakers_level_kernel", "speakers_select_kernel", "speakers_mix_kernel"):
        assert notes[kernel]["private_segment_fixed_size"] == 0 and notes[kernel]["group_segment_fixed_size"] == 0, (kernel, notes[kernel])
        assert notes[kernel]["vgpr_count"] <= 128, (kernel, notes[kernel])   # (at least four waves per SIMD)


# ---- 2. the model -----------------------------------------------------------------------------------------------------------

def test_the_slot_rule_on_hand_made_rows():
    free = [-1] * SLOTS
    assert np_slot_update(free, [30, 10, 20], 3) == [30, 10, 20, -1, -1, -1, -1, -1]           # selection order into free slots
    assert np_slot_update([30, 10, 20] + free[3:], [20, 30, 10], 3)[:3] == [30, 10, 20]         # the ranks change, the slots stay
    assert np_slot_update([30, 10, 20] + free[3:], [20, 40, 30], 3)[:3] == [30, 40, 20]         # 10 left: 40 takes its slot
    assert np_slot_update([30, 10, 20] + free[3:], [50, 40, 10], 3)[:3] == [50, 10, 40]         # two newcomers: the louder one lower
    assert np_slot_update([30, 10, 20] + free[3:], [20], 3)[:3] == [-1, -1, 20]                 # fewer speakers than N
    assert np_slot_update([30, 10, 20, 70, 80] + free[5:], [20, 30], 2) == [30, 20] + free[2:]  # N shrank: 20 moves below N
    assert np_slot_update([30, 30, 20] + free[3:], [30, 20, 10], 3)[:3] == [30, 10, 20]         # an id twice: the lower slot wins
    assert np_slot_update([30, 10] + free[2:], [], 3) == free


def test_the_scripted_conference_shows_every_slot_event():
    ticks, ids, keys, n_table = slot_script()
    out, seen = run_slot_script(ticks, ids, keys, n_table, fill=12345)
    assert len(ticks) >= 40
    for event in EVENTS:
        assert seen[event] >= 1, (event, seen)
    others = np.setdiff1d(np.arange(n_table), keys)
    assert all((rec["after"][others] == 12345).all() for rec in out), "a table row that belongs to no room changed"
    for rec in out:      # a speaker holds exactly one slot, everybody else none; a slot's mix leaves out exactly its holder
        N, x = rec["N"], rec["tick"]["x"].astype(np.int64)
        assert np.array_equal(rec["slot_of"] >= 0, rec["is_speaker"] == 1)
        for r, q in enumerate(keys):
            row = rec["after"][q]
            held = [int(v) for v in row if v >= 0]
            assert sorted(held) == sorted(rec["speakers"][r]) and (row[N:] == -1).all()
            total = x[[int(np.flatnonzero(ids == v)[0]) for v in held]].sum(axis=0) if held else np.zeros(320, np.int64)
            for j in range(N):
                own = x[int(np.flatnonzero(ids == row[j])[0])] if row[j] >= 0 else 0
                assert np.array_equal(rec["enc_mix"][r * (1 + N) + 1 + j], np.clip(total - own, -32768, 32767))
            assert np.array_equal(rec["enc_mix"][r * (1 + N)], np.clip(total, -32768, 32767))


def test_the_fan_out_of_the_encoder_mixes_is_the_loudest_n_mix():
    """What listener b would receive, were the "packets" the encoder mixes themselves, is row b of the loudest-N mix."""
    ticks, ids, keys, n_table = slot_script()
    out, _ = run_slot_script(ticks, ids, keys, n_table)
    for rec in out[::4]:
        N, B = rec["N"], ids.size
        E = rec["enc_mix"].shape[0]
        heard = np.zeros((B, 320), np.int16)
        for r in range(len(rec["start"]) - 1):
            for b in rec["order"][rec["start"][r]:rec["start"][r + 1]]:
                heard[b] = rec["enc_mix"][r * (1 + N) + (1 + rec["slot_of"][b] if rec["slot_of"][b] >= 0 else 0)]
        assert np.array_equal(heard, np_speakers_mix(rec["tick"]["x"], rec["order"], rec["start"], N)[0])
        pk = (np.arange(E * 23) % 251).astype(np.uint8).reshape(E, 23)
        sizes = np.where(np.arange(E) % 3 == 0, 0, 23).astype(np.int32)
        got, got_n = np_fanout(pk, sizes, B, rec["order"], rec["start"], rec["slot_of"], N, keys, n_table)
        rooms = rec["tick"]["rooms"]
        assert not got[rooms < 0].any() and not got_n[rooms < 0].any()
        for b in np.flatnonzero(rooms >= 0):
            e = int(rooms[b]) * (1 + N) + (1 + rec["slot_of"][b] if rec["slot_of"][b] >= 0 else 0)
            assert np.array_equal(got[b], pk[e]) and got_n[b] == sizes[e]
        bad = np_fanout(pk, sizes, B, rec["order"], rec["start"], rec["slot_of"], N, np.array([n_table, keys[1]]), n_table)
        assert not bad[0][rooms == 0].any() and not bad[1][rooms == 0].any() and np.array_equal(bad[0][rooms == 1], got[rooms == 1])


def test_a_bad_key_silences_its_room_only():
    ticks, ids, keys, n_table = slot_script()
    x, rooms = ticks[0]["x"], ticks[0]["rooms"]
    order, start = np_bridge_plan(rooms)
    table = np.full((n_table, SLOTS), -1, np.int32)
    good = np_shared_mix(x, ids, order, start, 3, table, keys)
    bad = np_shared_mix(x, ids, order, start, 3, table, np.array([keys[0], -1]))
    assert np.array_equal(bad[0][:4], good[0][:4]) and not bad[0][4:].any() and good[0][4:].any()
    assert np.array_equal(bad[1], good[1]) and np.array_equal(bad[2], good[2])          # levels and flags are the selection's
    assert (bad[3][rooms == 1] == -1).all() and np.array_equal(bad[3][rooms == 0], good[3][rooms == 0])
    assert np.array_equal(bad[4][keys[1]], table[keys[1]]) and np.array_equal(bad[4][keys[0]], good[4][keys[0]])


# ---- 3. the labels ----------------------------------------------------------------------------------------------------------

def test_the_planner_side_check_of_room_labels(tmp_path):
    exe = str(tmp_path / "shared_plan_test")
    subprocess.check_call(SAN + ["-I" + CSRC, "-o", exe, os.path.join(HERE, "shared_plan_test.cc")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=SAN_ENV)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    rooms = np.array([7, -1, 2, 7, 40, 2, -5, 7], np.int32)       # (the program's case, held to the model's check)
    assert check_labels(rooms, [2, 7, 40], 41) and not check_labels(rooms, [2, 7, 40], 40)
    for wrong in ([2, 7], [2, 7, 40, 41], [7, 2, 40], [2, 2, 40], [2, 8, 40], [-2, 7, 40]):
        assert not check_labels(rooms, wrong, 64), wrong


# ---- 4. the class -----------------------------------------------------------------------------------------------------------

def test_shared_bridge_host_logic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "shared_class_test")
    subprocess.check_call(SAN + ["-I" + HOST, "-I" + os.path.join(HOST, "shims"), "-I" + ROOT, "-I" + HERE,
                                 "-I" + os.path.join(ROOT, "tests", "bridge"), "-o", exe,
                                 os.path.join(HERE, "shared_class_test.cc"), os.path.join(HERE, "fake_shared_abi.cc"),
                                 os.path.join(ROOT, "tests", "bridge", "fake_bridge_abi.cc"),
                                 os.path.join(HOST, "lyra_shared_bridge.cc"), os.path.join(HOST, "lyra_conference_bridge.cc"),
                                 os.path.join(ROOT, "tests", "host_stub", "fake_lyra_hip_codec.cc")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=SAN_ENV)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_the_other_bridge_classes_reference_nothing_of_the_new_calls(tmp_path):
    syms = {}
    for name in ("lyra_conference_bridge", "lyra_speaker_bridge", "lyra_shared_bridge"):
        obj = str(tmp_path / (name + ".o"))
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + HOST, "-I" + os.path.join(HOST, "shims"), "-I" + ROOT, "-c",
                               os.path.join(HOST, name + ".cc"), "-o", obj], timeout=600)
        syms[name] = subprocess.check_output(["nm", "-C", "--undefined-only", obj], text=True)
    for old in ("lyra_conference_bridge", "lyra_speaker_bridge"):
        assert "lyra_hip_shared" not in syms[old] and "LyraSharedBridge" not in syms[old], old
        for text in (open(os.path.join(HOST, old + ".cc")).read(), open(os.path.join(HOST, old + ".h")).read()):
            assert "lyra_hip_shared" not in text and "lyra_hip_shared_bridge.h" not in text
    new = syms["lyra_shared_bridge"]
    assert all(f"lyra_hip_shared_{call}" in new for call in ("begin", "end", "reset_rooms"))
    assert "lyra_hip_bridge_begin" not in new and "lyra_hip_speakers" not in new and "encode_streams" not in new
