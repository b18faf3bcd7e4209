"""CPU: what lyra_hip_decode_spans_lossy rests on (include/lyra_hip.h "Time-parallel spans", packet loss).

1. The header, the ctypes prototypes of lyra_amd/codec.py and the built library agree on the three new symbols; a null context
   and everything the planner refuses give a negative code.
2. The planner (lyra_amd/csrc/spans_lossy_plan.h through lyra_hip_spans_lossy_plan) against a brute-force loop over lossy_tick
   (lyra_amd/csrc/lossy_plan.h, compiled here with a plain C++ compiler into a transition table): from every control word the
   state machine can hold (cp 0..4, fade 0..2, both directions) and over random receive patterns, all lost, all received, empty
   and one-frame spans -- the three frame lists, the estimate versions and their deduplicated set, the info words, the final
   control word, and the chunk plan = lyra_hip_spans_plan on the run_gen counts.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from lyra_amd import codec

from abi_loading import load_library
from signals import _gilbert_ticks as _gilbert

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = {"lyra_hip_decode_spans_lossy_dev": 13, "lyra_hip_decode_spans_lossy": 13, "lyra_hip_spans_lossy_plan": 19}
MAX_STREAMS = 96
WORDS = [cp | (fade << 8) | (d << 16) for cp in range(5) for fade in range(3) for d in range(2)]

_TABLE = r'''
#include <cstdio>
#include "lossy_plan.h"
// per (control word, received): ctl_out info run_gen run_cng feed_est
int main() {
  for (unsigned cp = 0; cp < 5; ++cp) for (unsigned fade = 0; fade < 3; ++fade) for (unsigned d = 0; d < 2; ++d)
    for (int rx = 0; rx < 2; ++rx) {
      const unsigned ctl = cp | (fade << 8) | (d << 16);
      const lyra::LossyTick t = lyra::lossy_tick(ctl, rx != 0);
      std::printf("%u %d %u %d %d %d %d\n", ctl, rx, t.ctl, (int)lyra::lossy_info(t), t.run_gen, t.run_cng, t.feed_est);
    }
  return 0;
}
'''


@pytest.fixture(scope="module")
def lib():
    return load_library()


@pytest.fixture(scope="module")
def tick(tmp_path_factory):
    """(ctl, received) -> (ctl_out, info, run_gen, run_cng, feed_est), from lossy_tick itself"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler: the library's own build needs one"
    d = tmp_path_factory.mktemp("lossy_table")
    (d / "table.cc").write_text(_TABLE)
    subprocess.check_call([cxx, "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "lyra_amd", "csrc"), str(d / "table.cc"),
                           "-o", str(d / "table")], timeout=120)
    rows = [[int(v) for v in l.split()] for l in subprocess.check_output([str(d / "table")], text=True, timeout=60).splitlines()]
    table = {(r[0], r[1]): tuple(r[2:]) for r in rows}
    assert len(table) == 60
    assert all(out[0] in WORDS for out in table.values()), "lossy_tick leaves the 30 words"
    return table


def test_header_ctypes_and_library_agree_on_the_new_symbols(lib):
    hdr = open(os.path.join(ROOT, "include", "lyra_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    protos = {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(lyra_hip_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)}
    for name, n_args in NEW.items():
        assert name in protos, f"{name} is not declared in include/lyra_hip.h"
        args = [a.strip() for a in protos[name].split(",")]
        assert len(args) == n_args, (name, args)
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name} is not exported by {codec.library_path()}"
        assert fn.argtypes is not None and len(fn.argtypes) == n_args, (name, fn.argtypes)
        for a, t in zip(args, fn.argtypes):   # pointers as void pointers, everything else an int
            assert ("*" in a) == (t is codec.C.c_void_p), (name, a, t)
    # a null context is refused, not dereferenced
    assert lib.lyra_hip_decode_spans_lossy_dev(None, None, 0, None, 0, None, None, 64, 16000, None, None, None, None) < 0
    assert lib.lyra_hip_decode_spans_lossy(None, None, 0, None, 0, None, None, 64, 16000, None, None, None, None) < 0
    assert hasattr(codec.LyraHip, "decode_spans_lossy") and hasattr(codec.LyraHip, "decode_spans_lossy_dev")


def _brute(tick, ctl, first, rx):
    """one span by the loop the hop-by-hop call runs"""
    out = dict(gen=[], gen_rx=[], rx=[], cng=[], ver=[], info=[])
    received = 0
    for k, r in enumerate(rx):
        ctl, info, run_gen, run_cng, feed = tick[(ctl, int(r))]
        if run_cng:   # reads the estimate in front of this tick's update
            out["cng"].append(first + k); out["ver"].append(received)
        if run_gen:
            out["gen"].append(first + k); out["gen_rx"].append(int(r))
        if feed:
            out["rx"].append(first + k); received += 1
        out["info"].append(info)
    out["ctl"] = ctl
    out["versions"] = sorted(set(out["ver"]))
    return out


def _check(tick, spans, rx_all, ctl_in, lanes, nbytes=15):
    pb = np.where(rx_all, nbytes, 0).astype(np.int32)
    got = codec.spans_lossy_plan(spans, pb, nbytes, ctl_in, lanes, MAX_STREAMS)
    at = dict(gen=0, rx=0, cng=0, ver=0, info=0)
    compact = []
    for s, (sid, first, n) in enumerate(spans):
        want = _brute(tick, ctl_in[s], first, rx_all[first:first + n])
        c = got["counts"][s]
        where = (s, sid, first, n, hex(ctl_in[s]))
        assert (c["n_gen"], c["n_received"], c["n_cng"], c["n_versions"], c["ctl_out"]) == \
               (len(want["gen"]), len(want["rx"]), len(want["cng"]), len(want["versions"]), want["ctl"]), where
        cut = lambda key, a, k: list(got[key][at[a]:at[a] + k])
        assert cut("gen_frames", "gen", len(want["gen"])) == want["gen"], where
        assert cut("gen_received", "gen", len(want["gen"])) == want["gen_rx"], where
        assert cut("rx_frames", "rx", len(want["rx"])) == want["rx"], where
        assert cut("cng_frames", "cng", len(want["cng"])) == want["cng"], where
        assert cut("cng_versions", "cng", len(want["cng"])) == want["ver"], where
        assert cut("versions", "ver", len(want["versions"])) == want["versions"], where
        assert cut("info", "info", n) == want["info"], where
        compact.append((sid, at["gen"], len(want["gen"])))
        at["gen"] += len(want["gen"]); at["rx"] += len(want["rx"]); at["cng"] += len(want["cng"])
        at["ver"] += len(want["versions"]); at["info"] += n
    for key, a in (("gen_frames", "gen"), ("rx_frames", "rx"), ("cng_frames", "cng"), ("versions", "ver"), ("info", "info")):
        assert len(got[key]) == at[a], key
    chunks, steps = codec.spans_plan("decoder", compact, lanes, MAX_STREAMS)
    assert np.array_equal(got["chunks"], chunks) and got["n_steps"] == steps
    return got


def test_planner_equals_the_loop_over_lossy_tick_from_every_control_word(lib, tick):
    rng = np.random.default_rng(11)
    for ctl in WORDS:
        for n in (0, 1, 2, 7, 40):
            for kind in ("lost", "received", "random"):
                rx = np.zeros(n, bool) if kind == "lost" else np.ones(n, bool) if kind == "received" else _gilbert(rng, n)
                buf = np.concatenate([np.ones(3, bool), rx, np.zeros(2, bool)])
                _check(tick, [(5, 3, n)], buf, [ctl], [])


def test_planner_on_several_spans_with_lanes(lib, tick):
    """lengths 350, 43, 26, 7, 1 and 0 in one buffer, 40 lanes: the long span's run_gen list is cut into lane chunks"""
    rng = np.random.default_rng(12)
    W = codec.span_warmup_frames("decoder", lib)
    lanes = np.arange(24, 64, dtype=np.int32)
    for trial in range(6):
        spans, parts, at = [], [], 0
        for sid, n in ((7, 350), (5, W + 18), (11, 26), (20, 7), (9, 1), (3, 0)):
            gap = int(rng.integers(0, 4))
            parts += [np.ones(gap, bool), _gilbert(rng, n)]
            spans.append((sid, at + gap, n))
            at += gap + n
        ctl_in = [int(rng.choice(WORDS)) for _ in spans]
        got = _check(tick, spans, np.concatenate(parts), ctl_in, lanes)
        assert any(c["n_warmup"] > 0 for c in got["chunks"]), "no lane chunk"
    # a span whose every tick is pure comfort noise runs no chunk
    got = _check(tick, [(1, 0, 30)], np.zeros(30, bool), [4 | (2 << 8) | (1 << 16)], lanes)
    assert len(got["chunks"]) == 0 and got["counts"][0]["n_gen"] == 0 and got["counts"][0]["n_cng"] == 30
    assert list(got["versions"]) == [0]


def test_planner_refusals(lib):
    ok = dict(spans=[(0, 0, 10)], pb=np.full(12, 8, np.int32), nbytes=8, ctl=[0], lanes=[1, 2])
    codec.spans_lossy_plan(ok["spans"], ok["pb"], ok["nbytes"], ok["ctl"], ok["lanes"], MAX_STREAMS)
    bad_size = ok["pb"].copy(); bad_size[4] = 15
    cases = [dict(pb=bad_size), dict(pb=-ok["pb"]), dict(nbytes=0), dict(spans=[(0, 0, 10), (3, 5, 2)], ctl=[0, 0]),
             dict(spans=[(MAX_STREAMS, 0, 10)]), dict(lanes=[0]), dict(lanes=[1, 1])]
    for case in cases:
        a = {**ok, **case}
        with pytest.raises(codec.LyraHipError):
            codec.spans_lossy_plan(a["spans"], a["pb"], a["nbytes"], a["ctl"], a["lanes"], MAX_STREAMS)
