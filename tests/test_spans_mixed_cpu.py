"""CPU: what the span calls with per-frame bitrates rest on (include/lyra_hip_spans_mixed.h; DESIGN.md 4.5 "Per-frame bitrates").

1. The new header, the second ctypes table of lyra_amd/codec.py (_SIGNATURES_SPANS_MIXED) and the built library agree on the five
   symbols; a null context is refused; include/lyra_hip.h and _SIGNATURES keep their counts.
2. The mixed planner (lyra_hip_spans_lossy_plan_mixed) against the uniform one: the loss state machine sees only whether a packet
   came, so for sizes drawn from {0, 8, 15, 23} every list equals lyra_hip_spans_lossy_plan's on where(pb > 0, 23, 0), and
   gen_bytes holds the sizes of the ticks fed from a packet.  Sizes that no bitrate has are refused on span frames only.
3. The planner header alone in a stand-alone program under -fsanitize=address,undefined over the same kind of inputs.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from lyra_amd import codec

from abi_loading import _protos, load_library
from signals import _gilbert_ticks as _gilbert

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = {"lyra_hip_encode_spans_mixed_dev": 12, "lyra_hip_encode_spans_mixed": 11, "lyra_hip_decode_spans_lossy_mixed_dev": 12,
       "lyra_hip_decode_spans_lossy_mixed": 12, "lyra_hip_spans_lossy_plan_mixed": 18}
MAX_STREAMS = 96
WORDS = [cp | (fade << 8) | (d << 16) for cp in range(5) for fade in range(3) for d in range(2)]
SIZES = np.array([8, 15, 23], np.int32)
LISTS = ("gen_frames", "rx_frames", "cng_frames", "cng_versions", "versions", "info", "chunks")


@pytest.fixture(scope="module")
def lib():
    return load_library()


def test_header_second_table_and_library_agree_on_the_five_symbols(lib):
    protos = _protos("lyra_hip_spans_mixed.h")
    assert set(protos) == set(NEW) == set(codec._SIGNATURES_SPANS_MIXED)
    for name, n_args in NEW.items():
        args = [a.strip() for a in protos[name].split(",")]
        assert len(args) == n_args, (name, args)
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name} is not exported by {codec.library_path()}"
        restype, argtypes = codec._SIGNATURES_SPANS_MIXED[name]
        assert restype is codec.C.c_int and fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert len(argtypes) == n_args, (name, argtypes)
        for a, t in zip(args, argtypes):   # pointers as void pointers, everything else an int
            assert ("*" in a) == (t is codec.C.c_void_p), (name, a, t)
    # a null context is refused, not dereferenced
    assert lib.lyra_hip_encode_spans_mixed_dev(None, None, 0, None, 0, None, 16000, None, None, 0, None, None) < 0
    assert lib.lyra_hip_encode_spans_mixed(None, None, 0, None, 0, None, 16000, None, 0, None, None) < 0
    assert lib.lyra_hip_decode_spans_lossy_mixed_dev(None, None, 0, None, 0, None, None, 16000, None, None, None, None) < 0
    assert lib.lyra_hip_decode_spans_lossy_mixed(None, None, 0, None, 0, None, None, 16000, None, None, None, None) < 0
    for name in ("encode_spans_mixed", "encode_spans_mixed_dev", "decode_spans_lossy_mixed", "decode_spans_lossy_mixed_dev",
                 "spans_lossy_plan_mixed"):
        assert hasattr(codec.LyraHip, name), name
    # the first header and the first table are what they were, and the new header is not pulled into the old one
    old = open(os.path.join(ROOT, "include", "lyra_hip.h")).read()
    assert "#include \"lyra_hip_spans_mixed.h\"" not in old
    old = re.sub(r"^[ \t]*#[^\n]*", "", re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", old, flags=re.S)), flags=re.M)
    all_protos = {name for _, name, _ in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(lyra_hip_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", old)}
    assert len(all_protos) == 98, len(all_protos)   # (the parse of tests/test_abi_cpu.py)
    assert len(codec._SIGNATURES) == 88
    assert not set(NEW) & set(codec._SIGNATURES)


def _same_as_uniform(spans, pb, ctl_in, lanes):
    """plan_mixed(pb) against plan(where(pb > 0, 23, 0), 23); returns the mixed plan"""
    got = codec.spans_lossy_plan_mixed(spans, pb, ctl_in, lanes, MAX_STREAMS)
    want = codec.spans_lossy_plan(spans, np.where(pb > 0, 23, 0), 23, ctl_in, lanes, MAX_STREAMS)
    where = (spans, [hex(c) for c in ctl_in])
    assert np.array_equal(got["counts"], want["counts"]), where   # n_gen, n_received, n_cng, n_versions, ctl_out
    for key in LISTS:
        assert np.array_equal(got[key], want[key]), (key, where)
    assert got["n_steps"] == want["n_steps"], where
    assert "gen_received" not in got and got["gen_bytes"].shape == want["gen_received"].shape, where
    fed = want["gen_received"] == 1
    assert np.array_equal(got["gen_bytes"][fed], pb[got["gen_frames"][fed]]), where
    assert not got["gen_bytes"][~fed].any(), where
    return got


def test_mixed_planner_equals_the_uniform_one_from_every_control_word(lib):
    rng = np.random.default_rng(21)
    seen = set()
    for ctl in WORDS:
        for n in (0, 1, 2, 7, 40):
            for kind in ("lost", "received", "random"):
                rx = np.zeros(n, bool) if kind == "lost" else np.ones(n, bool) if kind == "received" else _gilbert(rng, n)
                pb = np.concatenate([[23, 8, 15], np.where(rx, rng.choice(SIZES, n), 0), [0, 0]]).astype(np.int32)
                got = _same_as_uniform([(5, 3, n)], pb, [ctl], [])
                seen |= set(got["gen_bytes"].tolist())
    assert seen == {0, 8, 15, 23}


def test_mixed_planner_on_several_spans_with_lanes(lib):
    """lengths 350, W + 18, 26, 7, 1 and 0 in one buffer, 40 lanes: the long span's run_gen list is cut into lane chunks"""
    rng = np.random.default_rng(22)
    W = codec.span_warmup_frames("decoder", lib)
    lanes = np.arange(24, 64, dtype=np.int32)
    for trial in range(6):
        spans, parts, at = [], [], 0
        for sid, n in ((7, 350), (5, W + 18), (11, 26), (20, 7), (9, 1), (3, 0)):
            gap = int(rng.integers(0, 4))
            rx = np.zeros(n, bool) if (trial, sid) == (1, 11) else np.ones(n, bool) if (trial, sid) == (2, 11) else _gilbert(rng, n)
            parts += [np.full(gap, 85, np.int32), np.where(rx, rng.choice(SIZES, n), 0).astype(np.int32)]   # filler: no size at all
            spans.append((sid, at + gap, n))
            at += gap + n
        ctl_in = [int(rng.choice(WORDS)) for _ in spans]
        got = _same_as_uniform(spans, np.concatenate(parts), ctl_in, lanes)
        assert any(c["n_warmup"] > 0 for c in got["chunks"]), "no lane chunk"
        assert len(set(got["gen_bytes"].tolist())) == 4


def test_mixed_planner_refusals(lib):
    ok = dict(spans=[(0, 2, 10)], pb=np.tile(SIZES, 5)[:14].copy(), ctl=[0], lanes=[1, 2])
    codec.spans_lossy_plan_mixed(ok["spans"], ok["pb"], ok["ctl"], ok["lanes"], MAX_STREAMS)
    for size in (1, 7, 16, 24, -8):
        inside, outside = ok["pb"].copy(), ok["pb"].copy()
        inside[6] = size
        outside[[0, 1, 12, 13]] = size
        with pytest.raises(codec.LyraHipError):
            codec.spans_lossy_plan_mixed(ok["spans"], inside, ok["ctl"], ok["lanes"], MAX_STREAMS)
        _same_as_uniform(ok["spans"], outside, ok["ctl"], ok["lanes"])
    for case in (dict(spans=[(0, 0, 10), (3, 5, 2)], ctl=[0, 0]), dict(spans=[(MAX_STREAMS, 0, 10)]), dict(lanes=[0]),
                 dict(lanes=[1, 1])):
        a = {**ok, **case}
        with pytest.raises(codec.LyraHipError):
            codec.spans_lossy_plan_mixed(a["spans"], a["pb"], a["ctl"], a["lanes"], MAX_STREAMS)


_SANITIZED = r'''
#include <cstdio>
#include <cstdlib>
#include <random>
#include "spans_lossy_plan.h"
// plan_mixed against plan on the same receive pattern, from every control word: random, all-lost, all-received, empty and
// one-frame spans inside a buffer whose other frames hold sizes that no bitrate has.  Any difference: exit 1.
using namespace lyra;
static int fail(const char* what, int a, int b) { std::printf("%s (%d, %d)\n", what, a, b); return 1; }
int main() {
  std::mt19937 rng(5);
  const int sizes[3] = {8, 15, 23};
  long ticks = 0;
  for (unsigned cp = 0; cp < 5; ++cp) for (unsigned fade = 0; fade < 3; ++fade) for (unsigned d = 0; d < 2; ++d)
    for (int kind = 0; kind < 3; ++kind) for (int n : {0, 1, 2, 7, 40, 350}) {
      const uint32_t ctl[2] = {cp | (fade << 8) | (d << 16), 0u};
      const sp::Span spans[2] = {{5, 3, n}, {9, 3 + n + 2, n / 2}};
      const int frames = 3 + n + 2 + n / 2 + 1;
      std::vector<int32_t> pb((size_t)frames, 16), uni((size_t)frames, 16);
      for (const sp::Span& s : spans)
        for (int64_t f = s.first_frame; f < s.first_frame + s.n_frames; ++f) {
          const bool rx = kind == 0 ? false : kind == 1 ? true : rng() % 3 != 0;
          pb[(size_t)f] = rx ? sizes[rng() % 3] : 0;
          uni[(size_t)f] = rx ? 23 : 0;
        }
      std::vector<slp::SpanLists> got, want;
      if (slp::plan_mixed(spans, 2, pb.data(), ctl, &got) != 0 || slp::plan(spans, 2, uni.data(), 23, ctl, &want) != 0)
        return fail("a plan was refused", n, kind);
      for (int s = 0; s < 2; ++s) {
        const slp::SpanLists &G = got[(size_t)s], &U = want[(size_t)s];
        if (G.gen_frame != U.gen_frame || G.rx_frame != U.rx_frame || G.cng_frame != U.cng_frame ||
            G.cng_version != U.cng_version || G.versions != U.versions || G.info != U.info || G.ctl_out != U.ctl_out)
          return fail("a list differs", n, kind);
        if (G.gen_received.size() != U.gen_received.size()) return fail("gen_bytes: size", n, kind);
        for (size_t i = 0; i < G.gen_frame.size(); ++i, ++ticks)
          if ((int)G.gen_received[i] != (U.gen_received[i] ? pb[(size_t)G.gen_frame[i]] : 0)) return fail("gen_bytes", n, (int)i);
      }
      const std::vector<sp::Span> a = slp::compact_gen_spans(spans, got), b = slp::compact_gen_spans(spans, want);
      for (int s = 0; s < 2; ++s)
        if (a[(size_t)s].first_frame != b[(size_t)s].first_frame || a[(size_t)s].n_frames != b[(size_t)s].n_frames)
          return fail("compact spans", n, s);
      if (n) {   // a size of no bitrate on a span frame is refused, by both forms
        std::vector<int32_t> bad = pb;
        bad[3] = 16;
        if (slp::plan_mixed(spans, 2, bad.data(), ctl, &got) == 0) return fail("size 16 accepted", n, kind);
        bad[3] = -8;
        if (slp::plan_mixed(spans, 2, bad.data(), ctl, &got) == 0) return fail("size -8 accepted", n, kind);
        if (slp::plan(spans, 2, pb.data(), slp::SIZE_PER_FRAME, ctl, &got) == 0) return fail("plan took the mixed size", n, kind);
      }
    }
  std::printf("ok %ld ticks\n", ticks);
  return 0;
}
'''


def test_planner_header_under_address_and_ub_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler: the library's own build needs one"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = subprocess.run([cxx, *flags, "-x", "c++", "-", "-o", str(tmp_path / "probe")], input="int main(){return 0;}",
                           capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("no sanitizer runtimes for the host compiler here")
    (tmp_path / "plan.cc").write_text(_SANITIZED)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", *flags, "-I" + os.path.join(ROOT, "lyra_amd", "csrc"),
                           str(tmp_path / "plan.cc"), "-o", str(tmp_path / "plan")], timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([str(tmp_path / "plan")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.returncode, r.stdout[-500:], r.stderr[-2000:])
