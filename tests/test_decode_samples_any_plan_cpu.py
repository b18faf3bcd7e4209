"""CPU: the planning of lyra_hip_decode_samples_any_dev -- BufferedResampler's leftover on integers
(lyra_amd/csrc/decode_samples_any_plan.h) in front of ds_plan run in rounds of at most one hop -- compiled with a plain C++
compiler, WITH -fsanitize=address,undefined, and driven as a program of its own against oracle/lyra_codec_model.py's
RefLyraDecoder on tests/host_stub/fake_kit.py's counting components.  After every call: the six integers the model has
(concealment / fade progress, fade direction, the read positions in both hops, the waiting vectors) and the leftover count;
the generative hops, comfort-noise hops and estimator calls over all rounds; is_comfort_noise(); and, sample by sample,
where every internal sample comes from (which hop, which offset, which cross-fade index): a round boundary may cut one pass of
the reference loop in two, so passes are not compared one to one.  What the kernels rely on is asserted on the MODEL's
trajectory: the leftover never exceeds 2 / 1 / 0 / 0 samples at 48 / 32 / 16 / 8 kHz, n_int never exceeds 1280, a chunk of at
most 320 samples is cut by at most 2 passes.

Also here: the integer n_int against the reference's float expression, exhaustively; the size rule; the new verdict of
sb::validate; the ctypes table against include/lyra_hip_decode_samples_any.h."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from signals import _gilbert_ticks

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEPTH = 4
HOP = 320
RATES = [48000, 32000, 16000, 8000]
LEFT_MAX = {48000: 2, 32000: 1, 16000: 0, 8000: 0}

_DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "decode_samples_any_plan.h"
// plan <rate>: one script per input line, tokens "<packet 0/1>:<n external samples>" per call.
// nint <rate>: used, n_int, left for every n of 0 .. 4 hops and every leftover count 0 .. 2.
int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const int rate = std::atoi(argv[2]);
  if (!std::strcmp(argv[1], "nint")) {
    for (int n = 0; n <= 4 * (rate / 50); ++n)
      for (int L = 0; L <= lyra::DSA_LEFT_MAX; ++L) {
        const lyra::DsaStep s = lyra::ds_any_step(L, n, rate);
        std::printf("%d %d %d %d %d %d\n", n, L, s.used, s.n_int, s.left, lyra::ds_any_rounds(n, rate));
      }
    return 0;
  }
  if (!std::strcmp(argv[1], "valid")) {
    for (int i = 3; i < argc; ++i) std::printf("%d\n", lyra::ds_any_valid(std::atoi(argv[i]), rate) ? 1 : 0);
    return 0;
  }
  static char line[1 << 20];
  std::printf("depth %d max_internal %d left_max %d\n", lyra::DS_FIFO_DEPTH, lyra::DSA_MAX_INTERNAL, lyra::DSA_LEFT_MAX);
  while (std::fgets(line, sizeof line, stdin)) {
    lyra::DsState s;
    std::memset(&s, 0, sizeof s);   // all zero = the reference's initial state
    int left = 0;
    long gen_hops = 0, cng_hops = 0;
    for (char* tok = std::strtok(line, " \n"); tok; tok = std::strtok(nullptr, " \n")) {
      int pk = 0, n = 0;
      if (std::sscanf(tok, "%d:%d", &pk, &n) != 2) return 2;
      if (!lyra::ds_any_valid(n, rate)) { std::printf("einval\n"); continue; }
      const lyra::DsaStep st = lyra::ds_any_step(left, n, rate);
      left = st.left;
      const int R = lyra::ds_any_rounds(n, rate);
      int g = 0, c = 0, e = 0, dropped = 0, bad = 0, nseg = 0, cn = 0, done = 0;
      char segs[8192];
      int at = 0;
      for (int r = 0; r < (R > 0 ? R : 1); ++r) {
        const int total = lyra::ds_any_round_total(st.n_int, r);
        const lyra::DsPlan p = lyra::ds_plan(s, pk != 0 && r == 0, total);
        s = p.s;
        g += p.gen_start >= 0; c += p.cng_start >= 0; e += p.est_seg >= 0; dropped += p.dropped; bad += p.bad;
        cn = p.comfort_noise;
        for (int k = 0; k < p.nseg; ++k) {
          const lyra::DsSeg& q = p.seg[k];
          if (q.gen_n && q.gen_off == 0) gen_hops++;
          if (q.cng_n && q.cng_off == 0) cng_hops++;
          at += std::snprintf(segs + at, sizeof segs - at, " %d %d %d %d %d %d %ld %ld", q.gen_n, q.cng_n, q.gen_off, q.cng_off,
                              q.fade, q.dir, gen_hops - 1, cng_hops - 1);
          done += q.n;
          nseg++;
        }
      }
      if (done != st.n_int || st.n_int > R * 320) bad++;   // every internal sample is planned in the call's own rounds
      std::printf("%d %d %d %d %d %d %d  %d %d %d  %d %d %d  %d %d %d %d%s\n", s.cp, s.fade, s.to_cng ? 1 : -1, s.gpos, s.cpos, s.wait,
                  left, g, c, e, cn, dropped, bad, st.used, st.n_int, R, nseg, at ? segs : "");
    }
    std::printf("end\n");
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("plan_any")
    src, exe = d / "plan_any.cc", d / "plan_any"
    src.write_text(_DRIVER)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "lyra_amd", "csrc"), str(src),
                           "-o", str(exe)], timeout=300)
    return str(exe)


def _run(driver, args, text=""):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([driver] + [str(a) for a in args], input=text, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-4000:])
    return r.stdout


def _sizes(rate):
    hop = rate // 50
    # (1024 frames at 8 kHz are 6.4 hops: above the call's four, refused -- test_request_size_rule)
    return [n for n in (128, 256, 441, 512, 1024, 1, 2, 0, hop, 2 * hop + 1, 4 * hop - 1, 4 * hop) if n <= 4 * hop]


def _session(rng, rate, got, draw):
    """A receiver that asks for draw() samples per call while the packet of every 20 ms arrives (got[t]) when its playout
    time comes: more than one packet due -> the earlier ones in n = 0 calls of their own, the last one with the request."""
    calls, played, sent = [], 0, 0
    while sent < len(got):
        n = draw()
        due = min(len(got), played * 50 // rate + 1)
        arrived = [t for t in range(sent, due) if got[t]]
        sent = due
        calls += [(True, 0)] * max(0, len(arrived) - 1)
        calls.append((bool(arrived), n))
        played += n
    return calls


def _scripts(rng, rate):
    sizes, hop = _sizes(rate), rate // 50
    out = []
    for i in range(24):          # the audio-callback sizes in random order under Gilbert loss
        got = _gilbert_ticks(rng, int(rng.integers(30, 90)), recover_from=0.1).tolist()
        out.append(("sizes gilbert", _session(rng, rate, got, lambda: int(rng.choice(sizes)))))
    for n in sizes:              # one size held for a whole session, every packet received and then long losses
        if n:
            got = [True] * 8 + [False] * 14 + [True] * 9 + [False] * 3 + [True] * 6
            out.append(("fixed %d" % n, _session(rng, rate, got, lambda n=n: n)))
    for _ in range(24):          # random sizes of 0 .. 4 hops
        got = _gilbert_ticks(rng, int(rng.integers(30, 90)), recover_from=0.1).tolist()
        top = int(rng.choice([7, hop, 4 * hop]))
        out.append(("random n", _session(rng, rate, got, lambda: int(rng.integers(0, top + 1)))))
    for late in (1, 2):          # a packet handed over `late` calls late, in a call of its own
        calls, owed = [], 0
        for t in range(120):
            due = t % 2 == 0 and not (30 <= t < 70 and (t // 2) % 3 == 0)
            if due and (t // 2) % 5 == 2:
                owed, due = late, False
            elif owed:
                owed -= 1
                if owed == 0:
                    calls.append((True, 0))
            calls.append((due, [128, 441, 1, hop // 2][t % 4] if t % 7 else hop // 2))
        out.append(("late %d" % late, calls))
    half = hop // 2
    out.append(("overflow", [(True, half), (False, half)] * 2 + [(True, 0)] * (DEPTH + 3) + [(False, 4 * hop - 1)] * 8 +
                [(True, 129)] * 6))
    return out


def _waiting(dec):
    return len(dec.model.q) - (1 if dec.model.next > 0 else 0)


def _sources(segs, gpos, cpos, gid, cid):
    """[(gen_n, cng_n, fade, dir)] passes -> per internal sample (gen hop, gen offset, cng hop, cng offset, fade index), -1
    where a source is silent; gpos / cpos: read positions before; gid / cid: hops started before.  -> rows, counters"""
    rows = []
    for gen_n, cng_n, fade, d in segs:
        for i in range(max(gen_n, cng_n)):
            g = c = (-1, -1)
            if gen_n:
                if gpos == 0:
                    gid += 1
                g = (gid - 1, gpos)
                gpos = (gpos + 1) % HOP
            if cng_n:
                if cpos == 0:
                    cid += 1
                c = (cid - 1, cpos)
                cpos = (cpos + 1) % HOP
            rows.append(g + c + ((fade + i * d) if gen_n and cng_n else -1,))
    return rows, gid, cid


def _check(rate, name, calls, lines, stats):
    from fake_kit import FakeKit
    from oracle import lyra_codec_model as M
    assert len(lines) == len(calls), name
    kit = FakeKit()
    dec = M.RefLyraDecoder(None, rate, cng_seed=0, kit=kit)
    s = kit.s
    prev_cn = False
    for t, ((pk, n), row) in enumerate(zip(calls, lines)):
        hops0, cng0, est0 = s.dec_hops, s.cng_hops, s.noise_calls[1]
        gpos0, cpos0, left0 = dec.model.next, dec.cng.next, dec.leftover.size
        drop = False
        if pk:
            if _waiting(dec) >= DEPTH:      # the bounded queue: the packet is not delivered at all
                drop = True
            else:
                dec.SetEncodedPacket(np.full(23, 3 + t % 50, np.uint8))
        assert dec.DecodeSamples(n).size == n
        segs = dec.last_segments
        n_int = dec.last_internal.size
        # ---- what the kernels rely on, on the reference model's own trajectory ----
        assert dec.leftover.size <= LEFT_MAX[rate], (name, t, dec.leftover.size)
        assert n_int <= 4 * HOP, (name, t, n_int)
        edges = np.cumsum([0] + [max(g, c) for g, c, _, _ in segs])
        for lo in range(0, n_int, HOP):     # passes that reach into the chunk [lo, lo + 320)
            cut = sum(1 for a, b in zip(edges[:-1], edges[1:]) if a < min(lo + HOP, n_int) and b > lo)
            assert cut <= 2, (name, t, "a chunk of the model's call is cut by", cut, "passes")
        want_src, _, _ = _sources(segs, gpos0, cpos0, hops0, cng0)
        # ---- the driver's line ----
        head, rest = row[:17], row[17:]
        used, got_int, R, nseg = head[13:17]
        want = (dec.concealment, dec.fade, dec.fade_dir, dec.model.next, dec.cng.next, _waiting(dec), dec.leftover.size,
                s.dec_hops - hops0, s.cng_hops - cng0, s.noise_calls[1] - est0, int(dec.is_comfort_noise()), int(drop), 0)
        assert tuple(head[:13]) == want, (name, t, (pk, n), head, want)
        assert (used, got_int) == (min(left0, n), n_int), (name, t, (pk, n), head)
        assert R <= 4 and len(rest) == 8 * nseg
        got_src = []
        for k in range(nseg):
            gen_n, cng_n, gen_off, cng_off, fade, d, gid, cid = rest[8 * k:8 * k + 8]
            for i in range(max(gen_n, cng_n)):
                got_src.append(((gid, gen_off + i) if gen_n else (-1, -1)) + ((cid, cng_off + i) if cng_n else (-1, -1)) +
                               ((fade + i * d) if gen_n and cng_n else -1,))
        assert got_src == want_src, (name, t, (pk, n), "the rounds' samples come from other places than the model's")
        cn = int(dec.is_comfort_noise())
        stats["left"][dec.leftover.size] += 1
        stats["rounds"][R] += 1
        stats["seen_cn"] += cn
        stats["seen_back"] += int(prev_cn and not cn)
        stats["dropped"] += int(drop)
        stats["from_left_only"] += int(n > 0 and n_int == 0)
        stats["cut_pass"] += int(nseg > len(segs))
        prev_cn = bool(cn)


@pytest.mark.parametrize("rate", RATES)
def test_rounds_and_leftover_match_the_reference_model(driver, rate):
    sys.path.insert(0, os.path.join(ROOT, "tests", "host_stub"))
    scripts = _scripts(np.random.default_rng(23 + rate), rate)
    text = "\n".join(" ".join("%d:%d" % (int(p), n) for p, n in calls) for _, calls in scripts) + "\n"
    out = _run(driver, ["plan", rate], text)
    head, _, body = out.partition("\n")
    assert head == "depth %d max_internal 1280 left_max 2" % DEPTH
    blocks = body.split("end\n")[:-1]
    assert len(blocks) == len(scripts)
    stats = dict(left=[0, 0, 0], rounds=[0] * 5, seen_cn=0, seen_back=0, dropped=0, from_left_only=0, cut_pass=0)
    for (name, calls), b in zip(scripts, blocks):
        assert "einval" not in b, name
        _check(rate, name, calls, [list(map(int, ln.split())) for ln in b.strip().splitlines()], stats)
    print(rate, stats)
    assert stats["seen_cn"] > 0 and stats["seen_back"] > 0      # pure comfort noise is reached and left again
    assert all(stats["rounds"][r] > 0 for r in range(5))        # calls of 0, 1, 2, 3 and 4 rounds
    assert stats["cut_pass"] > 0                                # a round boundary did cut a pass of the model's loop
    assert stats["dropped"] >= 3                                # the overflow script
    for k in (1, 2):                                            # every leftover count the rate can reach was reached
        assert (stats["left"][k] > 0) == (k <= LEFT_MAX[rate]), stats["left"]
    if LEFT_MAX[rate]:
        assert stats["from_left_only"] > 0                      # a request served from the leftover alone


@pytest.mark.parametrize("rate", RATES)
def test_integer_n_int_equals_the_reference_float_expression(driver, rate):
    """buffered_resampler.cc: ceil(float(n - L) / (float(rate) / 16000.f)), for every n of 0 .. 4 hops and L of 0 .. 2."""
    rows = np.array([ln.split() for ln in _run(driver, ["nint", rate]).splitlines()], np.int64)
    n, L, used, n_int, left, rounds = rows.T
    assert rows.shape[0] == 3 * (4 * rate // 50 + 1)
    ratio = np.float32(rate) / np.float32(16000)
    want = np.where(n > L, np.ceil((n - L).astype(np.float32) / ratio).astype(np.int64), 0)
    assert np.array_equal(n_int, want)
    assert np.array_equal(used, np.minimum(n, L))
    made = n_int * rate // 16000
    assert np.array_equal(left, np.where(n_int > 0, made - (n - used), L - used))
    assert left.min() >= 0 and left.max() <= 2 and n_int.max() <= 4 * HOP
    whole = -((-n * 16000) // rate)                              # ceil(n * 16000 / rate)
    assert np.array_equal(rounds, -((-whole) // HOP)) and (n_int <= rounds * HOP).all()


def test_request_size_rule(driver):
    for rate, hop in ((8000, 160), (16000, 320), (32000, 640), (48000, 960)):
        ns = [-1, 0, 1, 128, 441, hop, 4 * hop - 1, 4 * hop, 4 * hop + 1, 10 ** 6]
        got = [int(x) for x in _run(driver, ["valid", rate] + ns).split()]
        assert got == [0, 1, 1, 1, 1, 1, 1, 1, 0, 0], (rate, got)
    assert set(_run(driver, ["valid", 44100, 0, 441, 882]).split()) == {"0"}
    assert set(_run(driver, ["valid", 0, 0, 1]).split()) == {"0"}


def test_validate_holds_the_leftover_count_to_its_domain(tmp_path):
    import json
    from state_bridge import _reset_blob, _verdicts, compile_tool
    tool = compile_tool(tmp_path)
    L = json.loads(subprocess.check_output([tool, "layout"]))
    good = _reset_blob(tool, tmp_path)
    off = L["pieces"][10][0] + 4            # R_RS_D, DSA_LEFT_COUNT
    assert off == L["pieces"][10][0] + L["rs_in_pos"] + 4
    cases = []
    for v in (0, 1, 2, 3, 4, 255, 256, 2 ** 31, 2 ** 32 - 1):
        b = good.copy()
        b[off:off + 4] = np.frombuffer(np.array([v], "<u4").tobytes(), np.uint8)
        b[off + 4:off + 8] = [0x34, 0x12, 0xCD, 0xAB]        # the two samples are payload: any value passes
        cases.append(b)
    got = _verdicts(tool, tmp_path, np.stack(cases))
    assert got[:3] == [0, 0, 0], got
    assert len(set(got[3:])) == 1 and got[3] == 15, got      # V_DSA_LEFT, appended behind V_CNG_HEADER (14)
    # the verdict is the LAST one: a blob that also fails an older check keeps that check's verdict
    b = cases[3].copy(); b[L["pieces"][10][0]] = 6           # RS_IN_POS out of domain
    assert _verdicts(tool, tmp_path, b[None]) == [11]
    # the same word in the ENCODER's resampler slot means nothing and is not looked at
    b = good.copy(); b[L["pieces"][9][0] + 4] = 9
    assert _verdicts(tool, tmp_path, b[None]) == [0]


NEW = {"lyra_hip_decode_samples_any_dev": 10, "lyra_hip_decode_samples_any_begin": 7, "lyra_hip_decode_samples_any_end": 2}


def test_header_table_and_library_agree_on_the_three_symbols():
    import re
    from abi_loading import _protos, load_library
    from lyra_amd import codec
    lib = load_library()
    protos = _protos("lyra_hip_decode_samples_any.h")
    assert set(protos) == set(NEW) == set(codec._SIGNATURES_DECODE_SAMPLES_ANY)
    for name, n_args in NEW.items():
        args = [a.strip() for a in protos[name].split(",")]
        assert len(args) == n_args, (name, args)
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name} is not exported by {codec.library_path()}"
        restype, argtypes = codec._SIGNATURES_DECODE_SAMPLES_ANY[name]
        assert restype is codec.C.c_int and fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        for a, t in zip(args, argtypes):   # pointers as void pointers, everything else an int
            assert t is (codec.C.c_void_p if "*" in a else codec.C.c_int), (name, a, t)
        assert fn(*[None if t is codec.C.c_void_p else 0 for t in argtypes]) < 0, name      # a null context is refused
        assert callable(getattr(codec.LyraHip, name[len("lyra_hip_"):], None)), name
    others = (set(codec._SIGNATURES) | set(codec._SIGNATURES_SPANS_MIXED) | set(codec._SIGNATURES_SPANS_RATES) |
              set(codec._SIGNATURES_SPANS_PACKED) | set(codec._SIGNATURES_ENCODE_STREAMS) | set(codec._SIGNATURES_DECODE_STREAMS))
    assert not set(NEW) & others
    hdr = open(os.path.join(ROOT, "include", "lyra_hip_decode_samples_any.h")).read()
    assert "#define LYRA_HIP_DECODE_SAMPLES_MAX_HOPS 4" in hdr and '#include "lyra_hip.h"' in hdr
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lyra_hip.h")).read(), flags=re.S)
    assert "decode_samples_any" not in text    # (lyra_hip.h points to the new header in a comment only)
    image = open(codec.library_path(), "rb").read()
    for kernel in (b"ds_plan_any_kernel", b"ds_splice_kernel"):
        assert re.search(rb"_ZN4lyra\d+" + kernel + rb"E\w*\.kd", image), kernel
