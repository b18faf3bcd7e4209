"""CPU: the general packet-loss transition of lyra_hip_decode_samples_dev (lyra_amd/csrc/decode_samples_plan.h, compiled
here with a plain C++ compiler) against oracle/lyra_codec_model.py's RefLyraDecoder -- SetEncodedPacket when a packet
arrives, then DecodeSamples(n) for request sizes that are not tied to the 20 ms hop -- with tests/host_stub/fake_kit.py's
counting components.  After every call: the integers (concealment / fade progress, fade direction, the read positions in
both hops, the waiting feature vectors), how many generative hops, comfort-noise hops and estimator calls the call made,
the slices (last_segments), is_comfort_noise(), and whether a comfort-noise hop that starts in the call reads the noise
estimate before or after the call's estimator update (FakeKit's comfort noise carries the estimator's call count).

The bounds the device call is built on are asserted on the REFERENCE MODEL's trajectory: for internal requests of at most
one hop DecodeSamplesInternal's loop runs at most twice, starts at most one generative and one comfort-noise hop, and
completes at most one received hop; and no script but the overflow script ever holds more than DS_FIFO_DEPTH waiting
vectors in the model's own queue."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from signals import _gilbert_ticks

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEPTH = 4   # DS_FIFO_DEPTH; the driver prints the header's value and the test compares

_DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "decode_samples_plan.h"
// argv[1] = sample rate.  One script per input line: tokens "<packet 0/1>:<n external samples>" per call.
int main(int argc, char** argv) {
  const int rate = std::atoi(argv[1]);
  static char line[1 << 20];
  std::printf("depth %d\n", lyra::DS_FIFO_DEPTH);
  while (std::fgets(line, sizeof line, stdin)) {
    lyra::DsState s;
    std::memset(&s, 0, sizeof s);   // all zero = the reference's initial state
    for (char* tok = std::strtok(line, " \n"); tok; tok = std::strtok(nullptr, " \n")) {
      int pk = 0, n = 0;
      if (std::sscanf(tok, "%d:%d", &pk, &n) != 2) return 2;
      const int ni = lyra::ds_internal_samples(n, rate);
      if (ni < 0) { std::printf("einval\n"); continue; }
      const lyra::DsPlan p = lyra::ds_plan(s, pk != 0, ni);
      s = p.s;
      int32_t w[4];
      lyra::ds_info(p, w);
      std::printf("%d %d %d %d %d %d  %d %d %d %d  %d %d %d  %d", s.cp, s.fade, s.to_cng ? 1 : -1, s.gpos, s.cpos, s.wait,
                  p.gen_start >= 0, p.cng_start >= 0, p.est_seg >= 0, p.est_seg >= 0 && p.cng_start > p.est_seg,
                  p.comfort_noise, p.dropped, p.bad, p.nseg);
      for (int k = 0; k < p.nseg; ++k) std::printf(" %d %d %d %d", p.seg[k].gen_n, p.seg[k].cng_n, p.seg[k].fade, p.seg[k].dir);
      std::printf("  %d %d %d %d", w[0], w[1], w[2], w[3]);
      for (int k = 0; k < p.nseg; ++k) std::printf("  %d %d", p.seg[k].gen_off, p.seg[k].cng_off);
      std::printf("\n");
    }
    std::printf("end\n");
  }
  return 0;
}
'''


def _gilbert(rng, ticks):
    return _gilbert_ticks(rng, ticks, recover_from=0.1).tolist()


def _scripts(rng, rate):
    """-> list of (name, [(packet, n_ext), ...]).  Every n obeys the size rule of the call (n * 16000 % rate == 0)."""
    half = rate // 100                       # 10 ms
    unit = {8000: 1, 16000: 1, 32000: 2, 48000: 3}[rate]
    top = rate // 50 // unit
    out = []
    # 10 ms requests, the packet of every 20 ms on the even / on the odd tick, every packet received and then long losses
    for phase in (0, 1):
        got = [True] * 8 + [False] * 14 + [True] * 9 + [False] * 3 + [True] * 4
        out.append(("10ms phase %d" % phase, [(t % 2 == phase and got[t // 2], half) for t in range(2 * len(got))]))
    for i in range(30):                      # Gilbert chains under 10 ms requests
        got = _gilbert(rng, int(rng.integers(20, 80)))
        phase = i & 1
        out.append(("gilbert 10ms", [(t % 2 == phase and got[t // 2], half) for t in range(2 * len(got))]))
    for late in (1, 2):                      # jitter: a packet handed over `late` ticks late, the next one on time
        calls, owed = [], 0
        for t in range(120):
            due = t % 2 == 0 and not (30 <= t < 70 and (t // 2) % 3 == 0)    # some packets are lost outright
            if due and (t // 2) % 5 == 2:
                owed, due = late, False      # ... and every fifth is late
            elif owed:
                owed -= 1
                if owed == 0:
                    calls.append((True, 0))  # the late packet in a call of its own (n = 0: SetEncodedPacket alone)
            calls.append((due, half))
        out.append(("late %d" % late, calls))
    for _ in range(40):                      # random request sizes, random arrivals (queue kept within the depth below)
        calls, ahead = [], 0.0               # arrivals run at most two packets ahead of the playout clock
        p_pk = rng.choice([0.1, 0.5, 0.9])
        for _ in range(int(rng.integers(40, 160))):
            n = int(rng.integers(0, top + 1)) * unit
            pk = bool(rng.random() < p_pk) and ahead <= 1.0
            ahead = max(0.0, ahead + int(pk) - n * 50 / rate)
            calls.append((pk, n))
        out.append(("random n", calls))
    for _ in range(10):                      # full hops with Gilbert loss: the hop-synchronous regime is a special case
        out.append(("hop", [(g, rate // 50) for g in _gilbert(rng, 60)]))
    return out


def _overflow_script(rate):
    half = rate // 100
    return [(True, half), (False, half)] * 2 + [(True, 0)] * (DEPTH + 3) + [(False, half)] * 30 + [(True, half)] * 6


def _run_driver(tmp_path, rate, scripts):
    src, exe = tmp_path / "plan.cc", tmp_path / "plan"
    src.write_text(_DRIVER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "lyra_amd", "csrc"), str(src),
                           "-o", str(exe)], timeout=120)
    text = "\n".join(" ".join("%d:%d" % (int(p), n) for p, n in calls) for _, calls in scripts) + "\n"
    r = subprocess.run([str(exe), str(rate)], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    head, _, body = r.stdout.partition("\n")
    assert head == "depth %d" % DEPTH
    blocks = body.split("end\n")[:-1]
    assert len(blocks) == len(scripts)
    return [[list(map(int, ln.split())) for ln in b.strip().splitlines() if ln != "einval"] for b in blocks]


def _waiting(dec):
    return len(dec.model.q) - (1 if dec.model.next > 0 else 0)


def _check(rate, name, calls, rows, overflow, stats):
    from fake_kit import FakeKit
    from oracle import lyra_codec_model as M
    assert len(rows) == len(calls), name
    kit = FakeKit()
    dec = M.RefLyraDecoder(None, rate, cng_seed=0, kit=kit)
    s = kit.s
    prev_cn = False
    for t, ((pk, n), row) in enumerate(zip(calls, rows)):
        hops0, cng0, est0 = s.dec_hops, s.cng_hops, s.noise_calls[1]
        gpos0, cpos0 = dec.model.next, dec.cng.next
        drop = False
        if pk:
            if _waiting(dec) >= DEPTH:      # the bounded queue: the packet is not delivered at all
                assert overflow, (name, t, "a script other than the overflow script fills the queue of the model")
                drop = True
            else:
                dec.SetEncodedPacket(np.full(23, 3 + t % 50, np.uint8))
                stats["max_wait"] = max(stats["max_wait"], _waiting(dec)) if not overflow else stats["max_wait"]
        assert dec.DecodeSamples(n).size == n
        assert dec.leftover.size == 0       # the size rule keeps BufferedResampler's leftover empty
        segs = dec.last_segments
        gen_hops, cng_hops, est = s.dec_hops - hops0, s.cng_hops - cng0, s.noise_calls[1] - est0
        # ---- the bounds, on the reference model's own trajectory ----
        assert len(segs) <= 2 and gen_hops <= 1 and cng_hops <= 1 and est <= 1, (name, t, segs, gen_hops, cng_hops, est)
        # comfort noise that started in this call: did it read the estimate after this call's estimator update?
        after = 0
        if cng_hops:
            seen = (int(dec.cng.hop[0]) - 2000 - 11 * cng0) // 3    # the estimator's call count the generator saw
            assert seen in (est0, est0 + est)
            after = int(est == 1 and seen == est0 + 1)
            if est == 1:
                stats["cng_after_est" if after else "cng_before_est"] += 1
        cp, fade, fdir, gpos, cpos, wait, g, c, e, c_after, cn, dropped, bad, nseg = row[:14]
        want = (dec.concealment, dec.fade, dec.fade_dir, dec.model.next, dec.cng.next, _waiting(dec), gen_hops, cng_hops,
                est, after, int(dec.is_comfort_noise()), int(drop), 0, len(segs))
        assert tuple(row[:14]) == want, (name, t, (pk, n), row, want)
        got_segs = [tuple(row[14 + 4 * k:18 + 4 * k]) for k in range(nseg)]
        assert got_segs == [tuple(x) for x in segs], (name, t, got_segs, segs)
        # the packed form the kernels read says the same
        w0, w1, w2, w3 = row[14 + 4 * nseg:18 + 4 * nseg]
        # where each pass reads its hops: pass 1 goes on where the model's FIFOs stood before the call, and pass 2 -- the
        # kernel has no offset word for it -- always starts at sample 0 of a hop that this call started
        offs = row[18 + 4 * nseg:]
        assert len(offs) == 2 * nseg
        if nseg:
            assert (offs[0], offs[1]) == (gpos0, cpos0) and w2 == (gpos0 | (cpos0 << 16))
            assert offs[0] + segs[0][0] <= 320 and offs[1] + segs[0][1] <= 320
        if nseg == 2:
            assert (offs[2], offs[3]) == (0, 0)
            assert (not segs[1][0] or (w1 & 64)) and (not segs[1][1] or (w1 & 128))
            assert max(segs[1][0], segs[1][1]) <= 320
        for g_n, c_n, f0, d in segs:       # the cross-fade's weight index stays inside the table (-640 .. 1280)
            if g_n and c_n:
                assert -640 <= f0 + min(0, d * (g_n - 1)) and f0 + max(0, d * (g_n - 1)) <= 1280
        ns = [w0 & 0xffff, w0 >> 16]
        assert [x for x in ns if x] == [max(a, b) for a, b, _, _ in segs]
        assert bool(w1 & 64) == bool(gen_hops) and bool(w1 & 128) == bool(cng_hops) and bool(w1 & 256) == bool(est)
        assert bool(w1 & 1024) == dec.is_comfort_noise()
        if segs:
            assert (w3 & 0xffff) == segs[0][2] and bool(w1 & 16) == (segs[0][3] > 0)
            assert bool(w1 & 1) == bool(segs[0][0]) and bool(w1 & 2) == bool(segs[0][1])
        if len(segs) == 2:
            assert (w3 >> 16) == segs[1][2] and bool(w1 & 32) == (segs[1][3] > 0)
            assert bool(w1 & 4) == bool(segs[1][0]) and bool(w1 & 8) == bool(segs[1][1])
        stats["two_pass"] += int(len(segs) == 2)
        stats["seen_cn"] += cn
        stats["seen_back"] += int(prev_cn and not cn)
        stats["dropped"] += int(drop)
        prev_cn = bool(cn)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
@pytest.mark.parametrize("rate", [16000, 48000, 8000, 32000])
def test_decode_samples_transition_matches_reference_model(tmp_path, rate):
    sys.path.insert(0, os.path.join(ROOT, "tests", "host_stub"))
    scripts = _scripts(np.random.default_rng(11 + rate), rate)
    scripts.append(("overflow", _overflow_script(rate)))
    blocks = _run_driver(tmp_path, rate, scripts)
    stats = dict(max_wait=0, cng_after_est=0, cng_before_est=0, two_pass=0, seen_cn=0, seen_back=0, dropped=0)
    for (name, calls), rows in zip(scripts, blocks):
        _check(rate, name, calls, rows, name == "overflow", stats)
    print(rate, stats)
    assert stats["seen_cn"] > 0 and stats["seen_back"] > 0      # pure comfort noise is reached and left again
    assert stats["two_pass"] > 0
    assert stats["cng_after_est"] > 0 and stats["cng_before_est"] > 0   # both orders of estimator and comfort noise occur
    assert 2 <= stats["max_wait"] <= DEPTH                      # the late-packet scripts queue, and stay inside the depth
    assert stats["dropped"] == 3                                # the overflow script: DEPTH + 3 packets into an empty queue


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_request_size_rule(tmp_path):
    """0 <= n <= rate / 50 and n * 16000 divisible by the rate; everything else is refused."""
    cases = {16000: [(0, 1), (1, 1), (37, 1), (320, 1), (321, 0), (-1, 0)],
             48000: [(480, 1), (3, 1), (481, 0), (482, 0), (960, 1), (963, 0)],
             32000: [(320, 1), (321, 0), (640, 1), (642, 0)],
             8000: [(80, 1), (1, 1), (160, 1), (161, 0)],
             44100: [(441, 0)]}
    for rate, lst in cases.items():
        rows = _run_driver(tmp_path, rate, [("x", [(False, n)]) for n, _ in lst])
        for (n, ok), r in zip(lst, rows):
            assert (len(r) == 1) == bool(ok), (rate, n, r)      # "einval" lines do not parse into a row
