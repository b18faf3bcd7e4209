"""CPU: the per-tick packet-loss transition of lyra_hip_decode_lossy_dev (lyra_amd/csrc/lossy_plan.h, compiled here with a
plain C++ compiler) against oracle/lyra_codec_model.py's RefLyraDecoder driven hop-synchronously -- SetEncodedPacket when
a packet arrives, then DecodeSamples(rate / 50) -- over random loss scripts, with tests/host_stub/fake_kit.py's counting
components: the integer trajectory (concealment progress, fade progress, fade direction), which legs run every tick
(generative model, comfort-noise generator, decoder-side noise estimator) and is_comfort_noise()."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

_DRIVER = r'''
#include <cstdio>
#include <cstring>
#include "lossy_plan.h"
// one loss script per input line ("0" / "1" per tick); per tick: cp fade dir gen cng est cn mix_fade mix_dir
int main() {
  static char line[1 << 16];
  while (std::fgets(line, sizeof line, stdin)) {
    uint32_t ctl = 0;   // all-zero control word = the reference's initial state
    for (const char* p = line; *p == '0' || *p == '1'; ++p) {
      const lyra::LossyTick t = lyra::lossy_tick(ctl, *p == '1');
      ctl = t.ctl;
      std::printf("%d %d %d %d %d %d %d %d %d\n", t.cp, t.fade, t.dir, t.run_gen, t.run_cng, t.feed_est, t.comfort_noise,
                  t.mix_fade, t.mix_dir);
    }
    std::printf("end\n");
  }
  return 0;
}
'''


def _scripts(rng):
    out = ["0" * 12, "1" * 5 + "0" * 14 + "1" * 6, "0101100011100000000000110"]
    for _ in range(40):   # two-state (Gilbert) chains of varied loss and burst length
        p_loss, p_recover = rng.uniform(0.02, 0.5), rng.uniform(0.1, 0.9)
        lost, s = rng.random() < 0.3, []
        for _ in range(int(rng.integers(20, 80))):
            lost = (rng.random() >= p_recover) if lost else (rng.random() < p_loss)
            s.append("0" if lost else "1")
        out.append("".join(s))
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
@pytest.mark.parametrize("rate", [16000, 48000])
def test_lossy_transition_matches_reference_model(tmp_path, rate):
    sys.path.insert(0, os.path.join(ROOT, "tests", "host_stub"))
    from fake_kit import FakeKit
    from oracle import lyra_codec_model as M
    src, exe = tmp_path / "plan.cc", tmp_path / "plan"
    src.write_text(_DRIVER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "lyra_amd", "csrc"), str(src),
                           "-o", str(exe)], timeout=120)
    scripts = _scripts(np.random.default_rng(7))
    r = subprocess.run([str(exe)], input="\n".join(scripts) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    blocks = r.stdout.split("end\n")[:-1]
    assert len(blocks) == len(scripts)
    seen_cn = seen_back = 0
    for script, block in zip(scripts, blocks):
        rows = [list(map(int, ln.split())) for ln in block.strip().splitlines()]
        assert len(rows) == len(script)
        kit = FakeKit()
        dec = M.RefLyraDecoder(None, rate, cng_seed=0, kit=kit)
        s = kit.s
        prev_cn = False
        for t, (c, row) in enumerate(zip(script, rows)):
            hops0, cng0, est0 = s.dec_hops, s.cng_hops, s.noise_calls[1]
            fade0 = dec.fade
            if c == "1":
                dec.SetEncodedPacket(np.full(23, 3 + t % 50, np.uint8))
            assert dec.DecodeSamples(rate // 50).size == rate // 50
            cp, fade, fdir, gen, cng, est, cn, mix_fade, mix_dir = row
            want = (dec.concealment, dec.fade, dec.fade_dir, s.dec_hops - hops0, s.cng_hops - cng0, s.noise_calls[1] - est0,
                    int(dec.is_comfort_noise()))
            assert (cp, fade, fdir, gen, cng, est, cn) == want, (script, t, row, want)
            assert mix_fade == fade0            # the cross-fade starts from the pre-update progress
            if gen and cng:
                assert mix_dir == fdir and (fade0, fade) in ((0, 320), (320, 640), (640, 320), (320, 0))
            seen_cn += cn
            seen_back += int(prev_cn and not cn)
            prev_cn = bool(cn)
    assert seen_cn > 0 and seen_back > 0       # the scripts reach pure comfort noise and come back from it


_WEIGHTS = r'''
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
// the cross-fade weight as a float variable initialised from the C++ expression, for fade progress -640 .. 1280
int main() {
  for (int f = -640; f <= 1280; ++f) {
    const float w = (1.f + std::cos(f * M_PI / 640)) / 2.f;
    uint32_t u;
    std::memcpy(&u, &w, 4);
    std::printf("%u\n", u);
  }
  return 0;
}
'''


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_fade_weight_is_the_cpp_expression(tmp_path):
    """oracle/lyra_codec_model.fade_weight (the model's cross-fade) against the overlap weight of MaybeOverlapAndInsert
    (lyra_decoder.cc:364-365) as a C++ compiler evaluates it -- in double, rounded to float once -- bit for bit over every
    fade progress the decoder can reach and beyond.  The float32 evaluation NumPy 2 gives np.float32(1) + math.cos(..)
    is off by one ulp in about a third of them; the check must see that."""
    from oracle import lyra_codec_model as M
    import math
    src, exe = tmp_path / "w.cc", tmp_path / "w"
    src.write_text(_WEIGHTS)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", str(src), "-o", str(exe)], timeout=120)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    want = np.array(r.stdout.split(), np.uint32).view(np.float32)
    f = np.arange(-640, 1281)
    assert want.size == f.size
    got = np.array([M.fade_weight(int(x)) for x in f], np.float32)
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    single = np.array([np.float32((np.float32(1.0) + math.cos(x * math.pi / 640)) / np.float32(2.0)) for x in f], np.float32)
    assert (single.view(np.uint32) != want.view(np.uint32)).sum() > 100      # the test tells the two apart
