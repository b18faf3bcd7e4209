"""CPU: what lyra_hip_decode_samples_streams_dev decides per row (lyra_amd/csrc/decode_samples_streams_plan.h) -- the row
verdict, the rounds of a batch, the packed layout -- compiled with a plain C++ compiler, WITH -fsanitize=address,undefined, and
driven as a program of its own against a Python restatement of the call's documentation
(include/lyra_hip_decode_samples_streams.h).  And: the header, the ctypes table of lyra_amd/codec.py and the built library agree
on the three symbols."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
OK, BAD_RATE, BAD_SIZE, BAD_ROUNDS, BAD_OFFSET = range(5)
CODEC_RATES = (8000, 16000, 32000, 48000)
STRIDE = 4 * 960

_DRIVER = r'''
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "decode_samples_streams_plan.h"
// verdict: one row per input line "<rate> <n> <max_hops> <offset> <n_pcm>" -> its verdict
// rounds:  one batch per input line "<rate>:<n> ..." -> dss_batch_rounds
// packed <first> <count> <size> ...: `count` rows whose sizes cycle through the list, behind `first` rows of 3839 samples ->
//          the last row's offset and the total
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  static char line[1 << 16];
  if (!std::strcmp(argv[1], "verdict")) {
    while (std::fgets(line, sizeof line, stdin)) {
      int rate, n, hops;
      long off, n_pcm;
      if (std::sscanf(line, "%d %d %d %ld %ld", &rate, &n, &hops, &off, &n_pcm) != 5) return 2;
      std::printf("%d\n", lyra::dss_row_verdict(rate, n, hops, off, n_pcm));
    }
    return 0;
  }
  if (!std::strcmp(argv[1], "rounds")) {
    while (std::fgets(line, sizeof line, stdin)) {
      std::vector<int32_t> rates, sizes;
      for (char* tok = std::strtok(line, " \n"); tok; tok = std::strtok(nullptr, " \n")) {
        int r, n;
        if (std::sscanf(tok, "%d:%d", &r, &n) != 2) return 2;
        rates.push_back(r); sizes.push_back(n);
      }
      std::printf("%d\n", lyra::dss_batch_rounds(rates.data(), sizes.data(), (int)rates.size()));
    }
    return 0;
  }
  if (!std::strcmp(argv[1], "packed") && argc > 4) {
    const long first = std::atol(argv[2]), count = std::atol(argv[3]);
    std::vector<int32_t> sizes((size_t)(first + count), 3839);
    for (long i = 0; i < count; ++i) sizes[(size_t)(first + i)] = std::atoi(argv[4 + i % (argc - 4)]);
    std::vector<long> offs(sizes.size());
    const long total = lyra::dss_packed_offsets(sizes.data(), (int)sizes.size(), offs.data());
    for (size_t i = 1; i < sizes.size(); ++i)
      if (offs[i] != offs[i - 1] + (sizes[i - 1] > 0 ? sizes[i - 1] : 0)) return 3;
    std::printf("%ld %ld %ld %d %ld\n", offs[0], offs.back(), total, lyra::DSS_ROW_STRIDE, lyra::dss_default_offset(289261));
    return 0;
  }
  return 2;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("plan_streams")
    src, exe = d / "plan_streams.cc", d / "plan_streams"
    src.write_text(_DRIVER)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "lyra_amd", "csrc"), str(src),
                           "-o", str(exe)], timeout=300)
    return str(exe)


def _run(driver, args, text=""):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    r = subprocess.run([driver] + [str(a) for a in args], input=text, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r.stdout.split("\n")[:-1]


def _rounds(n, rate):
    """ceil(ceil(n * 16000 / rate) / 320): hops of internal samples"""
    return (-(-n * 16000 // rate) + 319) // 320


def _verdict(rate, n, hops, off, n_pcm):
    """The header's "Invalid rows", in its order"""
    if rate not in CODEC_RATES:
        return BAD_RATE
    if not 0 <= n <= 4 * rate // 50:
        return BAD_SIZE
    if _rounds(n, rate) > hops:
        return BAD_ROUNDS
    if off < 0 or off + n > n_pcm:
        return BAD_OFFSET
    return OK


def test_row_verdict_at_and_around_every_bound(driver):
    cases = []
    n_pcm = 100000
    for rate in CODEC_RATES + (44100, 0, -16000, 16001, 96000):
        top = 4 * (rate // 50) if rate > 0 else 0
        sizes = {-1, 0, 1, top - 1, top, top + 1}
        for hops in (1, 2, 3, 4):       # ... and the largest size of `hops` rounds, and one more
            edge = 320 * hops * rate // 16000 if rate > 0 else 0
            sizes |= {edge - 1, edge, edge + 1}
        for n in sorted(sizes):
            for hops in (1, 2, 3, 4):
                cases.append((rate, n, hops, 0, n_pcm))
    for rate, n in ((48000, 441), (16000, 1), (8000, 640), (32000, 0)):      # both ends of the buffer, one sample past each
        for off in (-1, 0, 1, n_pcm - n - 1, n_pcm - n, n_pcm - n + 1, n_pcm, n_pcm + 1):
            cases.append((rate, n, 4, off, n_pcm))
        cases += [(rate, n, 4, 0, n), (rate, n, 4, 0, n - 1), (rate, n, 4, 0, 0), (rate, n, 4, 2 ** 40, 2 ** 40 + n),
                  (rate, n, 4, 2 ** 40 + 1, 2 ** 40 + n)]
    got = _run(driver, ["verdict"], "".join("%d %d %d %d %d\n" % c for c in cases))
    want = [_verdict(*c) for c in cases]
    assert [int(g) for g in got] == want, [(c, g, w) for c, g, w in zip(cases, got, want) if int(g) != w][:10]
    assert {OK, BAD_RATE, BAD_SIZE, BAD_ROUNDS, BAD_OFFSET} == set(want)
    # what the documentation promises in words
    assert _verdict(48000, 961, 1, 0, n_pcm) == BAD_ROUNDS and _verdict(48000, 960, 1, 0, n_pcm) == OK
    assert _verdict(48000, 441, 1, n_pcm - 440, n_pcm) == BAD_OFFSET and _verdict(32000, 0, 1, n_pcm, n_pcm) == OK


def test_batch_rounds_are_the_max_over_valid_rows(driver):
    rng = np.random.default_rng(17)
    batches = [[(48000, 0)], [(48000, 0), (8000, 0)], [(44100, 3000), (48000, 1)], [(48000, 3841), (16000, 321)],
               [(8000, 160), (32000, 441), (48000, 1024)], [(16000, 1280)], [(48000, -5), (32000, 2561)]]
    for _ in range(40):
        rates = rng.choice(CODEC_RATES + (44100,), size=rng.integers(1, 12))
        batches.append([(int(r), int(rng.integers(-2, 4 * max(r, 1) // 50 + 3))) for r in rates])
    got = _run(driver, ["rounds"], "".join(" ".join(f"{r}:{n}" for r, n in b) + "\n" for b in batches))
    want = [max([1] + [_rounds(n, r) for r, n in b if r in CODEC_RATES and 0 <= n <= 4 * r // 50]) for b in batches]
    assert [int(g) for g in got] == want
    assert set(want) == {1, 2, 3, 4}


def test_packed_layout_stays_exact_beyond_2_to_the_31(driver):
    """600,000 rows of 3839 samples put 2.3e9 samples in front of rows of odd sizes: the offsets are `long`."""
    first, sizes = 600000, [441, 1, 0, 959, 3, -7, 75]
    count = 1000
    seq = [sizes[i % len(sizes)] for i in range(count)]
    off0, last, total, stride, far = (int(x) for x in _run(driver, ["packed", first, count] + sizes)[0].split())
    want_total = first * 3839 + sum(max(s, 0) for s in seq)
    assert off0 == 0 and total == want_total and last == want_total - max(seq[-1], 0)
    assert first * 3839 > 2 ** 31 and last > 2 ** 31
    assert stride == STRIDE and far == 289261 * STRIDE          # the default layout at the largest documented stream count
    assert far + STRIDE < 2 ** 31                                # ... fits the int32 offsets of the device call


NEW = {"lyra_hip_decode_samples_streams_dev": 13, "lyra_hip_decode_samples_streams_begin": 7,
       "lyra_hip_decode_samples_streams_end": 4}


def test_header_table_and_library_agree_on_the_three_symbols():
    from abi_loading import _protos, load_library
    from lyra_amd import codec
    lib = load_library()
    protos = _protos("lyra_hip_decode_samples_streams.h")
    assert set(protos) == set(NEW) == set(codec._SIGNATURES_DECODE_SAMPLES_STREAMS)
    for name, n_args in NEW.items():
        args = [a.strip() for a in protos[name].split(",")]
        assert len(args) == n_args, (name, args)
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name} is not exported by {codec.library_path()}"
        restype, argtypes = codec._SIGNATURES_DECODE_SAMPLES_STREAMS[name]
        assert restype is codec.C.c_int and fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert len(argtypes) == n_args, (name, argtypes)
        for a, t in zip(args, argtypes):   # pointers as void pointers, `long` as a long, everything else an int
            want = codec.C.c_void_p if "*" in a else codec.C.c_long if a.startswith("long ") else codec.C.c_int
            assert t is want, (name, a, t)
        assert fn(*[None if t is codec.C.c_void_p else 0 for t in argtypes]) < 0, name      # a null context is refused
        assert callable(getattr(codec.LyraHip, name[len("lyra_hip_"):], None)), name
    others = (set(codec._SIGNATURES) | set(codec._SIGNATURES_SPANS_MIXED) | set(codec._SIGNATURES_SPANS_RATES) |
              set(codec._SIGNATURES_SPANS_PACKED) | set(codec._SIGNATURES_ENCODE_STREAMS) | set(codec._SIGNATURES_DECODE_STREAMS) |
              set(codec._SIGNATURES_DECODE_SAMPLES_ANY))
    assert not set(NEW) & others
    hdr = open(os.path.join(ROOT, "include", "lyra_hip_decode_samples_streams.h")).read()
    assert '#include "lyra_hip_decode_samples_any.h"' in hdr
    for older in ("lyra_hip.h", "lyra_hip_decode_samples_any.h", "lyra_hip_decode_streams.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", older)).read(), flags=re.S)
        assert "decode_samples_streams" not in text, older
    image = open(codec.library_path(), "rb").read()
    assert set(re.findall(rb"hip[v\d]*-amdgcn-amd-amdhsa--(gfx\w+)", image)) == {b"gfx950"}
    for kernel in (b"ds_plan_streams_kernel", b"ds_splice_streams_kernel", b"ds_plan_any_kernel", b"ds_splice_kernel"):
        assert re.search(rb"_ZN4lyra\d+" + kernel + rb"E\w*\.kd", image), kernel
