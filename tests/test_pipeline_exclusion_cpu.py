"""CPU: which pipelined host-buffer forms may be in flight together (lyra_amd/csrc/pipelines.h) -- the table every begin()
guard, the bridge's and the export/import guard loop over -- compiled with a plain C++ compiler and printed by a program of
its own.  The relation is written out here, literally; closing the decode <-> decode_samples gap is a behaviour change and
has to change this file."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

_DRIVER = r'''
#include <cstdio>
#include "pipelines.h"
int main() {
  std::printf("%d %d\n", (int)lyra::PL_COUNT, lyra::PL_DEPTH);
  for (int p = 0; p < lyra::PL_COUNT; ++p) {
    std::printf("%s", lyra::PL_NAME[p]);
    for (int o = 0; o < lyra::PL_COUNT; ++o) std::printf(" %d", (int)lyra::PL_EXCLUDES[p][o]);
    std::printf("\n");
  }
  for (int p = 0; p < lyra::PL_COUNT; ++p) std::printf("%s %s\n", lyra::PL_NAME[p], lyra::PL_IN_FLIGHT_NOUN[p]);
  return 0;
}
'''

NAMES = ["encode", "decode", "twin_fetch", "encode_streams", "decode_streams", "decode_samples", "decode_samples_any",
         "decode_samples_streams", "bridge"]
PL_COUNT = len(NAMES)
DECODE_GROUP = ["decode", "decode_streams", "decode_samples", "decode_samples_any", "decode_samples_streams"]
# row: the pipeline whose begin() is asked; column: the pipeline in flight; 1: refused
#            enc dec twf es  dst ds  dsa dss brg
RELATION = [[0, 0, 0, 1, 0, 0, 0, 0, 1],    # encode
            [0, 0, 0, 0, 1, 0, 1, 1, 1],    # decode
            [0, 0, 0, 0, 0, 0, 0, 0, 1],    # twin_fetch
            [1, 0, 0, 0, 0, 0, 0, 0, 1],    # encode_streams
            [0, 1, 0, 0, 0, 1, 1, 1, 1],    # decode_streams
            [0, 0, 0, 0, 1, 0, 1, 1, 1],    # decode_samples
            [0, 1, 0, 0, 1, 1, 0, 1, 1],    # decode_samples_any
            [0, 1, 0, 0, 1, 1, 1, 0, 1],    # decode_samples_streams
            [1, 1, 1, 1, 1, 1, 1, 1, 0]]    # bridge


@pytest.fixture(scope="module")
def table_lines(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("pipelines")
    src, exe = d / "pipelines.cc", d / "pipelines"
    src.write_text(_DRIVER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "lyra_amd", "csrc"), str(src),
                           "-o", str(exe)], timeout=300)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")[:-1]
    count, depth = (int(x) for x in lines[0].split())
    assert count == 9 and depth == 2 and len(lines) == 1 + 2 * PL_COUNT
    return lines


@pytest.fixture(scope="module")
def table(table_lines):
    return {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in table_lines[1:PL_COUNT + 1]}


def test_the_table_is_the_relation_written_out_here(table):
    assert list(table) == NAMES
    for name, row in zip(NAMES, RELATION):
        assert table[name] == row, name


def test_the_relation_in_words(table):
    ex = {(a, b): bool(table[a][NAMES.index(b)]) for a in NAMES for b in NAMES}
    assert not any(ex[a, a] for a in NAMES)                                  # (a pipeline's own limit is its depth)
    assert all(ex["bridge", o] and ex[o, "bridge"] for o in NAMES if o != "bridge")
    assert ex["encode", "encode_streams"] and ex["encode_streams", "encode"]
    for p in ("decode_streams", "decode_samples_any", "decode_samples_streams"):
        assert all(ex[p, o] and ex[o, p] for o in DECODE_GROUP if o != p), p
    assert sum(sum(r) for r in RELATION) == 16 + 2 + 18                     # bridge, the encode pair, the decode group: no more


def test_symmetric(table):
    for i, a in enumerate(NAMES):
        for j, b in enumerate(NAMES):
            assert table[a][j] == table[b][i], (a, b)


def test_end_refusals_keep_their_wordings(table_lines):
    """What each pipeline's end() calls a request when none is in flight: three wordings, kept as data beside the names."""
    nouns = dict(ln.split() for ln in table_lines[PL_COUNT + 1:])
    assert nouns == {"encode": "call", "decode": "call", "twin_fetch": "request", "encode_streams": "call", "decode_streams": "call",
                     "decode_samples": "request", "decode_samples_any": "request", "decode_samples_streams": "request",
                     "bridge": "tick"}


def test_staging_layout_program_under_sanitizers(tmp_path):
    """tests/host_staging/host_staging_test.cc over lyra_amd/csrc/host_staging.h: where the arrays of every pipeline's requests
    lie in the four runs of a staging slot -- no overlap, 256-byte boundaries on the device, the alignments, at least the
    room each family's own buffers had, no more than that plus padding."""
    exe = str(tmp_path / "host_staging_test")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "lyra_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "host_staging", "host_staging_test.cc")], timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_the_one_gap_in_the_decode_group(table):
    absent = {frozenset((a, b)) for a in DECODE_GROUP for b in DECODE_GROUP
              if a != b and not table[a][NAMES.index(b)]}
    assert absent == {frozenset(("decode", "decode_samples"))}
