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
  return 0;
}
'''

NAMES = ["encode", "decode", "twin_fetch", "encode_streams", "decode_streams", "decode_samples", "decode_samples_any",
         "decode_samples_streams", "bridge"]
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
def table(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("pipelines")
    src, exe = d / "pipelines.cc", d / "pipelines"
    src.write_text(_DRIVER)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "lyra_amd", "csrc"), str(src),
                           "-o", str(exe)], timeout=300)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")[:-1]
    count, depth = (int(x) for x in lines[0].split())
    assert count == 9 and depth == 2 and len(lines) == 10
    return {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in lines[1:]}


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


def test_the_one_gap_in_the_decode_group(table):
    absent = {frozenset((a, b)) for a in DECODE_GROUP for b in DECODE_GROUP
              if a != b and not table[a][NAMES.index(b)]}
    assert absent == {frozenset(("decode", "decode_samples"))}
