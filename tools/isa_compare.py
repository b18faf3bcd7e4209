#!/usr/bin/env python3
"""Compare the final ISA of every kernel that exists in two builds.

    make -C lyra_amd/csrc ODIR=obj_asm asm        # on each commit; keep a copy of obj_asm/*.s of the first
    python tools/isa_compare.py PARENT_DIR BRANCH_DIR

A kernel's text is everything between its label and its .Lfunc_end, comments and blank lines dropped; block labels carry
the function's ordinal in the file (.LBB12_3), which moves when a kernel is added in front, so the ordinal is masked.
Exit status 1 when a kernel present in both differs.
"""
import glob
import os
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = line.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = re.match(r"^(_Z\w+|\w+_kernel\w*):\s*$", line)
        if name is None and m:
            name, body = m.group(1), []
            continue
        if name is not None:
            if re.match(r"^\.Lfunc_end\d+:", line):
                out[name] = body
                name = None
                continue
            body.append(re.sub(r"\.LBB\d+_", ".LBB_", line))
    return out


def main():
    a_dir, b_dir = sys.argv[1:3]
    same = differ = only = 0
    for a in sorted(glob.glob(os.path.join(a_dir, "*.s"))):
        b = os.path.join(b_dir, os.path.basename(a))
        if not os.path.exists(b):
            print("missing in second build: %s" % os.path.basename(a))
            differ += 1
            continue
        ka, kb = kernels(a), kernels(b)
        for k in sorted(ka):
            if k not in kb:
                print("only in first: %s" % k)
                differ += 1
            elif ka[k] != kb[k]:
                print("DIFFERS: %s (%s): %d vs %d lines" % (k, os.path.basename(a), len(ka[k]), len(kb[k])))
                differ += 1
            else:
                same += 1
        for k in sorted(kb):
            if k not in ka:
                print("new: %s (%s): %d lines" % (k, os.path.basename(a), len(kb[k])))
                only += 1
    print("%d kernels identical, %d differ or are missing, %d new" % (same, differ, only))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
