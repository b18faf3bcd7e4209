#!/usr/bin/env python3
"""GPU box, -DLYRA_TIMING builds: shader cycles workgroup 0 (thread 0) spends in the conv that closes each fp32 stage
kernel, at B streams (every tile co-resident), per library given on the command line.

    make -C lyra_amd/csrc EXTRA="-DLYRA_TIMING -DLYRA_PFB_ENC_S0=4 ..." ODIR=obj_t4 OUT=../variants/timing_pfb4.so ../variants/timing_pfb4.so
    python tools/closing_conv_timing.py lyra_amd/variants/timing_pfb4.so [more.so ...]

One child process per library (the library is chosen at import).  Stamps (lyra_dev.h LYRA_TSTAMP): enc_s0 4 -> 5 (k10/s5 GEMM),
enc_s1 72 -> 73 (lrelu + carried rows + k4/s2 conv + stores) and 74 -> 75 (its GEMM), dec_s1 53 -> 54 -> 55 (tconv pass 1, rotate +
pass 2), dec_s2 62 -> 64 (lrelu + barrier + tconv GEMM) and 63 -> 64 (its GEMM).  Median of REPS steps after a warm-up.
"""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
REPS = int(os.environ.get("REPS", 9))
PHASES = [("enc_s0 k10s5 gemm", "e", 4, 5), ("enc_s1 tail", "e", 72, 73), ("enc_s1 k4s2 gemm", "e", 74, 75),
          ("dec_s1 tconv pass1", "d", 53, 54), ("dec_s1 rotate+pass2", "d", 54, 55), ("dec_s1 tconv", "d", 53, 55),
          ("dec_s2 tail", "d", 62, 64), ("dec_s2 tconv gemm", "d", 63, 64),
          ("enc_s0 kernel", "e", 0, 6), ("enc_s1 kernel", "e", 70, 73), ("dec_s1 kernel", "d", 50, 55), ("dec_s2 kernel", "d", 60, 64)]


def child(lib):
    os.environ["LYRA_HIP_LIB"] = os.path.abspath(lib)
    sys.path.insert(0, ROOT)
    import numpy as np
    import lyra_amd
    B = int(os.environ.get("B", 4096))
    ctx = lyra_amd.LyraHip(max_streams=B)
    pcm = np.random.default_rng(0).integers(-8000, 8000, size=(B, 320)).astype(np.int16)
    bufs = {"e": (ctypes.c_longlong * 128)(), "d": (ctypes.c_longlong * 128)()}
    fn = {"e": ctx.L.lyra_hip_debug_timing, "d": ctx.L.lyra_hip_debug_timing_d0}
    for f in fn.values():
        f.argtypes = [ctypes.c_void_p]
    rows = []
    for it in range(3 + REPS):
        pk = ctx.encode(pcm, 184)
        ctx.decode(pk, 184)
        if it < 3:
            continue
        t = {}
        for k in fn:
            fn[k](bufs[k])
            t[k] = np.array(bufs[k][:])
        rows.append([int(t[k][b] - t[k][a]) for _, k, a, b in PHASES])
    med = np.median(np.array(rows), axis=0).astype(int)
    lo, hi = np.min(rows, axis=0), np.max(rows, axis=0)
    print("%s  B=%d  median [min..max] shader cycles over %d steps" % (os.path.basename(lib), B, REPS))
    for (name, _, a, b), m, l, h in zip(PHASES, med, lo, hi):
        print("  %-22s %3d->%-3d %8d  [%d..%d]" % (name, a, b, m, l, h))
    ctx.close()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
        sys.exit(0)
    for lib in sys.argv[1:]:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib], timeout=120)
        if r.returncode != 0:   # nothing more is started on the GPU after a failure
            print("FAILED (%d): %s -- stopping" % (r.returncode, lib))
            sys.exit(1)
