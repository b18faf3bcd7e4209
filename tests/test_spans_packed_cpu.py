"""CPU: what the packed span calls rest on (include/lyra_hip_spans_packed.h; DESIGN.md 4.5 "Packed external-rate layout").

1. The header, the ctypes table of lyra_amd/codec.py (_SIGNATURES_SPANS_PACKED) and the built library agree on the seven symbols.
2. lyra_hip_spans_packed_layout and codec.spans_packed_layout on the layout of the GPU tests.
3. The any-rate file functions of lyra_amd/host/lyra_file_codec.h over a fake C ABI: tests/host_stub/fake_lyra_hip_spans_packed.cc
   beside the existing stand-in.  archive_demo's hop-by-hop half needs the mixed classes, whose C calls the stand-ins do not have,
   so the file functions run behind a small main of the test's own (tests/host_stub/any_rate_files_main.cc).  Every .lyra and
   every decoded WAV is what the reference model with the same fake components gives for that file alone, at that file's rate.
4. Weak binding: lyra_file_codec.cc against the old stand-in alone still links, and the new functions fail with a message.
5. The offset check and the layout (lyra_amd/csrc/spans_packed_plan.h) in a stand-alone program under AddressSanitizer and
   UBSan, against their restatement in Python (packed_cases.py) on a few thousand random span lists."""
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from lyra_amd import codec

from abi_loading import _protos, load_library
from packed_cases import HOPS, LAYOUT, LAYOUT_OFFSETS, LAYOUT_TOTAL, _back_to_back, _check_offsets

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HOST = os.path.join(ROOT, "lyra_amd", "host")
STUB = os.path.join(ROOT, "tests", "host_stub")
NEW = {"lyra_hip_encode_spans_packed_dev": 14, "lyra_hip_decode_spans_lossy_packed_dev": 14, "lyra_hip_decode_spans_packed_dev": 12,
       "lyra_hip_encode_spans_packed": 13, "lyra_hip_decode_spans_lossy_packed": 14, "lyra_hip_decode_spans_packed": 12}
LAYOUT_FN = "lyra_hip_spans_packed_layout"


@pytest.fixture(scope="module")
def lib():
    return load_library()


# ---- 1 --------------------------------------------------------------------------------------------------------------------------
def test_header_table_and_library_agree_on_the_seven_symbols(lib):
    protos = _protos("lyra_hip_spans_packed.h")
    assert set(protos) == set(NEW) and set(codec._SIGNATURES_SPANS_PACKED) == set(NEW) | {LAYOUT_FN}
    header = open(os.path.join(ROOT, "include", "lyra_hip_spans_packed.h")).read()
    assert f"long long {LAYOUT_FN}(const lyra_hip_span* spans, int n_spans," in header
    assert '#include "lyra_hip_spans_rates.h"' in header
    for name, n_args in NEW.items():
        args = [a.strip() for a in protos[name].split(",")]
        assert len(args) == n_args, (name, args)
        fn = getattr(lib, name, None)
        assert fn is not None, f"{name} is not exported by {codec.library_path()}"
        restype, argtypes = codec._SIGNATURES_SPANS_PACKED[name]
        assert restype is codec.C.c_int and fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert len(argtypes) == n_args, (name, argtypes)
        for a, t in zip(args, argtypes):   # pointers as void pointers, the 64-bit length as long long, everything else an int
            assert ("*" in a) == (t is codec.C.c_void_p) and a.startswith("long long ") == (t is codec.C.c_longlong), (name, a, t)
        assert getattr(lib, name)(*[None if t is codec.C.c_void_p else 0 for t in argtypes]) < 0, f"{name}: a null context"
        assert callable(getattr(codec.LyraHip, name[len("lyra_hip_"):], None)), name
    fn = getattr(lib, LAYOUT_FN, None)
    assert fn is not None and fn.restype is codec.C.c_longlong, LAYOUT_FN


# ---- 2 --------------------------------------------------------------------------------------------------------------------------
def test_packed_layout_of_the_seven_spans(lib):
    spans = [(i, 10 * k, n) for k, (i, n, _) in enumerate(LAYOUT)]
    rates = [r for _, _, r in LAYOUT]
    offsets, total = codec.spans_packed_layout(spans, rates)
    assert offsets.tolist() == LAYOUT_OFFSETS == [0, 134400, 134560, 134560, 144160, 145760, 147680]
    assert total == LAYOUT_TOTAL == 167200
    assert _back_to_back([n for _, n, _ in LAYOUT], rates) == (LAYOUT_OFFSETS, LAYOUT_TOTAL)
    sp, rt = codec._spans(spans), np.asarray(rates, np.int32)
    assert lib.lyra_hip_spans_packed_layout(sp.ctypes.data, sp.size, rt.ctypes.data, None) == 167200   # the offsets are optional
    bad = rt.copy()
    bad[4] = 44100
    assert lib.lyra_hip_spans_packed_layout(sp.ctypes.data, sp.size, bad.ctypes.data, None) == -1
    with pytest.raises(codec.LyraHipError):
        codec.spans_packed_layout(spans, bad)
    neg = codec._spans([(0, 0, 5), (1, 5, -1)])
    assert lib.lyra_hip_spans_packed_layout(neg.ctypes.data, 2, rt.ctypes.data, None) == -1
    assert lib.lyra_hip_spans_packed_layout(None, 2, rt.ctypes.data, None) == -1
    assert lib.lyra_hip_spans_packed_layout(sp.ctypes.data, sp.size, None, None) == -1
    assert lib.lyra_hip_spans_packed_layout(None, 0, None, None) == 0


# ---- 3, 4 -------------------------------------------------------------------------------------------------------------------------
def _build_driver(path, with_packed_stub):
    stubs = [os.path.join(STUB, "fake_lyra_hip_codec.cc")] + ([os.path.join(STUB, "fake_lyra_hip_spans_packed.cc")] if with_packed_stub else [])
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + HOST, "-I" + os.path.join(HOST, "shims"), "-I" + ROOT, "-o", path,
                           os.path.join(STUB, "any_rate_files_main.cc"), os.path.join(HOST, "lyra_file_codec.cc"),
                           os.path.join(HOST, "lyra_batch_codec.cc")] + stubs)
    return path


@pytest.fixture(scope="module")
def fake_driver(tmp_path_factory):
    """any_rate_files_main + the file and batch codecs against both stand-ins (no GPU, no product library)"""
    return _build_driver(str(tmp_path_factory.mktemp("any_rate") / "any_rate_fake"), True)


def _write_files(tmp_path, files):
    wavs = []
    for name, (rate, pcm) in files.items():
        with wave.open(str(tmp_path / f"{name}.wav"), "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
            w.writeframes(pcm.tobytes())
        wavs.append(str(tmp_path / f"{name}.wav"))
    return wavs


@pytest.mark.parametrize("bitrate", [3200, 9200])
def test_any_rate_file_functions_against_fake_abi(fake_driver, tmp_path, bitrate):
    sys.path.insert(0, STUB)
    from fake_kit import FakeKit
    from oracle import lyra_codec_model as M
    bits, nbytes = {3200: (64, 8), 6000: (120, 15), 9200: (184, 23)}[bitrate]
    rng = np.random.default_rng(bitrate)
    # (name: encode rate, samples, decode rate): four rates, unequal lengths, tails that are no whole hop, one shorter than a hop
    plan = {"a": (48000, 960 * 17 + 300, 8000), "b": (8000, 160 * 5, 32000), "c": (16000, 320 * 11 - 7, 16000),
            "d": (32000, 640 * 9 + 1, 48000), "tiny": (32000, 639, 8000), "e": (8000, 160 * 23, 16000)}
    files = {k: (rate, rng.integers(-9000, 9000, n).astype(np.int16)) for k, (rate, n, _) in plan.items()}
    wavs = _write_files(tmp_path, files)
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    r = subprocess.run([fake_driver, str(bitrate), str(out_dir), ",".join(str(p[2]) for p in plan.values())] + wavs, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    for name, (rate, pcm) in files.items():
        decode_rate = plan[name][2]
        hop, out_hop = HOPS[rate], HOPS[decode_rate]
        hops = len(pcm) // hop
        enc = np.fromfile(out_dir / f"{name}.lyra", np.uint8)
        with wave.open(str(out_dir / f"{name}_decoded.wav"), "rb") as w:
            assert w.getnchannels() == 1 and w.getframerate() == decode_rate, name
            dec = np.frombuffer(w.readframes(w.getnframes()), np.int16)
        assert enc.size == hops * nbytes and dec.size == hops * out_hop, name
        e = M.RefLyraEncoder(None, rate, bits, False, kit=FakeKit())
        d = M.RefLyraDecoder(None, decode_rate, cng_seed=0, kit=FakeKit())
        for h in range(hops):
            p = e.Encode(pcm[h * hop:(h + 1) * hop])
            assert np.array_equal(enc[h * nbytes:(h + 1) * nbytes], p), (name, h)
            d.SetEncodedPacket(p)
            assert np.array_equal(dec[h * out_hop:(h + 1) * out_hop], d.DecodeSamples(out_hop)), (name, h)


def test_new_file_functions_bind_weakly(tmp_path):
    """Against the old stand-in alone lyra_file_codec.cc still links; the new functions return false and say why."""
    exe = _build_driver(str(tmp_path / "any_rate_old_stub"), False)
    wavs = _write_files(tmp_path, {"x": (48000, np.zeros(960 * 3, np.int16))})
    r = subprocess.run([exe, "6000", str(tmp_path), "16000"] + wavs, capture_output=True, text=True, timeout=60)
    assert r.returncode == 4, (r.returncode, r.stderr[-2000:])
    assert "This build of the lyra_hip library has no packed per-rate span calls" in r.stderr + r.stdout


# ---- 5 --------------------------------------------------------------------------------------------------------------------------
def test_offset_check_and_layout_under_sanitizers_equal_their_restatement(tmp_path):
    exe = str(tmp_path / "spans_packed_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(STUB, "spans_packed_plan_main.cc")])
    rng = np.random.default_rng(2024)
    rates_pool = [8000, 16000, 32000, 48000]
    cases = []
    for k in range(4000):
        n = int(rng.integers(1, 9))
        frames = [int(f) for f in rng.choice([0, 0, 1, 2, 3, 5, 60, 400], n)]
        rates = [int(r) for r in rng.choice(rates_pool, n)]
        good, total = _back_to_back(frames, rates)
        order = rng.permutation(n)
        kind = k % 8
        if kind == 0:     # the back-to-back layout itself, by NULL
            use, offsets, n_ext = 0, [0] * n, total + int(rng.integers(0, 2)) * 8
        else:             # a scattered layout, then one fault (or none)
            use, at, offsets = 1, int(rng.integers(0, 3)) * 8, [0] * n
            for s in order:
                offsets[s] = at
                at += frames[s] * HOPS[rates[s]] + int(rng.integers(0, 3)) * 8
            n_ext = at
            s = int(rng.integers(0, n))
            if kind == 2: offsets[s] = -8 * int(rng.integers(1, 4))
            elif kind == 3: offsets[s] += int(rng.integers(1, 8))
            elif kind == 4: n_ext -= int(rng.integers(1, 200))
            elif kind == 5: offsets[s] = offsets[int(rng.integers(0, n))] + 8 * int(rng.integers(0, 40))
            elif kind == 6: rates[s] = int(rng.choice([0, 44100, 16001, -8000]))
            elif kind == 7: frames[s] = -int(rng.integers(1, 4))
        if k % 97 == 0:
            use, n_ext = 1, -1
        if k % 101 == 0 and frames[0] > 0:   # a base the 32-bit word of the kernel's row cannot carry
            use, offsets, n_ext = 1, [(1 << 34) + 8 * i * 400 * 960 for i in range(n)], (1 << 35)
        cases.append((n_ext, use, frames, rates, offsets))
    text = "".join(f"{len(f)} {n_ext} {use} " + " ".join(f"{a} {b} {c}" for a, b, c in zip(f, r, o)) + "\n"
                   for n_ext, use, f, r, o in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    accepted = 0
    for line, (n_ext, use, frames, rates, offsets) in zip(lines, cases):
        got = [int(v) for v in line.split()]
        b2b = _back_to_back(frames, rates)
        assert got[0] == (b2b[1] if b2b else -1), (line, frames, rates)
        used = offsets if use else (b2b[0] if b2b else None)
        want = used is not None and _check_offsets(frames, rates, used, n_ext)
        assert (got[1] == 0) == want, (line, n_ext, use, frames, rates, offsets)
        if want:
            accepted += 1
            assert got[2:] == list(used), (line, used)
    assert 500 < accepted < len(cases) - 500, accepted
