"""CPU checks of the stream-state blob (lyra_amd/csrc/stream_blob.h, lyra_hip_export_streams / lyra_hip_import_streams):
the layout table, the size, and validate() -- held against domains written down HERE, independently of the header -- plus
the exported symbols and the Python mirror.  The blob-handling program is tests/stream_state/blob_tool.cc, compiled with a
plain C++ compiler."""
import ctypes
import inspect
import json
import os
import subprocess

import numpy as np
import pytest

from abi_loading import load_library
from state_bridge import _reset_blob, _verdicts, compile_tool

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MODE = 2   # LYRA_HIP_REQUANT_XNNPACK
R_E1, R_E2, R_D0, R_D1, R_NOISE_E, R_NOISE_D, R_RS_E, R_RS_D, R_CNG = 1, 2, 3, 4, 7, 8, 9, 10, 11


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return compile_tool(tmp_path_factory.mktemp("blob_tool"))


@pytest.fixture(scope="module")
def L(tool):
    return json.loads(subprocess.check_output([tool, "layout"]))


@pytest.fixture(scope="module")
def lib():
    return load_library(raw=True)


def _region_off(L, r):
    return L["pieces"][r][0]


def checked_words(L):
    """name -> (byte offset in the blob, lowest, highest accepted value as a signed 32-bit integer).  The domains are the
    ones the kernels rely on, restated from the kernels: ring row (phase * T + t) mod R with phase < 18; the estimator's
    flags and its hop counter below the largest hops-per-update (48 kHz: 150); the decimator's first tap from in_pos mod 6;
    DsState as decode_samples_plan.h keeps it."""
    w = {}
    for name, r in (("E1", R_E1), ("E2", R_E2), ("D0", R_D0), ("D1", R_D1)):
        w[f"phase_{name}"] = (_region_off(L, r) + L["phase"], 0, 17)
    for name, r in (("E", R_NOISE_E), ("D", R_NOISE_D)):
        w[f"n_init_{name}"] = (_region_off(L, r) + L["n_init"], 0, 1)
        w[f"n_hops_{name}"] = (_region_off(L, r) + L["n_hops"], 0, 149)
        w[f"n_is_noise_{name}"] = (_region_off(L, r) + L["n_is_noise"], 0, 1)
    for name, r in (("E", R_RS_E), ("D", R_RS_D)):
        w[f"rs_in_pos_{name}"] = (_region_off(L, r) + L["rs_in_pos"], 0, 5)
    ds = _region_off(L, R_CNG) + L["ds_state"]
    for k, (name, lo, hi) in enumerate((("cp", -320, 1280), ("fade", 0, 640), ("to_cng", 0, 1), ("gpos", 0, 319),
                                        ("cpos", 0, 319), ("wait", 0, 4), ("head", 0, 3))):
        w[f"ds_{name}"] = (ds + 4 * k, lo, hi)
    return w


def lossy_ctl_ok(v):
    v &= 0xFFFFFFFF
    return (v & 255) <= 4 and ((v >> 8) & 255) <= 2 and (v >> 17) == 0


def _put(blob, off, v):
    blob[off:off + 4] = np.frombuffer(np.array([v & 0xFFFFFFFF], "<u4").tobytes(), np.uint8)


def test_layout_table_covers_the_payload_exactly_once(L, lib):
    pieces = L["pieces"]
    assert len(pieces) == 12 + 3
    pos = L["header_bytes"]
    for i, (off, n) in enumerate(pieces):
        assert off == pos and n > 0 and off % 16 == 0 and n % 16 == 0, (i, off, n, pos)
        pos += n
    assert pos == L["bytes"]
    assert [n for _, n in pieces[:12]] == L["region_bytes"]
    assert pieces[12][0] == L["ds_off"] == L["header_bytes"] + L["state_bytes"]
    assert [n for _, n in pieces[12:]] == [4 * 64 * 4, 640, 640] and sum(n for _, n in pieces[12:]) == L["section_bytes"]
    assert L["region_side"] == [1, 1, 1, 2, 2, 2, 2, 1, 2, 1, 2, 2]
    lib.lyra_hip_state_bytes_per_stream.restype = ctypes.c_size_t
    lib.lyra_hip_stream_blob_bytes.restype = ctypes.c_size_t
    assert L["bytes"] == 256 + lib.lyra_hip_state_bytes_per_stream() + L["section_bytes"]
    assert L["bytes"] % 256 == 0 and lib.lyra_hip_stream_blob_bytes() == L["bytes"]


def test_slot_key_sits_in_free_bytes_of_the_comfort_noise_slot(L):
    assert L["ds_state"] + 7 * 4 <= L["c_key"] and L["c_key"] % 8 == 0 and L["c_key"] + 8 <= L["c_ola"]


def test_validate_accepts_reset_values_and_rejects_each_header_field(tool, L, tmp_path):
    good = _reset_blob(tool, tmp_path)
    assert good.size == L["bytes"]
    cases, names = [good], ["reset values"]
    for name in ("magic", "version", "bytes", "fingerprint", "mode", "model"):
        b = good.copy()
        b[L["h"][name]] ^= 1
        cases.append(b); names.append(name)
    b = good.copy(); _put(b, L["h"]["src_id"], -1); cases.append(b); names.append("src_id")
    b = good.copy(); b[L["h"]["zero"]] = 1; cases.append(b); names.append("zero word")
    for off in (L["h_end"], 100, 255):
        b = good.copy(); b[off] = 1; cases.append(b); names.append(f"header byte {off}")
    b = good.copy(); b[_region_off(L, R_CNG) + L["c_key"] + 3] = 9; cases.append(b); names.append("key word in the payload")
    v = _verdicts(tool, tmp_path, np.stack(cases))
    assert v[0] == 0, v
    for name, x in zip(names[1:], v[1:]):
        assert x != 0, f"{name} changed: accepted"
    assert len(set(v[1:7])) == 6   # each of the six constants has a verdict of its own
    # the key and the source id are the stream's own: any value passes
    b = good.copy(); b[L["h"]["key"]:L["h"]["key"] + 8] = 0xA5; _put(b, L["h"]["src_id"], 123456)
    assert _verdicts(tool, tmp_path, b[None]) == [0]
    # a blob from another requant mode
    assert _verdicts(tool, tmp_path, _reset_blob(tool, tmp_path, mode=3)[None], mode=MODE) != [0]
    assert _verdicts(tool, tmp_path, _reset_blob(tool, tmp_path, mode=3)[None], mode=3) == [0]


def test_validate_rejects_each_listed_integer_just_outside_its_domain(tool, L, tmp_path):
    good = _reset_blob(tool, tmp_path)
    cases, names, want = [], [], []
    for name, (off, lo, hi) in checked_words(L).items():
        for v, ok in ((lo, True), (hi, True), (lo - 1, False), (hi + 1, False), (-2 ** 31, False), (2 ** 31 - 1, False)):
            b = good.copy(); _put(b, off, v)
            cases.append(b); names.append(f"{name} = {v}"); want.append(ok)
    ctl = _region_off(L, R_CNG) + L["lossy_ctl"]
    for v in (0, 4, 2 << 8, 1 << 16, 4 | (2 << 8) | (1 << 16), 5, 3 << 8, 1 << 17, 1 << 24, 0xFFFFFFFF):
        b = good.copy(); _put(b, ctl, v)
        cases.append(b); names.append(f"lossy_ctl = {v:#x}"); want.append(lossy_ctl_ok(v))
    got = _verdicts(tool, tmp_path, np.stack(cases))
    for name, g, ok in zip(names, got, want):
        assert (g == 0) == ok, f"{name}: verdict {g}"


def test_random_corruptions_never_pass_with_a_value_out_of_domain(tool, L, tmp_path):
    good = _reset_blob(tool, tmp_path)
    words = checked_words(L)
    ctl = _region_off(L, R_CNG) + L["lossy_ctl"]
    rng = np.random.default_rng(20240607)
    N = 6000
    blobs = np.repeat(good[None], N, axis=0)
    in_domain = np.ones(N, bool)
    keys = list(words)
    for i in range(N):
        for _ in range(int(rng.integers(1, 4))):
            k = int(rng.integers(0, len(keys) + 1))
            kind = int(rng.integers(0, 3))
            if k == len(keys):
                v = int(rng.integers(0, 2 ** 32)) if kind == 0 else int(rng.integers(0, 8)) | (int(rng.integers(0, 4)) << 8) | \
                    (int(rng.integers(0, 2)) << 16) | (int(rng.integers(0, 2) * rng.integers(0, 2)) << int(rng.integers(17, 32)))
                _put(blobs[i], ctl, v)
                continue
            off, lo, hi = words[keys[k]]
            v = int(rng.integers(-2 ** 31, 2 ** 31)) if kind == 0 else int(rng.integers(lo - 3, hi + 4)) if kind == 1 else \
                int(rng.choice([lo - 1, hi + 1, lo, hi, -1, 256 + lo, 65536 + hi]))
            _put(blobs[i], off, v)
        for off, lo, hi in words.values():
            v = int(np.frombuffer(blobs[i, off:off + 4].tobytes(), "<i4")[0])
            in_domain[i] &= lo <= v <= hi
        in_domain[i] &= lossy_ctl_ok(int(np.frombuffer(blobs[i, ctl:ctl + 4].tobytes(), "<u4")[0]))
    got = np.array(_verdicts(tool, tmp_path, blobs)) == 0
    assert 200 < in_domain.sum() < N - 200, in_domain.sum()       # both outcomes are well represented
    assert not (got & ~in_domain).any(), "validate accepted a blob with an out-of-domain value"
    assert np.array_equal(got, in_domain)                          # ... and refuses nothing that is inside


def test_library_exports_the_calls_and_refuses_a_null_context(lib):
    vp, ci = ctypes.c_void_p, ctypes.c_int
    buf = (ctypes.c_uint8 * 16)()
    ids = (ctypes.c_int32 * 1)(0)
    for suf in ("", "_dev"):
        e, i = getattr(lib, "lyra_hip_export_streams" + suf), getattr(lib, "lyra_hip_import_streams" + suf)
        e.argtypes = [vp, vp, ci, vp]
        i.argtypes = [vp, vp, ci, vp, ctypes.c_uint]
        assert e(None, ids, 1, buf) == -1      # LYRA_HIP_EINVAL
        assert i(None, ids, 1, buf, 3) == -1
    lib.lyra_hip_import_errors.argtypes = [vp, ci]
    lib.lyra_hip_import_errors.restype = ctypes.c_long
    assert lib.lyra_hip_import_errors(None, 0) == -1
    hdr = open(os.path.join(ROOT, "include", "lyra_hip.h")).read()
    assert "#define LYRA_HIP_STATE_ENCODER 1u" in hdr and "#define LYRA_HIP_STATE_DECODER 2u" in hdr


def test_python_mirror_signatures():
    import lyra_amd
    from lyra_amd import codec
    want = {"stream_blob_bytes": [], "export_streams": ["stream_ids"], "import_streams": ["stream_ids", "blobs", "sides"],
            "export_streams_dev": ["d_ids", "d_blobs"], "import_streams_dev": ["d_ids", "d_blobs", "sides"],
            "import_errors": ["clear"]}
    for name, params in want.items():
        sig = inspect.signature(getattr(lyra_amd.LyraHip, name))
        assert list(sig.parameters)[1:] == params, (name, sig)
    assert inspect.signature(lyra_amd.LyraHip.import_streams).parameters["sides"].default == 3
    assert (codec.STATE_ENCODER, codec.STATE_DECODER, codec.STATE_BOTH) == (1, 2, 3)
    L = codec._load()
    assert L.lyra_hip_stream_blob_bytes.restype is ctypes.c_size_t
    assert L.lyra_hip_import_errors.restype is ctypes.c_long
    for suf in ("", "_dev"):
        assert len(getattr(L, "lyra_hip_export_streams" + suf).argtypes) == 4
        assert len(getattr(L, "lyra_hip_import_streams" + suf).argtypes) == 5


def test_class_blobs_against_a_fake_abi(tmp_path):
    """lyra_amd/host/lyra_stream_state.cc with the two classes' own translation units, linked against the fake C ABI of
    tests/host_stub (unchanged) plus tests/stream_state/fake_stream_abi.cc: class header round trip, the rebuilt host mirror,
    the dropped staged packet, and the refusals (kind, rate, size, index, requests in flight)."""
    host = os.path.join(ROOT, "lyra_amd", "host")
    exe = str(tmp_path / "class_blob_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + host, "-I" + os.path.join(host, "shims"), "-I" + ROOT,
                           "-o", exe, os.path.join(ROOT, "tests", "stream_state", "class_blob_test.cc"),
                           os.path.join(ROOT, "tests", "stream_state", "fake_stream_abi.cc"),
                           os.path.join(host, "lyra_stream_state.cc"), os.path.join(host, "lyra_batch_codec.cc"),
                           os.path.join(host, "lyra_device_decoder.cc"),
                           os.path.join(ROOT, "tests", "host_stub", "fake_lyra_hip_codec.cc")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "class blobs ok" in r.stdout, r.stderr[-2000:]
