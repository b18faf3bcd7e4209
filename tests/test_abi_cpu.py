"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/lyra_hip.h declares, refuses to run without a GPU (no CPU fallback), and the host logic of the
Python plugin mirror follows the reference's validation rules.  No compute calls here."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from abi_loading import load_library

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def lib():
    return load_library(raw=True)


def test_exports_match_header(lib):
    hdr = open(os.path.join(ROOT, "include", "lyra_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(lyra_hip_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/lyra_hip.h but not exported"


def _header_prototypes():
    """name -> (return type, [parameter types]) of every lyra_hip_* prototype of include/lyra_hip.h, names and `const` dropped"""
    hdr = open(os.path.join(ROOT, "include", "lyra_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    hdr = re.sub(r"^[ \t]*#[^\n]*", "", hdr, flags=re.M)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(lyra_hip_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
        def ctype(decl, named):
            if "*" in decl:
                return decl[:decl.rindex("*") + 1].replace("const", "").replace(" ", "")
            words = [w for w in decl.split() if w != "const"]
            return " ".join(words[:-1] if named else words)
        assert name not in protos, name
        params = [p.strip() for p in params.split(",")]
        protos[name] = (ctype(" ".join(ret.split()), False), [] if params == ["void"] else [ctype(p, True) for p in params])
    return protos


def test_signature_table_matches_header():
    """Every entry of lyra_amd.codec's signature table against its prototype: declared, same arity, pointers where the header
    has pointers and nowhere else, scalars and return types of the header's width and signedness.  A hand-kept argtypes
    list that drifts from the header corrupts memory silently."""
    from lyra_amd import codec
    protos = _header_prototypes()
    assert len(protos) == 98

    def is_pointer(t):
        return t in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(t, type) and issubclass(t, ctypes._Pointer))
    scalars = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "long": ctypes.c_long, "size_t": ctypes.c_size_t}
    compared = 0
    for name, (restype, argtypes) in codec._SIGNATURES.items():
        assert name in protos, f"{name} is not declared in include/lyra_hip.h"
        ret, params = protos[name]
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        for i, (have, want) in enumerate(zip(argtypes, params)):
            if want.endswith("*"):
                assert is_pointer(have), (name, i, want, have)
            elif want == "uint64_t":
                assert not is_pointer(have) and ctypes.sizeof(have) == 8 and have(-1).value > 0, (name, i, have)
            else:
                assert have is scalars[want], (name, i, want, have)
        if ret == "char*":
            assert restype is ctypes.c_char_p, name
        elif ret == "void*":
            assert restype is ctypes.c_void_p, name
        elif ret != "void":
            assert restype is scalars[ret], (name, ret, restype)
        compared += 1
    assert compared == len(codec._SIGNATURES) == 88


def test_load_refuses_a_library_without_a_listed_symbol(tmp_path, monkeypatch):
    """A library that lacks a function of the signature table is refused at load, with the function's name."""
    import lyra_amd
    from lyra_amd import codec
    src, so = tmp_path / "one.c", tmp_path / "libone.so"
    src.write_text("int lyra_hip_create(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)])
    monkeypatch.setattr(codec, "_libs", {})
    with pytest.raises(lyra_amd.LyraHipError, match=r"libone\.so does not export lyra_hip_\w+"):
        codec._load(str(so))


def test_no_cpu_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import lyra_amd
    h = ctypes.c_void_p()
    lib.lyra_hip_create.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(ctypes.c_void_p)]
    rc = lib.lyra_hip_create(lyra_amd.default_model_dir().encode(), 0, 16, 0, ctypes.byref(h))
    assert rc == -2 and not h.value  # LYRA_HIP_ENODEV
    lib.lyra_hip_last_error.restype = ctypes.c_char_p
    assert b"no CPU path" in lib.lyra_hip_last_error(None)
    with pytest.raises(lyra_amd.LyraHipError):
        lyra_amd.LyraHip()


def test_create_refuses_more_streams_than_32_bit_state_offsets_hold(lib):
    """The kernels address a stream's state as id * region bytes in 32 bits: a context of more streams than that is refused at
    creation (with or without a GPU -- the check comes first), not left to wrap around."""
    import lyra_amd
    h = ctypes.c_void_p()
    lib.lyra_hip_create.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(ctypes.c_void_p)]
    lib.lyra_hip_last_error.restype = ctypes.c_char_p
    rc = lib.lyra_hip_create(lyra_amd.default_model_dir().encode(), 0, 300000, 0, ctypes.byref(h))
    assert rc == -1 and not h.value, rc          # LYRA_HIP_EINVAL
    msg = lib.lyra_hip_last_error(None)
    assert b"at most" in msg and b"289262" in msg, msg


def test_product_does_not_touch_the_oracle():
    """The product path must not import, link or call anything under oracle/."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "lyra_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp")) or f == "Makefile":
                src = open(os.path.join(dirpath, f)).read()
                # (comments may cite the oracle; code must not include, import, link or dlopen it)
                for pat in (r'#include\s*[<"][^>"]*oracle', r"^\s*(from|import)\s+oracle", r"liblyra_oracle",
                            r"dlopen", r"-l\s*lyra_oracle"):
                    assert not re.search(pat, src, flags=re.M), (f, pat)
    out = subprocess.run(["ldd", os.path.join(ROOT, "lyra_amd", "liblyra_hip.so")], capture_output=True, text=True)
    assert "oracle" not in out.stdout


def test_state_layout_constant(lib):
    lib.lyra_hip_state_bytes_per_stream.restype = ctypes.c_size_t
    n = lib.lyra_hip_state_bytes_per_stream()
    # codec state 64.8 KB (int8 histories as int8) + two NoiseEstimator slots of 4 KB + two resampler slots +
    # the comfort-noise overlap-add tail (8.3 KB); per-kernel regions, 256-B slots
    assert n % 256 == 0 and 60000 < n < 90000


def test_pack_container_roundtrip(tmp_path):
    """The weight container the library loads is what tools/pack_weights.py writes (format check)."""
    import struct
    path = os.path.join(ROOT, "lyra_amd", "assets", "lyra_v1.lyrapack")
    blob = open(path, "rb").read()
    assert blob[:8] == b"LYRAPK01"
    n = struct.unpack_from("<I", blob, 8)[0]
    names = {}
    for i in range(n):
        name, dtype, ndim, s0, s1, s2, s3, off, nb = struct.unpack_from("<56sII4IQQ", blob, 16 + 96 * i)
        names[name.rstrip(b"\0").decode()] = (dtype, (s0, s1, s2, s3)[:ndim], off, nb)
        assert off % 64 == 0 and off + nb <= len(blob)
    assert names["rvq.codebooks"][1] == (46, 16, 64)
    assert names["enc.conv.0.w"][1] == (64, 64, 1) and names["dec.tconv.7.w"][1] == (1, 64, 64)
    ver = np.frombuffer(blob, np.int32, 1, names["meta.version"][2])[0]
    assert ver == 3  # lyra_config.binarypb identifier == kVersionMinor (lyra_config.h:145-166)


def test_python_plugin_validation_rules():
    """Argument validation that never reaches the device (residual_vector_quantizer.cc:79-89,116-126;
    generative_model_interface.h:50-101)."""
    import lyra_amd

    class Boom:
        def __getattr__(self, k):
            raise AssertionError("device path must not be reached")
    q = lyra_amd.ResidualVectorQuantizer(Boom())
    assert q.Quantize(np.zeros(64), 185) is None
    assert q.Quantize(np.zeros(64), 62) is None
    assert q.DecodeToLossyFeatures("0" * 185) is None
    assert q.DecodeToLossyFeatures("01" * 31) is None
    g = lyra_amd.LyraGanModel(Boom())
    assert g.GenerateSamples(-1) is None
    assert g.GenerateSamples(0).size == 0
    assert g.GenerateSamples(5) is None
    assert g.AddFeatures(np.zeros(63)) is False
    assert g.num_samples_available() == 0
    assert g.AddFeatures(np.zeros(64)) and g.num_samples_available() == 320
    e = lyra_amd.SoundStreamEncoder(Boom())
    assert e.Extract(np.zeros(319, np.int16)) is None
    assert lyra_amd.packet_size(64) == 8 and lyra_amd.packet_size(120) == 15 and lyra_amd.packet_size(184) == 23
    assert lyra_amd.bitrate_to_num_bits(3200) == 64 and lyra_amd.bitrate_to_num_bits(9200) == 184


def test_bench_multi_rank_plumbing_gloo():
    """world_size 2 on CPU (gloo): stream sharding, barrier, max-over-ranks time, summed units."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29517", os.path.join(ROOT, "bench.py"), "--selftest-dist", "--gpus", "2",
           "--steps", "7", "--streams", "4096"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    r = json.loads(line)
    assert r["world"] == 2 and r["units"] == 2 * 4096 * 7 and abs(r["seconds"] - 0.75) < 1e-9
    assert r["per_rank"] == 4096 and r["first_id"] == 0


def test_bench_main_two_ranks_with_stub_context_gloo():
    """bench.main() itself on two CPU ranks (gloo) with a stand-in for the GPU shard: process group, strong-scaling
    shard of config #5, weight-container broadcast from rank 0, barriers around the timed region, max-over-ranks time,
    summed units, rank-0 result line."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29519", os.path.join(ROOT, "bench.py"), "--stub-context", "--gpus", "2",
           "--config", "5", "--steps", "6", "--warmup", "3", "--bcast-weights", "--no-kernel-table", "--no-cpu-baseline",
           "--latency-steps", "0", "--ramp-steps", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line, from rank 0"
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["steps"] == 6 and r["warmup"] == 3 and r["scaling"] == "strong"
    assert r["config"]["streams_per_gpu"] == 16384 and r["config"]["total_streams"] == 32768
    assert r["config"]["num_bits"] == 120
    secs = 6 * 1e-4 * 1.5                      # the slower stub rank (rank 1) defines the time
    assert abs(r["ms_per_step"] - secs / 6 * 1e3) < 1e-6
    assert abs(r["value"] - 32768 * 6 / secs) < 1.0   # whole-job frames / max-over-ranks seconds
    assert r["stub"]["first_id"] == 0 and r["stub"]["calls"]["encdec"] == 3 + 6
    assert r["stub"]["weights_bytes"] == os.path.getsize(os.path.join(ROOT, "lyra_amd", "assets", "lyra_v1.lyrapack"))


def test_bench_default_invocation_spawns_one_rank_per_gpu():
    """`python bench.py --gpus 2` exactly as a driver without a launcher types it: bench.py re-executes itself under
    torch.distributed.run, so the job is two processes with a process group (gloo here, RCCL on the GPU box), not two
    threads of one process.  Stub shard; the latency leg and the kernel-table pass run too (--full)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--stub-context", "--gpus", "2", "--steps", "5", "--warmup", "2",
           "--full", "--no-cpu-baseline", "--latency-steps", "10"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line, from rank 0"
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["ranks"] == 2 and r["scaling"] == "weak"
    assert "self-spawned" in r["config"]["parallelism"] and "2 rank(s)" in r["config"]["parallelism"]
    assert r["config"]["total_streams"] == 2 * 4096
    assert abs(r["value"] - 2 * 4096 * 5 / (5 * 1e-4 * 1.5)) < 1.0
    # warm-up 2 + kernel-table pass 10 + 2 + untimed ramp 64 + timed 5 + latency 10
    assert r["stub"]["calls"]["encdec"] == 2 + 10 + 2 + 64 + 5 + 10 and r["untimed_ramp_steps"] == 64
    lat = r["step_latency_us"]
    assert lat["n"] == 10 and lat["min"] == 100.0 and lat["max"] == 200.0 and lat["p50"] == 100.0 and lat["p99"] == 200.0


def test_bench_eight_ranks_config5_and_default_respawn():
    """The shape the driver's 8-GPU run has: `python bench.py --gpus 8 --config 5` typed without a launcher ->
    eight spawned ranks (gloo here), 4096 streams per rank, one JSON line that carries every rank's own clock and
    self-check next to the max-reduced time (a straggler must be visible), and rank 0's cpu_baseline leg is attempted at any
    world size (skipped here only because the stub has no oracle workload to time: --no-cpu-baseline)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--stub-context", "--gpus", "8", "--config", "5", "--steps", "4",
           "--warmup", "1", "--full", "--no-cpu-baseline", "--latency-steps", "0", "--no-kernel-table", "--ramp-steps", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line, from rank 0"
    r = json.loads(lines[0])
    assert r["n_gpus"] == 8 and r["ranks"] == 8 and r["scaling"] == "strong"
    assert r["config"]["streams_per_gpu"] == 4096 and r["config"]["total_streams"] == 32768 and r["config"]["num_bits"] == 120
    assert "8 rank(s)" in r["config"]["parallelism"] and "self-spawned" in r["config"]["parallelism"]
    # stub rank k reports K * 0.1 ms * (1 + k / 2): the slowest rank defines the job, every rank is listed
    assert r["per_rank_ms_per_step"] == [round(0.1 * (1 + 0.5 * k), 4) for k in range(8)]
    assert abs(r["ms_per_step"] - 0.1 * 4.5) < 1e-6
    assert abs(r["value"] - 32768 * 4 / (4 * 1e-4 * 4.5)) < 1.0
    assert r["verified"] is True and all(p["verified"] for p in r["per_rank"])


def test_bench_force_dist_one_rank_gloo():
    """--force-dist: ONE rank, process group up anyway (gloo here, RCCL on the GPU box -- tests/test_gpu_bench_verify.py):
    the N > 1 code path (rendezvous, weight broadcast, barriers, max / sum reduction, rank gather, teardown) on one rank,
    typed without a launcher."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--stub-context", "--force-dist", "--bcast-weights", "--steps", "5",
           "--warmup", "2", "--no-cpu-baseline", "--latency-steps", "0", "--no-kernel-table", "--ramp-steps", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["n_gpus"] == 1 and r["ranks"] == 1 and "forced at one rank" in r["process_group"]
    assert abs(r["value"] - 4096 * 5 / (5 * 1e-4)) < 1.0
    assert r["stub"]["weights_bytes"] == os.path.getsize(os.path.join(ROOT, "lyra_amd", "assets", "lyra_v1.lyrapack"))


def test_bench_plain_run_is_lean_and_full_run_has_every_leg(tmp_path):
    """A plain run: warm-up, the untimed ramp, the timed steps, the result line -- no kernel table, latency leg,
    self-check or CPU baseline; --full brings them all back.  --dump-outputs writes what the last timed step computed."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--stub-context", "--steps", "5", "--warmup", "2"]
    out = subprocess.run(base + ["--dump-outputs", str(tmp_path / "plain")], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r, k
    assert r["steps"] == 5 and abs(r["ms_per_step"] - 0.1) < 1e-9
    assert r["stub"]["calls"]["encdec"] == 2 + 64 + 5                  # warm-up + untimed ramp + timed, nothing else
    for k in ("kernels", "step_latency_us", "verified", "verify", "cpu_baseline", "cpu_baseline_xnnpack"):
        assert k not in r, k
    d = tmp_path / "plain"
    assert sorted(os.listdir(d)) == ["calls.npy", "step.npy", "stream_ids.npy"]
    ids, step, calls = (np.load(d / f) for f in ("stream_ids.npy", "step.npy", "calls.npy"))
    assert ids.dtype == step.dtype == calls.dtype == np.float32
    assert np.array_equal(ids, np.arange(4096)) and np.all(step == 2 + 64 + 5 - 1)
    assert np.all(calls == [2 + 64 + 5, 0, 0])                        # taken right after the timed region
    out = subprocess.run(base + ["--full", "--no-cpu-baseline", "--latency-steps", "10", "--dump-outputs", str(tmp_path / "full")],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert r["stub"]["calls"]["encdec"] == 2 + 10 + 2 + 64 + 5 + 10 and r["verified"] is True and r["step_latency_us"]["n"] == 10
    assert np.all(np.load(tmp_path / "full" / "calls.npy") == [2 + 10 + 2 + 64 + 5, 0, 0])


def test_bench_dump_outputs_stays_within_its_budget(tmp_path):
    """Over the budget every array keeps the same fixed, seeded sample of streams (rows), written in stream order; the
    same call twice writes the same files."""
    sys.path.insert(0, ROOT)
    import bench
    B = 1000
    arrays = {"pcm_out": (np.arange(B * 320) % 30000 - 15000).astype(np.int16).reshape(B, 320), "packets": np.full((B, 23), 255, np.uint8),
              "big": np.full(B, 1 << 30, np.int64)}
    small = bench.write_outputs(str(tmp_path / "a"), arrays, budget=B * 400 * 4)
    assert small == {"pcm_out.npy": [B, 320], "packets.npy": [B, 23], "big.npy": [B]}
    assert np.load(tmp_path / "a" / "big.npy").dtype == np.float64 and np.load(tmp_path / "a" / "pcm_out.npy").dtype == np.float32
    budget = 200 * 1024
    for sub in ("b", "c"):
        shapes = bench.write_outputs(str(tmp_path / sub), arrays, budget=budget)
    total = sum(os.path.getsize(tmp_path / "b" / f) for f in shapes)
    assert total <= budget and 0 < shapes["pcm_out.npy"][0] < B
    rows = np.load(tmp_path / "b" / "sampled_streams.npy")
    assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0)
    pcm = np.load(tmp_path / "b" / "pcm_out.npy")
    assert np.array_equal(pcm, arrays["pcm_out"][rows.astype(int)].astype(np.float32))
    for f in shapes:
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f)), f


def test_bench_roofline_bookkeeping():
    """Pure functions of bench.py: per-kernel bounds and the whole-step roofline of every leg."""
    sys.path.insert(0, ROOT)
    import bench
    b, t_ns, all_t = bench.kernel_bound("rvq_encode_kernel")
    # sub / mul / add are one flop each: priced at the non-FMA vector rate, not at the FMA peak
    assert b == "valu" and abs(t_ns - (3 * 16 * 64 * 46 + 3 * 64 * 46) / 78.65e12 * 1e9) < 1e-6
    assert bench.kernel_bound("enc_s0_kernel")[0] == "mfma" and bench.kernel_bound("dec_s0_kernel")[0] == "hbm"
    base = bench.step_work("encdec", dict(rate=16000))
    full = bench.step_work("encdec", dict(full_decoder=True, dtx=True, rate=48000))
    assert len(full[0]) == len(base[0]) + 4 and full[3] > base[3] and full[1] == base[1]
    r = bench.step_roofline("encdec", dict(rate=16000), 13.0e6, None)
    assert r["bound"] == "mfma" and abs(r["frac"] - 2 * base[1] * 13.0e6 / 157.3e12) < 1e-3
    # the committed counter tables (profiles/traffic.json, r05_pmc_sq.txt) carry the int8 stages under their mode-suffixed
    # symbols (enc_s2_xn_kernel): the whole-step traffic and issue-time figures must resolve them (they were null once)
    r = bench.step_roofline("encdec", dict(rate=16000), 14.0e6, bench.load_traffic())
    assert r["traffic"] is not None and 1.0 < r["traffic"] / r["moved_bytes_per_frame"] < 1.5
    assert r["issue_time"]["matrix_pipe_us_per_step_at_B4096"] > 100
    assert [bench.dominant_sample_every(k) for k in (20, 1000)] == [4, 31]
    st = bench.latency_stats([1e-4] * 99 + [5e-4])
    assert st["p50"] == 100.0 and st["p99"] == 100.0 and st["max"] == 500.0 and st["n"] == 100


def test_cpp_plugin_layer_host_logic_against_fake_abi(tmp_path):
    """lyra_amd/host/lyra_hip_components.cc (stream slots, call combining, per-call validation) compiled against a CPU
    stand-in for the C ABI (tests/host_stub/fake_lyra_hip.cc): 24 threads x 20 hops x 5 plugin calls, three bit rates.
    Every caller gets its own stream's result, device calls never overlap, and waiting calls were combined."""
    host = os.path.join(ROOT, "lyra_amd", "host")
    stub = os.path.join(ROOT, "tests", "host_stub")
    exe = str(tmp_path / "combiner_test")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I" + host, "-I" + os.path.join(host, "shims"), "-I" + ROOT,
                           "-o", exe, os.path.join(stub, "combiner_test.cc"), os.path.join(host, "lyra_hip_components.cc"),
                           os.path.join(stub, "fake_lyra_hip.cc")])
    r = subprocess.run([exe, "24", "20"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    st = dict(zip(r.stdout.split()[0::2], map(int, r.stdout.split()[1::2])))
    assert st["plugin_calls"] == 24 * 20 * 5 == st["fake_rows"] and st["overlapping"] == 0
    assert st["device_calls"] < st["plugin_calls"] and st["largest_batch"] >= 2, st
    # many more threads than cores: batches of dozens of requests, woken as a tree, leadership handed on, leaders gathering
    # stragglers; the extractor-side and decoder-side kinds run on two contexts (the fake counts overlap per context)
    r = subprocess.run([exe, "160", "8"], capture_output=True, text=True, timeout=300, env=dict(os.environ, FAKE_CALL_US="50"))
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-500:])
    st = dict(zip(r.stdout.split()[0::2], map(int, r.stdout.split()[1::2])))
    assert st["plugin_calls"] == 160 * 8 * 5 == st["fake_rows"] and st["overlapping"] == 0
    assert st["largest_batch"] >= 4 and st["device_calls"] * 2 < st["plugin_calls"], st



def test_call_combiner_under_thread_sanitizer(tmp_path):
    """The same host logic built with -fsanitize=thread (CPU only; the GPU pool has no sanitizer runs): no data race report
    with 24 threads x 20 hops and with 64 threads behind a 50 us device call."""
    host = os.path.join(ROOT, "lyra_amd", "host")
    stub = os.path.join(ROOT, "tests", "host_stub")
    exe = str(tmp_path / "combiner_tsan")
    cc = subprocess.run(["g++", "-O1", "-g", "-fsanitize=thread", "-std=c++17", "-pthread", "-I" + host,
                         "-I" + os.path.join(host, "shims"), "-I" + ROOT, "-o", exe, os.path.join(stub, "combiner_test.cc"),
                         os.path.join(host, "lyra_hip_components.cc"), os.path.join(stub, "fake_lyra_hip.cc")],
                        capture_output=True, text=True)
    if cc.returncode != 0:
        pytest.skip("no ThreadSanitizer runtime for g++ here: " + cc.stderr[-200:])
    for argv, env in ((["24", "20"], {}), (["64", "6"], {"FAKE_CALL_US": "50"})):
        r = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
        assert "ThreadSanitizer" not in r.stderr and "ThreadSanitizer" not in r.stdout, (r.stdout + r.stderr)[-3000:]
        assert r.returncode == 0, (r.returncode, r.stderr[-500:])


def _pack_tool():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "lyra_amd", "csrc"), "../pack_tool"], stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "lyra_amd", "pack_tool")


def test_cxx_tflite_reader_reproduces_the_shipped_container(tmp_path, ref_model_coeffs):
    """lyra_hip_create() accepts the reference's model directory as is (three .tflite + lyra_config.binarypb,
    lyra_components.cc:42-55): its C++ flatbuffer reader (csrc/tflite_pack.cc) must yield, byte for byte, the
    container the repository ships (written by tools/pack_weights.py from the same directory)."""
    out = tmp_path / "cxx.lyrapack"
    subprocess.check_call([_pack_tool(), ref_model_coeffs, str(out)], stdout=subprocess.DEVNULL)
    shipped = open(os.path.join(ROOT, "lyra_amd", "assets", "lyra_v1.lyrapack"), "rb").read()
    assert open(out, "rb").read() == shipped


def test_cxx_tflite_reader_rejects_bad_model_dirs(tmp_path, ref_model_coeffs):
    import shutil
    tool = _pack_tool()
    names = ["soundstream_encoder.tflite", "quantizer.tflite", "lyragan.tflite", "lyra_config.binarypb"]

    def fresh(name):
        d = tmp_path / name
        d.mkdir()
        for n in names:
            shutil.copy(os.path.join(ref_model_coeffs, n), d / n)
        return d

    def run(d):
        return subprocess.run([tool, str(d), str(tmp_path / "o.bin")], capture_output=True, text=True)

    assert run(fresh("ok")).returncode == 0
    d = fresh("missing")
    os.remove(d / "quantizer.tflite")
    r = run(d)
    assert r.returncode == 1 and "quantizer.tflite" in r.stderr
    d = fresh("truncated")
    blob = open(d / "lyragan.tflite", "rb").read()
    open(d / "lyragan.tflite", "wb").write(blob[: len(blob) // 3])
    assert run(d).returncode == 1
    d = fresh("notflatbuffer")
    open(d / "soundstream_encoder.tflite", "wb").write(b"\x00" * 4096)
    assert run(d).returncode == 1
    d = fresh("config")
    open(d / "lyra_config.binarypb", "wb").write(b"\x10\x03")   # wrong field number
    r = run(d)
    assert r.returncode == 1 and "lyra_config.binarypb" in r.stderr
    # a wrong version identifier converts (meta.version = 2) and is rejected later by the model builder
    d = fresh("version")
    open(d / "lyra_config.binarypb", "wb").write(b"\x08\x02")
    assert run(d).returncode == 0


def test_bench_one_rank_has_no_process_group_and_says_so():
    """N = 1 without --force-dist: no torch.distributed process group exists, and the line says that instead of naming a
    backend that never ran (round-5 review, weak #10)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--stub-context", "--steps", "5", "--warmup", "2", "--no-cpu-baseline",
           "--latency-steps", "0", "--no-kernel-table", "--ramp-steps", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert r["n_gpus"] == 1 and r["ranks"] == 1 and "process_group" not in r
    assert "no process group at one rank" in r["config"]["parallelism"] and "RCCL" not in r["config"]["parallelism"]


def test_bench_ranks_confine_themselves_to_their_share_of_the_cpu_quota():
    """--gpus N: every rank takes a disjoint slice of the CPUs the quota is worth (confine_rank_to_cpu_share), rank 0 gets the
    original mask back for the CPU legs, and the line reports the share (round-5 review, item 9)."""
    code = ("import os, sys, json; sys.path.insert(0, %r); import bench\n"
            "full = sorted(os.sched_getaffinity(0)); got = []; quota = bench.usable_cores()\n"
            "for local in range(2):\n"
            "    os.sched_setaffinity(0, full)\n"
            "    r = bench.confine_rank_to_cpu_share(local, 2)\n"
            "    got.append(None if r is None else (r[0] == full, r[1], sorted(os.sched_getaffinity(0))))\n"
            "print(json.dumps(dict(full=full, quota=quota, got=got)))\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    if len(r["full"]) < 4:
        pytest.skip("fewer than 4 CPUs visible")
    per = max(2, r["quota"] // 2)
    a, b = r["got"]
    assert a[0] and b[0] and a[1] == a[2] and b[1] == b[2]            # the mask was applied, the original one is returned
    assert len(a[1]) == per and len(b[1]) == per and not set(a[1]) & set(b[1])
    # ... and through main(): two stub ranks, the share is in the line
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--stub-context", "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--no-cpu-baseline", "--latency-steps", "0", "--no-kernel-table", "--ramp-steps", "0"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["cpus_per_rank"] == per
