"""lyra_hip_export_streams / lyra_hip_import_streams on the GPU: a stream that is exported, imported under another id into a
context with another max_streams and another comfort-noise seed, and continued there, produces what it would have produced
had it stayed -- every comparison between two device runs is bit for bit, no row left out.  The moved decoder is also held
against the reference model (RefLyraDecoder with cng_seed = seed of the FIRST context ^ id in the first context) with
test_gpu_lossy_decode.py's Tally / CnReach bounds.  Refusal uses only blobs that tests/test_stream_state_cpu.py shows
validate() rejects.

Stream kind: the contexts of up to 1,024 streams here run on the CU-masked streams the library picks for them, which are
blocking streams with respect to the NULL stream (the 4,096-stream case: hipStreamNonBlocking streams); the case with
streams="plain" runs its small contexts on hipStreamNonBlocking streams too (tests/gpu_plumbing.py make_ctx)."""
import os

import numpy as np
import pytest

import gpu_plumbing
from gpu_plumbing import make_ctx, stream_cases
from receiver_models import Device, Model, _model_packets as _packets
from signals import _gilbert, _speech

pytestmark = pytest.mark.gpu
RATE, BITS, ENC_BYTES = 48000, 120, 15
SEED_A, SEED_B = 0x1234ABCD5EED, 0x0BADC0DE77
R_E1, R_NOISE_D, R_RS_D, R_CNG = 1, 8, 10, 11


def _ctx(max_streams, seed=None, mode="xnnpack", streams=None):
    return make_ctx(max_streams, mode, RATE, seed, streams=streams)


SeededModel = Model   # (oracle, rate, ids, seed): with the comfort-noise seed of a context that is not the default one


def _enc_input(golden_dir, n, T):
    """[T][n][960] int16 at 48 kHz: speech (each 16 kHz sample three times) with stretches of faint noise, so that the DTX
    encoder's estimator meets speech, noise and the changes between them"""
    rng = np.random.default_rng(99)
    x = np.repeat(_speech(golden_dir, n, T, offset=3111), 3, axis=2)
    for s in range(n):
        for a in range(8 + 3 * s, T, 37):
            x[a:a + 14, s] = rng.integers(-40, 41, size=x[a:a + 14, s].shape)
    return x


class Rig:
    """One context driven as a media server drives it: per hop one DTX encode call at 48 kHz and two 10 ms
    decode_samples_dev requests; everything the calls deliver is returned."""

    def __init__(self, ctx, ids):
        import torch
        self.torch, self.ctx = torch, ctx
        self.dev = torch.device("cuda", 0)
        self.set_ids(ids)

    def set_ids(self, ids):
        torch = self.torch
        self.ids = np.asarray(ids, np.int32)
        self.d_ids = torch.from_numpy(self.ids.copy()).to(self.dev)
        self.dec = Device(self.ctx, self.ids, RATE)

    def encode(self, pcm_ext):
        torch, B = self.torch, self.ids.size
        pk = torch.zeros((B, ENC_BYTES), dtype=torch.uint8, device=self.dev)
        nb = torch.zeros(B, dtype=torch.int32, device=self.dev)
        self.ctx.encode_ext_dev(self.d_ids, torch.from_numpy(np.ascontiguousarray(pcm_ext)).to(self.dev), RATE, BITS, pk, nb, dtx=True)
        self.ctx.synchronize()
        return pk.cpu().numpy(), nb.cpu().numpy()

    def decode(self, rows, nbytes):
        return self.dec.call(rows, nbytes, RATE // 100)


def _same(where, a, b):
    gpu_plumbing._same(a, b, where, names=None)


def _loss_script(T1, T2, n, size):
    """per 10 ms call [2 (T1 + T2) + 1][n] packet sizes (0 = none): a Gilbert chain per stream, packets on the even or the odd
    call of their hop.  The cut comes after call 2 T1, an ODD number of requests, so streams in steady reception are inside a
    generative hop; before it stream 0 loses 12 hops in a row (comfort noise), stream 1 six (in the middle of the fade), and
    stream 2 is handed four packets in the last four calls (two feature vectors wait at the cut)."""
    T = T1 + T2 + 1
    rx = _gilbert(np.random.default_rng(4711), T, n, p_loss=0.12, p_stay=0.8).astype(bool)
    rx[T1 - 12:T1 + 1, 0] = False
    rx[T1 - 9:T1 - 6, 1] = True
    rx[T1 - 6:T1, 1] = False
    rx[T1 - 4:T1, 2] = True
    calls = np.zeros((2 * T, n), np.int32)
    hop_of = np.repeat(np.arange(T), 2)[:, None].repeat(n, axis=1)    # which hop's packet a call hands over
    for s in range(n):
        calls[(s & 1)::2, s] = np.where(rx[:, s], size[s], 0)
    calls, hop_of = calls[:2 * T - 1], hop_of[:2 * T - 1]
    calls[2 * T1 - 5:2 * T1 + 1, 2] = 0
    for k, c in enumerate(range(2 * T1 - 3, 2 * T1 + 1)):   # stream 2: four packets in the last four calls before the cut
        calls[c, 2] = size[2]
        hop_of[c, 2] = T1 - 3 + k
    return calls, hop_of


@pytest.mark.parametrize("mode,streams", stream_cases(["xnnpack", "builtin_mixed"], plain="xnnpack"))
def test_continuation_in_another_context_under_other_ids(golden_dir, oracle_default, oracle_mixed, mode, streams):
    import torch
    oracle = oracle_default if mode == "xnnpack" else oracle_mixed
    T1, T2, n = 30, 104, 8
    ids_a = [5, 17, 2, 40, 9, 33, 21, 0]
    ids_b = [70, 3, 95, 12, 44, 8, 61, 30]
    rows, size = _packets(oracle, golden_dir, [64, 120, 184, 120, 64, 184, 120, 64], T1 + T2 + 2)
    calls, hop_of = _loss_script(T1, T2, n, size)
    pcm = _enc_input(golden_dir, n, T1 + T2)
    model = SeededModel(oracle, RATE, ids_a, SEED_A)
    a, b = _ctx(64, SEED_A, mode, streams), _ctx(96, SEED_B, mode, streams)
    try:
        ra, rb = Rig(a, ids_a), Rig(b, ids_b)

        def hop(t, rigs):
            outs = [[] for _ in rigs]
            for k, r in enumerate(rigs):
                outs[k].extend(r.encode(pcm[t]))
            for c in ([0] if t == 0 else []) + [2 * t + 1, 2 * t + 2]:
                pk = np.stack([rows[hop_of[c, s], s] for s in range(n)])
                got = [r.decode(pk, calls[c]) for r in rigs]
                model.call(f"{mode} call {c}", ids_a, pk, calls[c], RATE // 100, got[-1])   # (the last rig: B after the cut)
                for k in range(len(rigs)):
                    outs[k].extend(got[k])
            return outs

        for t in range(T1):
            hop(t, [ra])
        # the cut, judged on the reference model
        d = [model.decs[i] for i in ids_a]
        waiting = [len(x.model.q) - (1 if x.model.next > 0 else 0) for x in d]
        assert d[0].is_comfort_noise(), "stream 0 should sit in comfort noise at the cut"
        assert 0 < d[1].fade < 640, ("stream 1 should be in the middle of a fade at the cut", d[1].fade)
        assert waiting[2] == 2, ("stream 2 should hold two waiting vectors at the cut", waiting)
        assert any(x.model.next > 0 for x in d), "some stream should be inside a generative hop at the cut"
        if mode == "xnnpack":      # host forms
            blobs = a.export_streams(ids_a)
            assert blobs.shape == (n, a.stream_blob_bytes())
            b.import_streams(ids_b, blobs)
        else:                      # device forms: the blobs never touch the host
            dev = torch.device("cuda", 0)
            d_blobs = torch.zeros((n, a.stream_blob_bytes()), dtype=torch.uint8, device=dev)
            a.export_streams_dev(ra.d_ids, d_blobs)
            b.import_streams_dev(rb.d_ids, d_blobs)
            assert b.import_errors() == 0
        saw_dtx = saw_pkt = saw_cn = 0
        for t in range(T1, T1 + T2):
            oa, ob = hop(t, [ra, rb])
            _same(f"{mode} hop {t}", oa, ob)     # packets, sizes; per request PCM, is_noise, is_comfort_noise
            saw_dtx += int((ob[1] == 0).sum()); saw_pkt += int((ob[1] > 0).sum()); saw_cn += int(ob[-1].sum() + ob[-4].sum())
        assert saw_dtx > 20 and saw_pkt > 200 and saw_cn > 20, (saw_dtx, saw_pkt, saw_cn)
        assert np.array_equal(a.noise_estimate(np.asarray(ids_a, np.int32), side="decoder"),
                              b.noise_estimate(np.asarray(ids_b, np.int32), side="decoder"))
        assert a.decode_samples_errors() == b.decode_samples_errors()
    finally:
        a.close()
        b.close()
    model.tally.report(f"moved streams vs reference model, {mode}")
    assert model.saw_cn and model.saw_mix and model.saw_back


def _warm(rig, golden_dir, T, n, seed=7, offset=500):
    """T hops of mixed traffic on a rig (DTX encode + lossy 10 ms decode), inputs reproducible from the arguments"""
    pcm = _enc_input(golden_dir, n, T)
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 256, size=(2 * T, n, 23), dtype=np.uint8)     # any bytes are a packet to the decoder
    nb = rng.choice(np.array([0, 8, 15, 23], np.int32), size=(2 * T, n), p=[0.55, 0.15, 0.15, 0.15])
    out = []
    for t in range(T):
        o = list(rig.encode(pcm[t]))
        for c in (2 * t, 2 * t + 1):
            o.extend(rig.decode(rows[c], nb[c]))
        out.append(o)
    return out


def test_fixed_point_and_reset_blobs(golden_dir):
    n = 6
    ids_a, ids_b = [3, 9, 1, 30, 14, 7], [50, 2, 77, 31, 8, 19]
    a, b, c = _ctx(32, SEED_A), _ctx(80, SEED_B), _ctx(32, SEED_A)
    try:
        fresh_a, fresh_b = a.export_streams(np.arange(32)), b.export_streams([0, 79, 41])
        assert all(np.array_equal(x[256:], fresh_a[0, 256:]) for x in list(fresh_a) + list(fresh_b)), "reset payloads differ"
        # headers: equal up to the source id and the key, which is seed ^ id
        for i, x in enumerate(fresh_a):
            assert int(x[24:28].view("<i4")[0]) == i and int(x[32:40].view("<u8")[0]) == SEED_A ^ i
            y = x.copy(); y[24:28] = 0; y[32:40] = 0
            z = fresh_a[0].copy(); z[24:28] = 0; z[32:40] = 0
            assert np.array_equal(y, z)
        ra, rb, rc = Rig(a, ids_a), Rig(b, ids_b), Rig(c, ids_a)
        _warm(ra, golden_dir, 14, n)
        _warm(rc, golden_dir, 14, n)
        e1 = a.export_streams(ids_a)
        assert not np.array_equal(e1[0, 256:], fresh_a[0, 256:])
        b.import_streams(ids_b, e1)
        e2 = b.export_streams(ids_b)
        assert np.array_equal(e1[:, 32:], e2[:, 32:]), "export -> import -> export changed key or payload"
        assert np.array_equal(e1[:, :24], e2[:, :24]) and np.array_equal(e2[:, 24:28].view("<i4").ravel(), np.asarray(ids_b))
        a.import_streams(ids_a, e2)     # and back, onto itself
        assert np.array_equal(a.export_streams(ids_a), e1)
        # importing a reset blob is a reset: contexts a (the streams' own blobs from before they ran) and c (lyra_hip_reset_streams)
        a.import_streams(ids_a[:3], fresh_a[ids_a[:3]])
        c.reset(ids_a[:3])
        for t, (x, y) in enumerate(zip(_warm(ra, golden_dir, 12, n, seed=8), _warm(rc, golden_dir, 12, n, seed=8))):
            _same(f"after reset, hop {t}", x, y)
    finally:
        for x in (a, b, c):
            x.close()


def test_isolation_swap_and_sides(golden_dir):
    n = 8
    ids = [4, 11, 6, 20, 1, 15, 9, 2]
    a, c = _ctx(24, SEED_A), _ctx(24, SEED_A)
    try:
        ra, rc = Rig(a, ids), Rig(c, ids)
        _warm(ra, golden_dir, 12, n)
        _warm(rc, golden_dir, 12, n)
        # swap ids 11 and 20 (rows 1 and 3) inside a, through blobs
        two = a.export_streams([11, 20])
        a.import_streams([20, 11], two)
        swapped = [0, 3, 2, 1, 4, 5, 6, 7]
        ra.set_ids([ids[k] for k in swapped])      # row r of a now carries the stream that row r of c carries
        for t, (x, y) in enumerate(zip(_warm(ra, golden_dir, 10, n, seed=21), _warm(rc, golden_dir, 10, n, seed=21))):
            _same(f"after the swap, hop {t}", x, y)
        # sides: the encoder side of row 0's stream goes to a reset state, its decoder side stays; then the other way for row 4
        fresh = a.export_streams([23])
        from lyra_amd import codec
        a.import_streams([ra.ids[0]], fresh, sides=codec.STATE_ENCODER)
        a.import_streams([ra.ids[4]], fresh, sides=codec.STATE_DECODER)
        xs, ys = _warm(ra, golden_dir, 10, n, seed=22), _warm(rc, golden_dir, 10, n, seed=22)
        enc_differs = dec_differs = False
        for t, (x, y) in enumerate(zip(xs, ys)):
            keep = np.ones(n, bool); keep[[0, 4]] = False
            _same(f"sides, other rows, hop {t}", [v[keep] for v in x], [v[keep] for v in y])
            _same(f"sides = ENCODER, decoder output of the target, hop {t}", [v[0:1] for v in x[2:]], [v[0:1] for v in y[2:]])
            _same(f"sides = DECODER, encoder output of the target, hop {t}", [v[4:5] for v in x[:2]], [v[4:5] for v in y[:2]])
            enc_differs |= not np.array_equal(x[0][0], y[0][0]) or x[1][0] != y[1][0]
            dec_differs |= not np.array_equal(x[2][4], y[2][4])
        assert enc_differs and dec_differs, "the imported sides should have changed their own outputs"
    finally:
        a.close()
        c.close()


def test_scale_4096_streams_permuted(golden_dir):
    import torch
    B, steps = 4096, 20
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(31)
    a, c = _ctx(B, SEED_A), _ctx(B, SEED_A)
    try:
        sp = np.load(os.path.join(golden_dir, "sample_wavs.npz"))["sample1_16kHz"].astype(np.int16)
        start = rng.integers(0, sp.size - 2 * steps * 320, size=B)
        ring = np.stack([sp[start[:, None] + t * 320 + np.arange(320)[None]] for t in range(2 * steps)])   # [2 steps][B][320]
        d_ring = torch.from_numpy(ring).to(dev)
        ident = torch.arange(B, dtype=torch.int32, device=dev)

        def run(ctx, d_ids, first):
            pk = [torch.zeros((B, 15), dtype=torch.uint8, device=dev) for _ in range(2)]
            out = [torch.zeros((B, 320), dtype=torch.int16, device=dev) for _ in range(2)]
            got = []
            for t in range(steps):      # one step per call so that every step's rows are compared
                ctx.run_steps_dev(d_ids, BITS, 1, first_step=first + t, d_pcm_ring=d_ring, d_packets=pk, d_pcm_out=out)
                ctx.synchronize()
                k = (first + t) & 1
                got.append((pk[k].cpu().numpy().copy(), out[k].cpu().numpy().copy()))
            return got

        run(a, ident, 0)
        run(c, ident, 0)
        perm = rng.permutation(B).astype(np.int32)
        d_perm = torch.from_numpy(perm).to(dev)
        d_blobs = torch.zeros((B, a.stream_blob_bytes()), dtype=torch.uint8, device=dev)
        a.export_streams_dev(ident, d_blobs)          # row r = stream r ...
        a.import_streams_dev(d_perm, d_blobs)         # ... continues as stream perm[r]
        assert a.import_errors() == 0
        for t, (x, y) in enumerate(zip(run(a, d_perm, steps), run(c, ident, steps))):
            _same(f"step {t}", x, y)
    finally:
        a.close()
        c.close()


def _bad_blobs(good, layout):
    """blobs the CPU test shows validate() rejects, from a good one: wrong magic, version, fingerprint, mode; phase, decimator
    position, estimator counter, loss control word and DsState integers out of domain"""
    import struct
    reg = layout["pieces"]

    def put(b, off, v):
        b[off:off + 4] = np.frombuffer(struct.pack("<I", v & 0xFFFFFFFF), np.uint8)
    out = []
    for name in ("magic", "version", "fingerprint", "mode"):
        b = good.copy(); b[layout["h"][name]] ^= 1; out.append(b)
    for off, v in ((reg[R_E1][0] + layout["phase"], 18), (reg[R_RS_D][0] + layout["rs_in_pos"], -1),
                   (reg[R_NOISE_D][0] + layout["n_hops"], 150), (reg[R_CNG][0] + layout["lossy_ctl"], 5),
                   (reg[R_CNG][0] + layout["ds_state"] + 12, 320), (reg[R_CNG][0] + layout["ds_state"] + 24, 4),
                   (reg[R_CNG][0] + layout["ds_state"] + 4, 641)):
        b = good.copy(); put(b, off, v); out.append(b)
    return np.stack(out)


def test_refusal(golden_dir, tmp_path_factory):
    import json
    import subprocess
    import torch
    import lyra_amd
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    exe = str(tmp_path_factory.mktemp("blob_tool") / "blob_tool")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(root, "lyra_amd", "csrc"),
                           os.path.join(root, "tests", "stream_state", "blob_tool.cc"), "-o", exe])
    layout = json.loads(subprocess.check_output([exe, "layout"]))
    n = 16
    ids = list(range(3, 3 + n))
    dev = torch.device("cuda", 0)
    a, c, src = _ctx(32, SEED_A), _ctx(32, SEED_A), _ctx(48, SEED_B)
    try:
        ra, rc, rs = Rig(a, ids), Rig(c, ids), Rig(src, ids)
        _warm(ra, golden_dir, 10, n)
        _warm(rc, golden_dir, 10, n)
        _warm(rs, golden_dir, 10, n, seed=77)
        blobs = src.export_streams(ids)               # good blobs of streams with a different history
        bad = _bad_blobs(blobs[0], layout)
        path = str(tmp_path_factory.mktemp("blobs") / "bad.bin")
        bad.tofile(path)
        verdicts = [int(v) for v in subprocess.check_output([exe, "validate", path, "2"]).split()]
        assert len(verdicts) == len(bad) == 11 and all(verdicts), verdicts      # validate() rejects every one of them
        call = blobs.copy()
        bad_rows = [0, 2, 3, 5, 7, 8, 10, 11, 12, 14, 15]
        call[bad_rows] = bad
        good_rows = [r for r in range(n) if r not in bad_rows]
        # the host form refuses the whole call and changes nothing
        with pytest.raises(lyra_amd.LyraHipError):
            a.import_streams(ids, call)
        assert a.L.lyra_hip_import_streams(a.h, np.asarray(ids, np.int32).ctypes.data, n, call.ctypes.data, 3) == -1
        before = a.export_streams(ids)
        assert np.array_equal(before[:, 256:], c.export_streams(ids)[:, 256:])
        # the device form skips exactly the bad rows, counts them and imports the others
        d_call = torch.from_numpy(call).to(dev)
        a.import_streams_dev(ra.d_ids, d_call)
        assert a.import_errors() == len(bad_rows)
        assert a.import_errors(clear=True) == len(bad_rows) and a.import_errors() == 0
        after = a.export_streams(ids)
        assert np.array_equal(after[bad_rows], before[bad_rows])
        assert np.array_equal(after[good_rows][:, 32:], blobs[good_rows][:, 32:])
        c.import_streams([ids[r] for r in good_rows], blobs[good_rows])           # the control takes the good rows only
        for t, (x, y) in enumerate(zip(_warm(ra, golden_dir, 10, n, seed=5), _warm(rc, golden_dir, 10, n, seed=5))):
            _same(f"after the refused rows, hop {t}", x, y)
        # a pipelined request is outstanding: refused
        i32 = np.asarray(ids, np.int32)
        a.encode_begin(np.zeros((n, 320), np.int16), BITS, ids)
        out = np.zeros((n, a.stream_blob_bytes()), np.uint8)
        assert a.L.lyra_hip_export_streams(a.h, i32.ctypes.data, n, out.ctypes.data) == -1
        assert a.L.lyra_hip_import_streams(a.h, i32.ctypes.data, n, blobs.ctypes.data, 3) == -1
        assert a.L.lyra_hip_export_streams_dev(a.h, ra.d_ids.data_ptr(), n, d_call.data_ptr()) == -1
        assert a.L.lyra_hip_import_streams_dev(a.h, ra.d_ids.data_ptr(), n, d_call.data_ptr(), 3) == -1
        assert "outstanding" in a.last_error()
        a.encode_end()
        assert a.L.lyra_hip_export_streams(a.h, i32.ctypes.data, n, out.ctypes.data) == 0
    finally:
        for x in (a, c, src):
            x.close()


@pytest.mark.parametrize("rate", [48000, 16000])
def test_classes_move_streams_between_objects(rate):
    """lyra_amd/stream_state_demo: streams moved mid-session between two DeviceLyraDecoder objects (10 ms requests, loss, one in
    comfort noise, staged packets travelling along) and between two BatchLyraEncoder objects with DTX continue as on objects
    that never moved; the sequence that depends on the rebuilt host mirror (a second packet before the next request, then a
    full FIFO) behaves the same; blobs of the other class or rate and calls with requests in flight are refused.  The program
    compares bit for bit and exits non-zero at the first difference."""
    import subprocess
    import lyra_amd
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    r = subprocess.run([os.path.join(root, "lyra_amd", "stream_state_demo"), lyra_amd.default_model_dir(), str(rate)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == 4 and lines[0].startswith("decoders: 6 streams moved") and lines[1].startswith("host mirror:")
    assert lines[2].startswith("encoders: 6 streams moved") and lines[3].startswith("refusals:")
