"""lyra_hip_decode_samples_dev: LyraDecoder::SetEncodedPacket + DecodeSamples(n) for request sizes that are not tied to the
20 ms hop, with the whole loss state machine on the device.  Expectations: oracle/lyra_codec_model.py's RefLyraDecoder
on the C oracle, stream by stream and call by call, compared with test_gpu_lossy_decode.py's Tally / CnReach -- exact where
only the generative model speaks, within 1 LSB where comfort noise reaches (that file's bounds; none of its own) --
is_noise, is_comfort_noise and the decoder-side noise estimate after every call; and bit for bit against the calls that
already exist where the regimes coincide (lyra_hip_decode_lossy_mixed_dev for n = one hop, lyra_hip_decode_dev when every
packet arrives).

Stream kind: the contexts here (256 streams) run on the CU-masked streams the library picks up to 1,024 streams, which are
blocking streams with respect to the NULL stream; the case with streams="plain" runs on hipStreamNonBlocking streams, the kind
of a 4,096-stream context (tests/gpu_plumbing.py make_ctx)."""
import os

import numpy as np
import pytest

from gpu_plumbing import make_ctx, stream_cases
from receiver_models import DEPTH, Device, Model, _model_packets as _packets
from signals import _patterns, _speech

pytestmark = pytest.mark.gpu


def _ctx(max_streams=256, streams=None):
    return make_ctx(max_streams, streams=streams)


def _ten_ms_calls(mask, phase):
    """hop mask [T][n] -> per 10 ms call (hop index, [n] packet present): stream s gets the packet of hop t in call
    2 t + phase[s]"""
    T, n = mask.shape
    for c in range(2 * T):
        t = c // 2
        yield t, np.array([(c & 1) == phase[s] and bool(mask[t, s]) for s in range(n)])


@pytest.mark.parametrize("rate", [16000, 48000])
def test_ten_ms_receiver_vs_reference_model(golden_dir, oracle_default, rate):
    """10 ms requests, a packet every second call (on the even call for half of the streams, on the odd call for the
    others), the four loss patterns of the hop-synchronous tests at all three bitrates in one batch; every sample, both
    flags and the decoder-side estimate after EVERY call -- the estimate is what tells a comfort-noise hop that read the
    noise estimate on the wrong side of the call's estimator update."""
    T = 36
    bits = [64, 120, 184] * 4
    ids = [5, 17, 2, 40, 9, 33, 21, 0, 63, 12, 48, 7]
    rows, size = _packets(oracle_default, golden_dir, bits, T)
    mask = np.repeat(_patterns(T), 3, axis=1)
    phase = [s & 1 for s in range(12)]
    model = Model(oracle_default, rate, ids)
    ctx = _ctx()
    try:
        devc = Device(ctx, ids, rate)
        for c, (t, has) in enumerate(_ten_ms_calls(mask, phase)):
            nb = np.where(has, size, 0).astype(np.int32)
            got = devc.call(rows[t], nb, rate // 100)
            model.call(f"call {c}", ids, rows[t], nb, rate // 100, got)
            model.check_estimates(ctx, f"call {c}", ids)
        assert ctx.decode_samples_errors() == 0
    finally:
        ctx.close()
    model.tally.report(f"decode_samples 10 ms {rate} Hz")
    assert model.saw_cn and model.saw_mix and model.saw_back


@pytest.mark.parametrize("rate,streams", stream_cases([16000, 48000], plain=48000))
def test_one_hop_requests_equal_lossy_mixed_bit_for_bit(golden_dir, oracle_default, rate, streams):
    """n = one hop, at most one packet per call: the same kernels in the same order as lyra_hip_decode_lossy_mixed_dev on
    a second context with the same seed -- samples (comfort noise included), is_noise, is_comfort_noise, estimates."""
    import torch
    T, hop = 36, rate // 50
    bits = [64, 120, 184] * 4
    ids = [5, 17, 2, 40, 9, 33, 21, 0, 63, 12, 48, 7]
    rows, size = _packets(oracle_default, golden_dir, bits, T, offset=777)
    mask = np.repeat(_patterns(T), 3, axis=1)
    a, b = _ctx(streams=streams), _ctx(streams=streams)
    try:
        devc = Device(a, ids, rate)
        dev = torch.device("cuda", 0)
        d_ids = torch.from_numpy(np.asarray(ids, np.int32)).to(dev)
        saw_cn = saw_back = 0
        was = np.zeros(12, bool)
        for t in range(T):
            nb = np.where(mask[t], size, 0).astype(np.int32)
            pcm, isn, icn = devc.call(rows[t], nb, hop)
            saw_cn += int(icn.sum())
            saw_back += int((was & (icn == 0)).sum())
            was = icn != 0
            pk, dnb = torch.from_numpy(rows[t].copy()).to(dev), torch.from_numpy(nb).to(dev)
            o16 = torch.zeros((12, 320), dtype=torch.int16, device=dev)
            oext = torch.zeros((12, hop), dtype=torch.int16, device=dev)
            f1, f2 = torch.zeros(12, dtype=torch.int32, device=dev), torch.zeros(12, dtype=torch.int32, device=dev)
            b.decode_lossy_mixed_dev(d_ids, pk, dnb, rate, o16, oext if rate != 16000 else None, f1, f2)
            b.synchronize()
            want = (oext if rate != 16000 else o16).cpu().numpy()
            assert np.array_equal(pcm, want), f"tick {t}"
            assert np.array_equal(isn, f1.cpu().numpy()) and np.array_equal(icn, f2.cpu().numpy()), f"tick {t}"
        assert np.array_equal(a.noise_estimate(np.asarray(ids, np.int32), side="decoder"),
                              b.noise_estimate(np.asarray(ids, np.int32), side="decoder"))
        assert saw_cn >= 3 and saw_back >= 3    # pure comfort noise was reached and left again inside the compared run
    finally:
        a.close()
        b.close()


def test_two_ten_ms_requests_equal_decode_dev(golden_dir, oracle_default):
    """Every packet received, 10 ms requests at 16 kHz: two calls concatenated are lyra_hip_decode_dev's hop bit for bit."""
    import torch
    T, n, bits = 12, 9, 120
    rows, size = _packets(oracle_default, golden_dir, [bits] * n, T, offset=4242)
    ids = [3, 1, 4, 15, 9, 2, 6, 5, 35]
    a, b = _ctx(), _ctx()
    try:
        devc = Device(a, ids, 16000)
        dev = torch.device("cuda", 0)
        d_ids = torch.from_numpy(np.asarray(ids, np.int32)).to(dev)
        for t in range(T):
            first = devc.call(rows[t], size, 160)[0]
            second = devc.call(rows[t], np.zeros(n, np.int32), 160)[0]
            pk = torch.from_numpy(np.ascontiguousarray(rows[t, :, :15])).to(dev)
            out = torch.zeros((n, 320), dtype=torch.int16, device=dev)
            b.decode_dev(d_ids, pk, bits, out)
            b.synchronize()
            assert np.array_equal(np.concatenate([first, second], axis=1), out.cpu().numpy()), f"hop {t}"
    finally:
        a.close()
        b.close()


def test_mixed_sizes_late_packets_and_overflow(golden_dir, oracle_default):
    """16 kHz, request sizes that change from call to call (160, 320, 37, 0, 283, ...); packets handed over late, two in
    successive calls, up to the FIFO depth; one stream is sent DEPTH + 2 packets with nothing played in between: two are
    refused, counted, and the stream goes on as the model does when those packets are simply not delivered."""
    sizes = [160, 320, 37, 0, 283, 160, 1, 319, 160, 160, 0, 320, 77, 243, 160]
    T = 40
    bits = [64, 120, 184, 120, 64, 184]
    ids = [11, 3, 60, 27, 8, 19]
    rows, size = _packets(oracle_default, golden_dir, bits, T, offset=99)
    rng = np.random.default_rng(5)
    model = Model(oracle_default, 16000, ids)
    ctx = _ctx()
    try:
        devc = Device(ctx, ids, 16000)
        played, sent, flush = 0, [0] * 6, [False] * 6
        burst = [1, 1, 2, 3, 3, 1]         # stream s holds its packets back until `burst` are due, then hands one over per call
        for c in range(64):
            n = sizes[c % len(sizes)]
            due = played // 320 + 1        # packets the sender has produced by the start of this request
            if c == 30:                    # the overflow: DEPTH + 2 packets for stream 5 in calls of their own with n = 0
                assert model.dropped == 0
                for _ in range(DEPTH + 2):
                    x = np.zeros(6, np.int32)
                    x[5] = size[5]
                    pk = np.stack([rows[sent[s], s] for s in range(6)])
                    model.call(f"call {c} overflow", ids, pk, x, 0, devc.call(pk, x, 0))
                    sent[5] += 1
                assert model.dropped >= 2
            nb = np.zeros(6, np.int32)
            pk = np.stack([rows[sent[s], s] for s in range(6)])
            for s in range(6):
                flush[s] = sent[s] < due and (flush[s] or due - sent[s] >= burst[s])
                if flush[s]:
                    lost = (s == 1 and 8 <= sent[s] < 22) or (s == 4 and rng.random() < 0.3)
                    nb[s] = 0 if lost else size[s]
                    sent[s] += 1
            got = devc.call(pk, nb, n)
            model.call(f"call {c}", ids, pk, nb, n, got)
            model.check_estimates(ctx, f"call {c}", ids)
            played += n
            assert max(sent) < T
        assert model.dropped >= 1
        assert ctx.decode_samples_errors(clear=True) == model.dropped
        bad = np.array([7, 0, 0, 24, 0, -3], np.int32)     # sizes that are no packet size: no packet, counted
        pk = np.stack([rows[0, s] for s in range(6)])
        model.call("bad sizes", ids, pk, bad, 160, devc.call(pk, bad, 160))
        assert ctx.decode_samples_errors() == 3
    finally:
        ctx.close()
    model.tally.report("decode_samples mixed sizes 16 kHz")
    assert model.saw_two and model.saw_cn and model.saw_mix


def test_subsets_shuffled_ids_and_resets(golden_dir, oracle_default):
    """A different subset of the streams in every call, ids in shuffled order, some streams reset mid-run (their model
    decoder starts afresh), 10 ms at 48 kHz."""
    rate, T, n = 48000, 30, 10
    bits = [64, 120, 184, 64, 120, 184, 64, 120, 184, 120]
    all_ids = np.array([50, 3, 41, 18, 7, 29, 36, 12, 0, 63], np.int32)
    rows, size = _packets(oracle_default, golden_dir, bits, T, offset=1234)
    rng = np.random.default_rng(21)
    model = Model(oracle_default, rate, all_ids)
    calls = np.zeros(n, int)               # 10 ms calls every stream has made: its packet of hop k comes with call 2 k
    ctx = _ctx()
    try:
        devc = Device(ctx, all_ids, rate)
        for c in range(2 * T + 20):
            pick = rng.permutation(n)[:int(rng.integers(1, n + 1))]
            pick = pick[calls[pick] < 2 * T]
            if pick.size == 0:
                continue
            if c in (23, 41):
                ctx.synchronize()
                gone = all_ids[[1, 4, 8]] if c == 23 else all_ids[[0]]
                ctx.reset(gone)
                for i in gone:
                    model.reset(int(i))
            devc.set_ids(all_ids[pick])
            hop = calls[pick] // 2
            lost = (hop % 7 == 3) | ((pick == 2) & (hop >= 5) & (hop < 18))
            nb = np.where((calls[pick] % 2 == 0) & ~lost, size[pick], 0).astype(np.int32)
            pk = rows[hop, pick]
            got = devc.call(pk, nb, rate // 100)
            model.call(f"call {c}", all_ids[pick], pk, nb, rate // 100, got)
            model.check_estimates(ctx, f"call {c}", all_ids[pick])
            calls[pick] += 1
        assert ctx.decode_samples_errors() == 0
    finally:
        ctx.close()
    model.tally.report("decode_samples subsets 48 kHz")
    assert model.saw_cn and model.saw_mix


def test_full_batch_vs_reference_model(golden_dir, oracle_default):
    """4096 streams, 40 calls of 10 ms at 16 kHz, none synchronised until its result is read; every row carries the packets
    and the loss pattern of one of 32 modelled streams, and 32 rows spread over the plan kernel's blocks, the tiles of four
    and the logmel pairs are compared with the model after every call."""
    B, T, nm = 4096, 20, 32
    bits = [(64, 120, 184)[s % 3] for s in range(nm)]
    rows, size = _packets(oracle_default, golden_dir, bits, T, offset=31)
    rng = np.random.default_rng(77)
    mask = np.ones((T, nm), bool)
    state = rng.random(nm) < 0.2
    for t in range(T):
        state = np.where(state, rng.random(nm) < 0.6, rng.random(nm) < 0.12)
        mask[t] = ~state
    mask[2:15, 0] = False                  # one run into pure comfort noise and back
    ids = rng.permutation(B).astype(np.int32)
    src = np.arange(B) % nm                # row r plays modelled stream r % 32 ...
    phase = (np.arange(B) // nm) & 1       # ... with its packet on the even or on the odd call
    watch = np.array([0, 1, 2, 3, 37, 255, 256, 257, 511, 1023, 1024, 1500, 2047, 2048, 2049, 2050, 2051, 2600, 3000, 3071,
                      3072, 3333, 3584, 3585, 3839, 3840, 3999, 4000, 4092, 4093, 4094, 4095])
    model = Model(oracle_default, 16000, ids[watch])
    ctx = _ctx(B)
    try:
        devc = Device(ctx, ids, 16000)
        for c in range(2 * T):
            t = c // 2
            nb = np.where(((c & 1) == phase) & mask[t, src], size[src], 0).astype(np.int32)
            pk = rows[t, src]
            pcm, isn, icn = devc.call(pk, nb, 160)
            model.call(f"call {c}", ids[watch], pk[watch], nb[watch], 160, (pcm[watch], isn[watch], icn[watch]))
            if c % 4 == 3:
                model.check_estimates(ctx, f"call {c}", ids[watch])
            # rows that play the same stream in the same phase are the same stream under another id but for comfort noise
            same = np.flatnonzero((src == src[watch[4]]) & (phase == phase[watch[4]]))
            if not icn[same].any():
                assert (pcm[same] == pcm[same[0]]).all(), f"call {c}"
        assert ctx.decode_samples_errors() == 0
    finally:
        ctx.close()
    model.tally.report("decode_samples full batch")
    assert model.saw_cn and model.saw_mix


def test_invalid_arguments_enqueue_nothing(golden_dir, oracle_default):
    import torch
    from lyra_amd.codec import LyraHipError
    rows, size = _packets(oracle_default, golden_dir, [120, 184], 2)
    ids = [1, 2]
    ctx = _ctx()
    try:
        dev = torch.device("cuda", 0)
        d_ids = torch.tensor(ids, dtype=torch.int32, device=dev)
        pk = torch.from_numpy(rows[0].copy()).to(dev)
        nb = torch.from_numpy(size.copy()).to(dev)
        for n, rate in ((321, 16000), (481, 48000), (482, 48000), (963, 48000), (321, 32000), (161, 8000), (160, 44100)):
            with pytest.raises(LyraHipError):
                ctx.decode_samples_dev(d_ids, pk, nb, n, rate, torch.zeros((2, n), dtype=torch.int16, device=dev))
        with pytest.raises(LyraHipError):
            ctx.decode_samples_dev(d_ids, pk, nb, 160, 16000, None)          # null output with samples requested
        ctx.synchronize()
        assert ctx.decode_samples_errors() == 0
        # nothing was enqueued: the streams are still in their initial state and decode as a fresh model does
        model = Model(oracle_default, 16000, ids)
        devc = Device(ctx, ids, 16000)
        for t in range(2):
            for k, n in enumerate((160, 160)):
                x = size if k == 0 else np.zeros(2, np.int32)
                model.call(f"hop {t}.{k}", ids, rows[t], x, n, devc.call(rows[t], x, n))
    finally:
        ctx.close()


def test_odd_request_sizes_through_the_resampler(golden_dir, oracle_default):
    """48 kHz with request sizes whose internal length is odd or tiny (111 -> 37, 849 -> 283, 3 -> 1, 0) and 8 / 32 kHz with
    sizes off the 10 ms grid: the output resampler on row lengths that are not multiples of 8, against the model."""
    T = 24
    bits = [64, 120, 184, 120]
    ids = [6, 1, 30, 14]
    rows, size = _packets(oracle_default, golden_dir, bits, T, offset=555)
    for rate, sizes in ((48000, [111, 0, 849, 3, 480, 957, 6]), (8000, [1, 80, 53, 0, 160, 27]), (32000, [2, 320, 638, 74, 0])):
        model = Model(oracle_default, rate, ids)
        ctx = _ctx()
        try:
            devc = Device(ctx, ids, rate)
            played, sent = 0, 0
            for c in range(40):
                n = sizes[c % len(sizes)]
                due = played * 50 // rate + 1
                nb = np.zeros(4, np.int32)
                pk = rows[min(sent, T - 1)]
                if sent < due and sent < T:
                    lost = np.array([False, 6 <= sent < 19, sent % 5 == 2, False])
                    nb = np.where(lost, 0, size).astype(np.int32)
                    sent += 1
                model.call(f"{rate} Hz call {c}", ids, pk, nb, n, devc.call(pk, nb, n))
                played += n
            model.check_estimates(ctx, f"{rate} Hz", ids)
            assert ctx.decode_samples_errors() == 0
        finally:
            ctx.close()
        model.tally.report(f"decode_samples odd sizes {rate} Hz")
        assert model.saw_two and model.saw_mix


def test_host_form_with_a_larger_batch_begun_behind_one_in_flight(golden_dir, oracle_default):
    """lyra_hip_decode_samples_begin / _end (the C calls: the Python mirror has none) on a fresh context: requests of 2, 5 and
    max_streams = 8 rows, each begun while the one before is in flight -- the scratch grows under a request in flight, and at
    8 rows the last row of every array of the slot borders the next array.  Against the blocking `_dev` call on a second
    context."""
    import ctypes
    rate, ms = 48000, 8
    rows, size = _packets(oracle_default, golden_dir, [120, 184, 64, 184, 120, 64, 184, 120], 3)
    calls = [(2, 480), (5, 960), (8, 3)]
    ctx, ref = _ctx(ms), _ctx(ms)
    try:
        vp, ci = ctypes.c_void_p, ctypes.c_int
        begin, end = ctx.L.lyra_hip_decode_samples_begin, ctx.L.lyra_hip_decode_samples_end
        begin.restype, begin.argtypes = ci, [vp, vp, ci, vp, vp, ci, ci]
        end.restype, end.argtypes = ci, [vp, vp]
        ids = np.arange(ms, dtype=np.int32)
        want = [Device(ref, ids[:B], rate).call(rows[k][:B], size[:B], n)[0] for k, (B, n) in enumerate(calls)]
        got = [np.full((B, n), 0x3333, np.int16) for B, n in calls]
        assert end(ctx.h, got[0].ctypes.data) != 0                                  # nothing in flight
        for k, (B, n) in enumerate(calls):
            pk, nb = np.ascontiguousarray(rows[k][:B]), np.ascontiguousarray(size[:B])
            assert begin(ctx.h, ids.ctypes.data, B, pk.ctypes.data, nb.ctypes.data, n, rate) == 0, ctx.last_error()
            pk[...] = 0xEE                                                          # the arrays are the caller's again
            if k:
                assert end(ctx.h, got[k - 1].ctypes.data) == 0
        assert end(ctx.h, got[-1].ctypes.data) == 0
        for k, (w, g) in enumerate(zip(want, got)):
            assert np.array_equal(w, g), f"request {k}"
        assert np.array_equal(ctx.export_streams(ids), ref.export_streams(ids))
        assert ctx.decode_samples_errors() == 0
    finally:
        ctx.close(); ref.close()


@pytest.mark.parametrize("pipelined", [False, True])
def test_device_decoder_class_equals_batch_decoder(tmp_path, golden_dir, pipelined):
    """DeviceLyraDecoder through lyra_amd/device_decoder_demo against BatchLyraDecoder through lyra_amd/decoder_demo on the
    same script: a 10 ms / 48 kHz session with bursty loss (one stream all the way into comfort noise and back), the same
    packets and the same samples bit for bit, blocking and pipelined; a request outside the size rule is refused."""
    import subprocess
    import lyra_amd
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    old, new = os.path.join(root, "lyra_amd", "decoder_demo"), os.path.join(root, "lyra_amd", "device_decoder_demo")
    assert os.path.exists(old) and os.path.exists(new), "demos not built (__graft_entry__.build())"
    rate, bitrate, n, T = 48000, 6000, 70, 40
    hop = rate // 50
    rng = np.random.default_rng(19)
    up = np.repeat(_speech(golden_dir, n, T), 3, axis=2)
    mask = np.ones((T, n), np.uint8)
    state = np.zeros(n, bool)
    for t in range(T):
        state = np.where(state, rng.random(n) < 0.6, rng.random(n) < 0.12)
        mask[t] = ~state
    mask[5:17, 7] = 0
    pin, sc = tmp_path / "in.s16", tmp_path / "script.txt"
    up.astype(np.int16).tofile(pin)
    sc.write_text("\n".join("".join(map(str, mask[t])) + f" {hop // 2} {hop // 2}" for t in range(T)) + "\n")
    env = dict(os.environ, LYRA_DEMO_PIPELINED="1" if pipelined else "0")
    res = {}
    for name, exe in (("old", old), ("new", new)):
        files = [tmp_path / f"{name}.{x}" for x in ("pk", "len", "pcm")]
        r = subprocess.run([exe, lyra_amd.default_model_dir(), str(sc), str(pin), str(rate), str(bitrate), "0", str(n)] +
                           [str(f) for f in files], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-3000:])
        res[name] = [np.fromfile(f, np.uint8) for f in files]
    assert res["old"][2].size == T * n * hop * 2
    for a, b in zip(res["old"], res["new"]):
        assert np.array_equal(a, b)
    # a request outside the size rule (481 is no multiple of 3; 963 is more than a hop) takes the error path with a reason
    for k in (481, 963):
        sc.write_text("1" * n + f" {k}\n")
        files = [tmp_path / f"bad.{x}" for x in ("pk", "len", "pcm")]
        r = subprocess.run([new, lyra_amd.default_model_dir(), str(sc), str(pin), str(rate), str(bitrate), "0", str(n)] +
                           [str(f) for f in files], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 6 and "size rule" in r.stderr, (k, r.returncode, r.stderr[-2000:])
        assert files[2].stat().st_size == 0
