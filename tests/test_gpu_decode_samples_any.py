"""lyra_hip_decode_samples_any_dev: LyraDecoder::SetEncodedPacket + DecodeSamples(n) for ANY n of 0 .. 4 hops on the device,
BufferedResampler's leftover included.  Expectations: oracle/lyra_codec_model.py's RefLyraDecoder on the C oracle, stream by
stream and call by call, with receiver_models' Tally / CnReach -- exact where only the generative model speaks, within 1 LSB
where comfort noise reaches (that module's bounds; none of its own) --, both flags and the decoder-side estimate; and bit for
bit against lyra_hip_decode_samples_dev where the old size rule holds, against the same samples asked for in pieces, and
against the same streams in other batch shapes or moved to another context.

Stream kind: the contexts here (64 to 512 streams) run on the CU-masked streams the library picks up to 1,024 streams, which
are blocking streams with respect to the NULL stream; the case with streams="plain" runs on hipStreamNonBlocking streams, the
kind of a 4,096-stream context (tests/gpu_plumbing.py make_ctx)."""
import ctypes

import numpy as np
import pytest

from gpu_plumbing import make_ctx, stream_cases
from receiver_models import ROW, Device, _model_packets as _packets
from receiver_models_any import DeviceAny, ModelAny

pytestmark = pytest.mark.gpu

SIZES = {48000: [128, 1024, 441, 1, 2, 0, 960, 3840, 959], 32000: [128, 1, 641, 2560, 75], 8000: [128, 161, 640, 1],
         16000: [321, 1024, 1280, 7]}


def _deliver(model, devc, ids, rows, size, lost, sent, due, T, n, where):
    """The packets that are due: all but the last in n = 0 calls of their own, the last with the request of n samples."""
    while True:
        nb = np.zeros(len(ids), np.int32)
        pk = rows[min(sent, T - 1)]
        if sent < due and sent < T:
            nb = np.where(lost(sent), 0, size).astype(np.int32)
            sent += 1
        last = not (sent < due and sent < T)
        k = n if last else 0
        model.call(where, ids, pk, nb, k, devc.call(pk, nb, k))
        if last:
            return sent


@pytest.mark.parametrize("rate", [48000, 32000, 8000, 16000])
def test_audio_callback_sizes_vs_reference_model(golden_dir, oracle_default, rate):
    """About 40 calls whose sizes cycle through callback sizes, single samples, whole hops and four hops; the loss pattern of
    test_odd_request_sizes_through_the_resampler (stream 1 goes into comfort noise and back)."""
    sizes = SIZES[rate]
    T = sum(sizes[c % len(sizes)] for c in range(40)) * 50 // rate + 2      # the packets the session's playout time asks for
    bits = [64, 120, 184, 120]
    ids = [6, 1, 30, 14]
    rows, size = _packets(oracle_default, golden_dir, bits, T, offset=555)
    model = ModelAny(oracle_default, rate, ids)
    ctx = make_ctx(256)
    try:
        devc = DeviceAny(ctx, ids, rate)
        played, sent = 0, 0
        for c in range(40):
            n = sizes[c % len(sizes)]
            due = played * 50 // rate + 1
            sent = _deliver(model, devc, ids, rows, size, lambda t: np.array([False, 6 <= t < 19, t % 5 == 2, False]), sent, due,
                            T, n, f"{rate} Hz call {c}")
            played += n
            if c % 8 == 7:
                model.check_estimates(ctx, f"{rate} Hz call {c}", ids)
        model.check_estimates(ctx, f"{rate} Hz", ids)
        assert ctx.decode_samples_errors() == model.dropped    # (a packet that finds 4 waiting is dropped by both)
    finally:
        ctx.close()
    model.tally.report(f"decode_samples_any {rate} Hz")
    print("rounds", model.saw_rounds, "leftover", model.saw_left, "from the leftover alone", model.saw_left_only)
    assert model.saw_two and model.saw_mix and model.saw_cn and model.saw_back
    assert model.saw_rounds[2] + model.saw_rounds[3] and model.saw_rounds[4]
    top = {48000: 2, 32000: 1, 16000: 0, 8000: 0}[rate]
    assert all(model.saw_left[k] > 0 for k in range(top + 1)) and not any(model.saw_left[top + 1:])


def test_rows_with_different_leftovers_in_one_call(golden_dir, oracle_default):
    """48 kHz: three streams brought to leftover 0, 1 and 2 by calls of 128, then ONE call of 961 (internal lengths 321, 320,
    320: the first row needs two rounds, the others one), then a call of 2 that the row holding 2 serves with no internal
    sample, then 128 and 3840 for all."""
    rate, ids = 48000, [11, 4, 200]
    rows, size = _packets(oracle_default, golden_dir, [184, 120, 64], 10, offset=100)
    model = ModelAny(oracle_default, rate, ids)
    ctx = make_ctx(256)
    try:
        devc = DeviceAny(ctx, ids, rate)
        zero = np.zeros(3, np.int32)

        def call(where, sel, t, n, with_packet=True):
            sub = [ids[s] for s in sel]
            devc.set_ids(sub)
            nb = size[sel] if with_packet else zero[sel]
            model.call(where, sub, rows[t][sel], nb, n, devc.call(rows[t][sel], nb, n))

        call("128 for b, c", [1, 2], 0, 128)
        call("128 for c", [2], 1, 128)
        assert [model.decs[i].leftover.size for i in ids] == [0, 1, 2]
        call("961 for all", [0, 1, 2], 1, 961)
        assert model.saw_rounds[2] == 1 and [model.decs[i].leftover.size for i in ids] == [2, 0, 1]
        call("2 for all", [0, 1, 2], 2, 2, with_packet=False)
        assert model.saw_left_only == 1
        call("1 for all", [2, 0, 1], 2, 1, with_packet=False)
        call("128 for all", [0, 1, 2], 3, 128)
        call("3840 for all", [0, 1, 2], 4, 3840)
        model.check_estimates(ctx, "end", ids)
        assert ctx.decode_samples_errors() == 0
    finally:
        ctx.close()


def _lossy_ten_ms(rows, size, T):
    """10 ms calls: (rows of the hop, sizes or zeros): a packet every second call, stream 1 loses hops 4..15, stream 2 every
    fourth"""
    for c in range(2 * T):
        t = c // 2
        lost = np.array([False, 4 <= t < 16, t % 4 == 1])
        yield rows[t], (np.where(lost, 0, size) if c % 2 == 0 else np.zeros(3)).astype(np.int32)


def test_old_rule_sizes_are_the_old_call(golden_dir, oracle_default):
    """The same 10 ms / 48 kHz lossy session through decode_samples_dev on one context and decode_samples_any_dev on another:
    PCM, flags and the exported state byte for byte; stream 2 switches from the new call to the old one mid-session."""
    rate, T, ids = 48000, 22, [3, 60, 17]
    rows, size = _packets(oracle_default, golden_dir, [120, 184, 64], T, offset=300)
    a, b = make_ctx(64), make_ctx(64)
    try:
        old, new = Device(a, ids, rate), DeviceAny(b, ids, rate)
        new01, old2 = DeviceAny(b, ids[:2], rate), Device(b, ids[2:], rate)
        for c, (pk, nb) in enumerate(_lossy_ten_ms(rows, size, T)):
            want = old.call(pk, nb, 480)
            if c < T:
                got = new.call(pk, nb, 480)
            else:
                x, y = new01.call(pk[:2], nb[:2], 480), old2.call(pk[2:], nb[2:], 480)
                got = tuple(np.concatenate([p, q]) for p, q in zip(x, y))
            for w, g, what in zip(want, got, ("pcm", "is_noise", "is_comfort_noise")):
                assert np.array_equal(w, g), f"call {c}: {what}"
            if c == 30:
                assert want[2][1] == 1, "stream 1 never reached comfort noise"
        assert np.array_equal(a.export_streams(ids), b.export_streams(ids))
        assert a.decode_samples_errors() == 0 and b.decode_samples_errors() == 0
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("rate,streams", stream_cases([16000, 48000], plain=48000))
def test_whole_equals_pieces(golden_dir, oracle_default, rate, streams):
    """4 packets queued by n = 0 calls, then one request of 4 hops against four requests of one hop on a second context; then
    the same without packets (concealment, the fade to comfort noise) and with one late packet: PCM and state byte for byte."""
    ids, hop = [9, 2], rate // 50
    rows, size = _packets(oracle_default, golden_dir, [184, 64], 9, offset=40)
    a, b = make_ctx(64, streams=streams), make_ctx(64, streams=streams)
    try:
        da, db = DeviceAny(a, ids, rate), DeviceAny(b, ids, rate)
        none = np.zeros(2, np.int32)
        for phase, queued in enumerate(([0, 1, 2, 3], [], [], [4], [5, 6, 7, 8])):
            for t in queued:
                da.call(rows[t], size, 0); db.call(rows[t], size, 0)
            whole = da.call(rows[0], none, 4 * hop)
            parts = [db.call(rows[0], none, hop) for _ in range(4)]
            assert np.array_equal(whole[0], np.concatenate([p[0] for p in parts], axis=1)), f"phase {phase}: pcm"
            assert np.array_equal(whole[1], parts[-1][1]) and np.array_equal(whole[2], parts[-1][2]), f"phase {phase}: flags"
            assert np.array_equal(a.export_streams(ids), b.export_streams(ids)), f"phase {phase}: state"
            if phase == 2:
                assert whole[2].all(), "three times four lost hops did not reach comfort noise"
        # ... and in uneven pieces that leave and use a leftover (48 kHz): 3840 = 128 + 1024 + 441 + 2247
        whole = da.call(rows[0], none, 4 * hop)
        parts = [db.call(rows[0], none, n) for n in (128, 1024, 441, 4 * hop - 1593)] if rate == 48000 else \
                [db.call(rows[0], none, n) for n in (7, 321, 640, 4 * hop - 968)]
        assert np.array_equal(whole[0], np.concatenate([p[0] for p in parts], axis=1))
        assert np.array_equal(a.export_streams(ids), b.export_streams(ids))
        assert a.decode_samples_errors() == 0 and b.decode_samples_errors() == 0
    finally:
        a.close(); b.close()


def test_a_leftover_travels_with_the_stream(golden_dir, oracle_default):
    """A 48 kHz stream holding 2 leftover samples in the middle of a loss burst is exported and imported under another id of
    another context; both go on, into comfort noise and back: bit for bit."""
    rate = 48000
    rows, size = _packets(oracle_default, golden_dir, [184], 12, offset=70)
    a, b = make_ctx(64), make_ctx(64, cng_seed=12345)
    try:
        da, db = DeviceAny(a, [5], rate), DeviceAny(b, [41], rate)
        none = np.zeros(1, np.int32)
        da.call(rows[0], size, 128)
        da.call(rows[1], size, 128)          # 128 + 128 = 256 = 3 * 86 - 2: two samples stay
        da.call(rows[1], none, 960 + 1920)   # ... and three hops into a burst: 958 internal samples' worth, 2 stay again
        blob = a.export_streams([5])
        b.import_streams([41], blob)
        for c, (n, t) in enumerate([(2, None), (1, None), (1024, None), (3840, None), (3840, None), (441, 2), (128, 3), (1024, 4),
                                    (3, None), (959, 5)]):
            nb = none if t is None else size
            pk = rows[t or 0]
            x, y = da.call(pk, nb, n), db.call(pk, nb, n)
            for u, v, what in zip(x, y, ("pcm", "is_noise", "is_comfort_noise")):
                assert np.array_equal(u, v), f"call {c} ({n} samples): {what}"
            if c == 4:
                assert x[2][0] == 1, "the burst did not reach comfort noise"
        assert x[2][0] == 0
        x, y = a.export_streams([5]), b.export_streams([41])
        assert x[0, 24] == 5 and y[0, 24] == 41            # the blob header's source stream id: the one word that differs
        x[0, 24], y[0, 24] = 0, 0
        assert np.array_equal(x, y)
    finally:
        a.close(); b.close()


def test_batch_shape(golden_dir, oracle_default):
    """B = 261: two plan blocks, a last group of one row.  Every row byte for byte the same streams run in batches of at most
    16 on a second context; 8 rows against the model."""
    rate, B = 48000, 261
    rng = np.random.default_rng(5)
    ids = rng.permutation(300)[:B].astype(np.int32)
    sizes = [128, 961, 2, 1024, 0, 3840]
    pk = rng.integers(0, 256, size=(len(sizes), B, ROW)).astype(np.uint8)
    nb = rng.choice([0, 8, 15, 23, 23], size=(len(sizes), B)).astype(np.int32)
    nb[4] = 0                                             # (at most 2 vectors ever wait: nothing is dropped)
    nb[2:, 256] = 0; nb[2:, 260] = 0; nb[2:, 7] = 0       # rows that run into concealment across the large calls
    rows8 = [0, 7, 63, 64, 255, 256, 259, 260]
    model = ModelAny(oracle_default, rate, [int(ids[r]) for r in rows8])
    a, b = make_ctx(512), make_ctx(512)
    try:
        da = DeviceAny(a, ids, rate)
        for c, n in enumerate(sizes):
            got = da.call(pk[c], nb[c], n)
            lo = k = 0
            while lo < B:
                hi = min(B, lo + 16 - k % 3)               # batches of 16, 15 and 14 rows
                part = DeviceAny(b, ids[lo:hi], rate).call(pk[c, lo:hi], nb[c, lo:hi], n)
                for g, p, what in zip(got, part, ("pcm", "is_noise", "is_comfort_noise")):
                    assert np.array_equal(g[lo:hi], p), f"call {c}, rows {lo}..{hi}: {what}"
                lo, k = hi, k + 1
            model.call(f"call {c}", ids[rows8], pk[c][rows8], nb[c][rows8], n, tuple(x[rows8] for x in got))
        assert np.array_equal(a.export_streams(ids), b.export_streams(ids))
        assert a.decode_samples_errors() == 0 and b.decode_samples_errors() == 0
    finally:
        a.close(); b.close()


def test_host_form_and_refusals(golden_dir, oracle_default):
    import torch
    from lyra_amd.codec import LyraHipError
    rate, ids = 48000, [1, 2]
    rows, size = _packets(oracle_default, golden_dir, [120, 184], 6)
    ctx, ref = make_ctx(64), make_ctx(64)
    try:
        dev = torch.device("cuda", 0)
        d_ids = torch.tensor(ids, dtype=torch.int32, device=dev)
        pk = torch.from_numpy(rows[0].copy()).to(dev)
        nb = torch.from_numpy(size.copy()).to(dev)
        for n, r in ((3841, 48000), (-1, 48000), (1281, 16000), (441, 44100), (641, 8000)):
            with pytest.raises(LyraHipError):
                ctx.decode_samples_any_dev(d_ids, pk, nb, n, r, torch.zeros((2, n), dtype=torch.int16, device=dev) if n > 0 else None)
            with pytest.raises(LyraHipError):
                ctx.decode_samples_any_begin(rows[0], size, n, r, ids)
        with pytest.raises(LyraHipError):
            ctx.decode_samples_any_dev(d_ids, pk, nb, 128, rate, None)            # null output with samples requested
        with pytest.raises(LyraHipError):
            ctx.decode_samples_any_end()                                          # nothing in flight
        with pytest.raises(LyraHipError):
            ctx.decode_samples_any_begin(rows[0], size, 128, rate, [1, 1])        # duplicate id
        # one decode pipeline at a time: a decode_streams hop or a decode_samples request in flight refuses begin()
        ctx.decode_streams_begin(rows[0], np.zeros(2, np.int32), np.full(2, rate, np.int32), [40, 41])
        with pytest.raises(LyraHipError):
            ctx.decode_samples_any_begin(rows[0], size, 128, rate, ids)
        ctx.decode_streams_end()
        L = ctx.L
        vp, ci = ctypes.c_void_p, ctypes.c_int
        L.lyra_hip_decode_samples_begin.restype, L.lyra_hip_decode_samples_begin.argtypes = ci, [vp, vp, ci, vp, vp, ci, ci]
        L.lyra_hip_decode_samples_end.restype, L.lyra_hip_decode_samples_end.argtypes = ci, [vp, vp]
        other, none = np.array([40, 41], np.int32), np.zeros(2, np.int32)
        assert L.lyra_hip_decode_samples_begin(ctx.h, other.ctypes.data, 2, rows[0].ctypes.data, none.ctypes.data, 0, rate) == 0
        with pytest.raises(LyraHipError):
            ctx.decode_samples_any_begin(rows[0], size, 128, rate, ids)
        assert L.lyra_hip_decode_samples_end(ctx.h, None) == 0
        # ... and the other way round, and export / import, while a request of this pipeline is in flight
        ctx.decode_samples_any_begin(rows[0], none, 0, rate, [40, 41])
        assert L.lyra_hip_decode_samples_begin(ctx.h, other.ctypes.data, 2, rows[0].ctypes.data, none.ctypes.data, 0, rate) != 0
        with pytest.raises(LyraHipError):
            ctx.decode_streams_begin(rows[0], none, np.full(2, rate, np.int32), [40, 41])
        with pytest.raises(LyraHipError):
            ctx.export_streams([40])
        ctx.decode_samples_any_begin(rows[0], none, 0, rate, [40, 41])
        with pytest.raises(LyraHipError):
            ctx.decode_samples_any_begin(rows[0], none, 0, rate, [40, 41])        # a third begin()
        assert ctx.decode_samples_any_end().shape == (2, 0) and ctx.decode_samples_any_end().shape == (2, 0)
        ctx.synchronize()
        assert ctx.decode_samples_errors() == 0
        # nothing was enqueued for streams 1 and 2: they decode as fresh ones.  The host form two deep against the _dev form.
        devc = DeviceAny(ref, ids, rate)
        calls = [(0, size, 128), (1, size, 1024), (1, np.zeros(2, np.int32), 441), (2, size, 3840), (3, size, 2), (4, size, 959)]
        want = [devc.call(rows[t], x, n)[0] for t, x, n in calls]
        got = []
        for k, (t, x, n) in enumerate(calls):
            ctx.decode_samples_any_begin(rows[t], x, n, rate, ids)
            if k:
                got.append(ctx.decode_samples_any_end())
        got.append(ctx.decode_samples_any_end())
        for k, (w, g) in enumerate(zip(want, got)):
            assert np.array_equal(w, g), f"request {k}"
        assert np.array_equal(ctx.export_streams(ids), ref.export_streams(ids))
    finally:
        ctx.close(); ref.close()


def test_a_larger_batch_begun_behind_one_in_flight(golden_dir, oracle_default):
    """Requests of 2, 5 and max_streams = 8 rows, each begun while the one before is in flight: the scratch grows under a
    request in flight, and at 8 rows the last row of every array of the slot borders the next array.  Against the blocking
    `_dev` call on a second context."""
    rate, ms = 48000, 8
    rows, size = _packets(oracle_default, golden_dir, [120, 184, 64, 184, 120, 64, 184, 120], 3)
    calls = [(2, 441), (5, 1024), (8, 3840)]
    ctx, ref = make_ctx(ms), make_ctx(ms)
    try:
        ids = np.arange(ms, dtype=np.int32)
        want = [DeviceAny(ref, ids[:B], rate).call(rows[k][:B], size[:B], n)[0] for k, (B, n) in enumerate(calls)]
        got = []
        for k, (B, n) in enumerate(calls):
            ctx.decode_samples_any_begin(rows[k][:B].copy(), size[:B].copy(), n, rate, ids[:B])
            if k:
                got.append(ctx.decode_samples_any_end())
        got.append(ctx.decode_samples_any_end())
        for k, (w, g) in enumerate(zip(want, got)):
            assert np.array_equal(w, g), f"request {k}"
        assert np.array_equal(ctx.export_streams(ids), ref.export_streams(ids))
        assert ctx.decode_samples_errors() == 0
    finally:
        ctx.close(); ref.close()


@pytest.mark.parametrize("pipelined", [False, True])
def test_any_size_class_equals_batch_decoder(tmp_path, golden_dir, pipelined):
    """AnySizeDeviceLyraDecoder through lyra_amd/device_decoder_demo (LYRA_DEMO_ANY_SIZE=1) against BatchLyraDecoder, which keeps
    the leftover on the host, through lyra_amd/decoder_demo on the same script: 48 kHz, callbacks of 128 / 1024 / 441 frames
    under bursty loss (one stream into comfort noise and back): the same packets and samples byte for byte, blocking and
    pipelined; a request above four hops is refused with a reason."""
    import os
    import subprocess
    import lyra_amd
    from signals import _speech
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    old, new = os.path.join(root, "lyra_amd", "decoder_demo"), os.path.join(root, "lyra_amd", "device_decoder_demo")
    assert os.path.exists(old) and os.path.exists(new), "demos not built (__graft_entry__.build())"
    rate, bitrate, n, T = 48000, 6000, 20, 36
    hop = rate // 50
    rng = np.random.default_rng(23)
    up = np.repeat(_speech(golden_dir, n, T), 3, axis=2)
    mask = np.ones((T, n), np.uint8)
    state = np.zeros(n, bool)
    for t in range(T):
        state = np.where(state, rng.random(n) < 0.6, rng.random(n) < 0.12)
        mask[t] = ~state
    mask[5:17, 7] = 0
    lines, played, k = [], 0, 0
    for t in range(T):          # per hop at least one callback (a second packet of a stream cannot overtake requests in flight),
        sizes = []              # and as many as fit into the playout time of the packets handed over so far
        while not sizes or played + (128, 1024, 441)[k % 3] <= (t + 1) * hop:
            sizes.append((128, 1024, 441)[k % 3])
            played, k = played + sizes[-1], k + 1
        lines.append("".join(map(str, mask[t])) + "".join(f" {s}" for s in sizes))
    assert k > 50
    pin, sc = tmp_path / "in.s16", tmp_path / "script.txt"
    up.astype(np.int16).tofile(pin)
    sc.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, LYRA_DEMO_PIPELINED="1" if pipelined else "0", LYRA_DEMO_ANY_SIZE="1")
    res = {}
    for name, exe in (("old", old), ("new", new)):
        files = [tmp_path / f"{name}.{x}" for x in ("pk", "len", "pcm")]
        r = subprocess.run([exe, lyra_amd.default_model_dir(), str(sc), str(pin), str(rate), str(bitrate), "0", str(n)] +
                           [str(f) for f in files], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, (name, r.returncode, r.stderr[-3000:])
        res[name] = [np.fromfile(f, np.uint8) for f in files]
    assert res["old"][2].size == played * n * 2
    for a, b in zip(res["old"], res["new"]):
        assert np.array_equal(a, b)
    sc.write_text("1" * n + " 3841\n")
    files = [tmp_path / f"bad.{x}" for x in ("pk", "len", "pcm")]
    r = subprocess.run([new, lyra_amd.default_model_dir(), str(sc), str(pin), str(rate), str(bitrate), "0", str(n)] +
                       [str(f) for f in files], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 6 and "hops per request" in r.stderr, (r.returncode, r.stderr[-2000:])
    assert files[2].stat().st_size == 0
