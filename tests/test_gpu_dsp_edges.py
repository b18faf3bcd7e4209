"""The four DSP kernels beside the networks at their edges, through the public calls only (helpers and bounds: tests/dsp_cases.py,
checked on the CPU by tests/test_dsp_refs_cpu.py):
  * log-mel against a float64 reference on 14 signal kinds, quiet rows paired with full-scale ones in one FFT, B = 1 / 2 / 3,
    the filterbanks of all four rates (uniform, and mixed inside one workgroup);
  * the estimator recurrence bit for bit at 16 kHz over 160 hops, and its constants at 8 / 32 / 48 kHz across the period wrap;
  * the resampler on chunks of any admitted length -- the scalar load path, chunks shorter than the history, the length checks;
  * the comfort noise on both rails, from given features and from the stream's own noise estimate."""
import functools

import numpy as np
import pytest

import dsp_cases as dc
from oracle import lyra_oracle

pytestmark = pytest.mark.gpu

BITS = 184


@pytest.fixture(scope="module")
def ctx():
    import lyra_amd
    c = lyra_amd.LyraHip(max_streams=64)
    yield c
    c.close()


@pytest.fixture
def fresh(ctx):
    """the module's context with every stream reset, the encoder-side estimator at 16 kHz, the comfort-noise seed set"""
    ctx.reset()
    ctx.set_encoder_sample_rate(16000)
    ctx.set_cng_seed(dc.CNG_SEED)
    return ctx


@functools.lru_cache(maxsize=None)
def _want16(golden_dir):
    """[14][T][160] float64: the log-mel of every signal kind at 16 kHz"""
    x = dc.signals(golden_dir)
    w = np.stack([dc.logmel64(x[k], 16000) for k in range(len(dc.KINDS))])
    w.flags.writeable = False
    return w


# ---- log-mel ---------------------------------------------------------------------------------------------------------------------
def test_logmel_against_float64_in_every_placement(fresh, golden_dir):
    """ctx.logmel on the 14 kinds as one batch, the batch again with the rows of each pair swapped, and B = 1, 2, 3: zeros, +-1
    and speech // 64 each share an FFT with a full-scale row, once as its real and once as its imaginary part.  Every value
    within the device bound of the float64 reference; the placements of a stream within 1 ULP of each other; zeros and +-1
    exactly at the floor."""
    x, want, K = dc.signals(golden_dir), _want16(golden_dir), dc.K
    bound = dc.device_bound(16000)
    pairs = [("white", "zeros"), ("pm1", "square"), ("alternating", "speech64"), ("speech", "dc_hi"), ("dc_lo", "impulses"),
             ("pm12", "pm40"), ("sine", "gated")]
    order_a = [K[n] for p in pairs for n in p]
    order_b = [K[n] for p in pairs for n in p[::-1]]
    assert sorted(order_a) == sorted(order_b) == list(range(14))
    ids = np.random.default_rng(3).permutation(64).astype(np.int32)
    placements = [("batch of 14", order_a, ids[:14]), ("batch of 14, pairs swapped", order_b, ids[14:28]),
                  ("B = 1", [K["speech64"]], ids[28:29]), ("B = 2", [K["white"], K["pm1"]], ids[29:31]),
                  ("B = 3", [K["zeros"], K["square"], K["pm40"]], ids[31:34])]
    seen = {}
    worst = 0.0
    for where, order, pids in placements:
        got = np.stack([fresh.logmel(x[order, t], pids) for t in range(dc.T)])      # [T][n][160]
        for row, k in enumerate(order):
            g = np.ascontiguousarray(got[:, row])
            worst = max(worst, dc.check_logmel(f"{where}, row {row} ({dc.KINDS[k]})", g, want[k], bound))
            if dc.KINDS[k] in ("zeros", "pm1"):
                assert (g == dc.SILENCE).all(), f"{where}, row {row} ({dc.KINDS[k]}): not every band at the floor"
            seen.setdefault(k, []).append((where, g))
    print(f"device log-mel within {worst:.3f} ULP of the float64 reference (bound {bound})")
    assert {len(v) for v in seen.values()} == {2, 3} and all(len(seen[K[n]]) == 3 for n in ("zeros", "pm1", "speech64"))
    for k, runs in seen.items():      # every pair of placements: the largest against the smallest value, element by element
        bits = np.stack([g.view(np.int32).astype(np.int64) for _, g in runs])           # (positive floats: ordered like their bits)
        apart = bits.max(axis=0) - bits.min(axis=0)
        if apart.max() > 1:
            at = tuple(int(v) for v in np.argwhere(apart > 1)[0])
            raise AssertionError(f"{dc.KINDS[k]}: the placements are {int(apart.max())} ULP apart at {at}: "
                                 + ", ".join(f"{where} {g[at]!r}" for where, g in runs))


RATE_ROWS = ("white", "square", "impulses", "pm40")


@pytest.mark.parametrize("rate", dc.RATES)
def test_logmel_filterbank_of_each_rate(fresh, golden_dir, rate):
    """A fresh encoder-side estimator at `rate`, one hop: the first update leaves estimate = sf cur + (1 - sf) cur, the hop's
    log-mel to within 1 ULP -- held to the float64 log-mel with the filterbank of that rate."""
    x = dc.signals(golden_dir)
    rows = [dc.K[n] for n in RATE_ROWS]
    ids = np.array([9, 60, 3, 22], np.int32)
    fresh.set_encoder_sample_rate(rate)
    flags = fresh.noise_receive(x[rows, 0], ids, side="encoder")
    assert not flags.any(), f"the first hop of a stream is an update: {flags}"
    est = fresh.noise_estimate(ids, side="encoder")
    for row, k in enumerate(rows):
        dc.check_logmel(f"{rate} Hz, {dc.KINDS[k]}", est[row:row + 1], dc.logmel64(x[k, :1], rate), dc.device_bound(rate) + 1)


def _ext_hop(rng, rate, kind):
    n = rate // 50
    if kind == "pm40":
        return rng.integers(-40, 41, size=n).astype(np.int16)
    if kind == "square":
        return np.where((np.arange(n) // (n // 4)) % 2 == 0, 32767, -32768).astype(np.int16)
    return rng.integers(-32768, 32768, size=n, dtype=np.int16)


# case -> (rates, dtx, signal kind per row, seed of the rows' noise)
MIXED = {"8k+48k": ((8000, 48000), (1, 1), ("white", "white"), 101),
         "48k+8k": ((48000, 8000), (1, 1), ("white", "square"), 102),
         "16k+32k": ((16000, 32000), (1, 1), ("pm40", "white"), 103),
         "second row without dtx": ((8000, 48000), (1, 0), ("white", "white"), 104),
         "odd row count": ((32000, 8000, 48000), (1, 1, 1), ("white", "pm40", "white"), 105)}


@pytest.mark.parametrize("case", list(MIXED))
def test_logmel_mixed_rates_in_one_workgroup(fresh, case):
    """One hop through encode_streams_begin / _end with DTX: the two rows of a workgroup carry different filterbanks (the second
    weight table in LDS, band edges per item).  Want: the oracle's resampler (held bit-exact elsewhere) feeding the float64
    log-mel of the row's rate; a row without DTX has no estimator and its slot stays as reset left it."""
    rates, dtx, kinds, seed = MIXED[case]
    rng = np.random.default_rng(seed)
    ext = [_ext_hop(rng, r, k) for r, k in zip(rates, kinds)]
    ids = np.array([17, 4, 50][:len(rates)], np.int32)
    fresh.encode_streams_begin(np.concatenate(ext), np.array(rates, np.int32), np.full(len(rates), BITS, np.int32),
                               np.array(dtx, np.int32), ids)
    _, nbytes = fresh.encode_streams_end()
    assert (nbytes == BITS // 8).all(), f"the first hop of a stream is never noise: packet bytes {nbytes}"
    est = fresh.noise_estimate(ids, side="encoder")
    for row, (rate, on) in enumerate(zip(rates, dtx)):
        if not on:
            assert not est[row].any(), f"row {row} has no estimator, yet its estimate is not the reset one"
            continue
        hop16 = ext[row] if rate == 16000 else lyra_oracle.Resampler(rate, 16000).Resample(ext[row])
        assert hop16.size == 320
        dc.check_logmel(f"{case}, row {row} at {rate} Hz", est[row:row + 1], dc.logmel64(hop16[None], rate), dc.device_bound(rate) + 1)


# ---- estimator ---------------------------------------------------------------------------------------------------------------------
EST_ROWS = ("speech", "noise", "white", "zeros", "speech64", "noise_then_speech", "swell")


@pytest.mark.parametrize("side", ["encoder", "decoder"])
def test_estimator_recurrence_bit_for_bit(fresh, golden_dir, oracle_default, side):
    """The same batch to noise_receive and to ctx.logmel on other ids in the same row order: the same kernel with the same
    pairing, so the mel bits are the estimator's own.  They drive the oracle's ReceiveMel: decisions identical and the estimate
    bit-equal after every one of 160 hops (the 50-hop period three times), as misc_kernels.hip claims for noise_update_wave."""
    hops = 160
    streams = dc.estimator_streams(golden_dir, hops)
    pcm = np.stack([streams[n] for n in EST_ROWS], axis=1)                # [hops][7][320]
    ids_n = np.array([12, 0, 44, 7, 31, 58, 25], np.int32)
    ids_m = np.array([13, 1, 45, 8, 32, 59, 26], np.int32)
    refs = [lyra_oracle.NoiseEstimator(oracle_default) for _ in EST_ROWS]
    n_noise = n_update = 0
    for t in range(hops):
        before = [r.noise_estimate() for r in refs]
        flags = fresh.noise_receive(pcm[t], ids_n, side=side)
        mel = fresh.logmel(pcm[t], ids_m)
        want = np.array([r.ReceiveMel(mel[b]) for b, r in enumerate(refs)], np.int32)
        assert np.array_equal(flags, want), f"{side}, hop {t}: is_noise {flags}, oracle {want} (rows {EST_ROWS})"
        est = fresh.noise_estimate(ids_n, side=side)
        for b, r in enumerate(refs):
            w = r.noise_estimate()
            if not np.array_equal(est[b].view(np.uint32), w.view(np.uint32)):
                i = int(np.flatnonzero(est[b].view(np.uint32) != w.view(np.uint32))[0])
                raise AssertionError(f"{side}, hop {t}, row {b} ({EST_ROWS[b]}), bin {i}: estimate {est[b][i]!r}, oracle {w[i]!r}; "
                                     f"operands: mel {mel[b][i]!r}, estimate before {before[b][i]!r}, is_noise {int(want[b])}, "
                                     f"mean mel {mel[b].mean()!r}")
        n_noise += int(want.sum())
        n_update += int(want.size - want.sum())
    assert n_noise > 0 and n_update > 0, (n_noise, n_update)


@pytest.mark.parametrize("rate", [8000, 32000, 48000])
def test_estimator_constants_per_rate(fresh, golden_dir, oracle_default, rate):
    """330 hops at 8 / 32 / 48 kHz (update periods 25 / 100 / 150 hops): decisions identical to the oracle's estimator of that
    rate on every hop, the estimate within the project's atol = 1e-4 every 10 hops and on the two hops behind each multiple of
    the period."""
    hops, period = 330, rate // 320
    names = ("speech", "noise", "noise_then_speech", "zeros", "swell")
    streams = dc.estimator_streams(golden_dir, hops)
    pcm = np.stack([streams[n] for n in names], axis=1)
    ids = np.array([6, 61, 30, 2, 47], np.int32)
    refs = [lyra_oracle.NoiseEstimator(oracle_default, sample_rate_hz=rate) for _ in names]
    fresh.set_encoder_sample_rate(rate)
    updates = np.zeros(len(names), int)
    for t in range(hops):
        flags = fresh.noise_receive(pcm[t], ids, side="encoder")
        want = np.array([r.ReceiveSamples(pcm[t, b])[0] for b, r in enumerate(refs)], np.int32)
        assert np.array_equal(flags, want), f"{rate} Hz, hop {t}: is_noise {flags}, oracle {want} (rows {names})"
        updates += 1 - want
        # (hops counted in calls, as the schedule is worded: the estimator's own counter advances on updates only, so for a
        # stream that also takes the decay branch the wrap falls on other hops -- those the 10-hop grid and the decisions cover)
        n = t + 1
        if n % 10 == 0 or (n > period and n % period in (1, 2)):
            est = fresh.noise_estimate(ids, side="encoder")
            for b, r in enumerate(refs):
                d = np.abs(est[b] - r.noise_estimate())
                assert d.max() <= 1e-4, f"{rate} Hz, after hop {n}, {names[b]}: estimate off by {d.max():.3g} at bin {int(d.argmax())}"
    assert updates.max() >= 2 * period, f"no stream passed the {period}-hop period twice: updates {updates}"


# ---- resampler ---------------------------------------------------------------------------------------------------------------------
RS_IDS = {1: [41], 4: [5, 0, 33, 12], 5: [7, 63, 2, 50, 19]}


@pytest.mark.parametrize("in_rate,out_rate", dc.DESIGNS)
def test_resampler_any_chunk_length(fresh, in_rate, out_rate):
    """The chunk plan of the CPU test through ctx.resample on both sides, B = 1, 4 and 5 (a full workgroup plus one), scattered
    ids: every chunk bit-equal to the oracle stream's -- the scalar load path, chunks shorter than the 34-sample history, and a
    whole hop on the 16-byte path behind them."""
    plan = dc.chunk_plan(in_rate, out_rate)
    up, down = dc.up_down(in_rate, out_rate)
    lo = hi = 0
    for side in ("encoder", "decoder"):
        for B, ids in RS_IDS.items():
            ids = np.array(ids, np.int32)
            x = [dc.resampler_input(sum(plan), seed=in_rate + out_rate + 10 * B + b + (side == "decoder"), down=down) for b in range(B)]
            parts = [dc.split(r, plan) for r in x]
            refs = [lyra_oracle.Resampler(in_rate, out_rate) for _ in range(B)]
            for i, n_in in enumerate(plan):
                got = fresh.resample(np.stack([p[i] for p in parts]), in_rate, out_rate, ids, side=side)
                want = np.stack([r.Resample(p[i]) for r, p in zip(refs, parts)])
                dc.same_samples(f"{in_rate} -> {out_rate}, {side}, B = {B}, chunk {i} of {n_in} samples", got, want)
                a, b = dc.rails(got)
                lo, hi = lo + a, hi + b
    assert lo > 0 and hi > 0, f"{in_rate} -> {out_rate}: {lo} device samples at -32768, {hi} at 32767"


def test_resample_dev_unaligned_rows_take_the_scalar_path(golden_dir):
    """resample_dev on a whole hop in a 16-byte-aligned tensor, and on the same data in a view that starts one int16 later (the
    scalar path with n_in % 8 == 0), on two contexts: equal to each other and to the oracle, for the six designs."""
    import torch
    import lyra_amd
    dev = torch.device("cuda", 0)
    a, b = lyra_amd.LyraHip(max_streams=64), lyra_amd.LyraHip(max_streams=64)
    ids = np.array([7, 63, 2, 50, 19], np.int32)
    B = ids.size
    try:
        d_ids = torch.from_numpy(ids).to(dev)
        for in_rate, out_rate in dc.DESIGNS:
            a.reset(); b.reset()
            n_in, n_out = in_rate // 50, out_rate // 50
            down = dc.up_down(in_rate, out_rate)[1]
            x = np.stack([dc.resampler_input(n_in, seed=in_rate + out_rate + r, down=down, burst_at=20) for r in range(B)])
            side = "encoder" if out_rate == 16000 else "decoder"
            aligned = torch.from_numpy(x).to(dev)
            room = torch.zeros(B * n_in + 8, device=dev, dtype=torch.int16)
            assert aligned.data_ptr() % 16 == 0 and room.data_ptr() % 16 == 0
            shifted = room[1:1 + B * n_in].view(B, n_in)
            shifted.copy_(aligned)
            assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 2
            out_a = torch.zeros((B, n_out), device=dev, dtype=torch.int16)
            out_b = torch.zeros((B, n_out), device=dev, dtype=torch.int16)
            a.resample_dev(d_ids, aligned, in_rate, out_rate, out_a, side=side)
            b.resample_dev(d_ids, shifted, in_rate, out_rate, out_b, side=side)
            a.synchronize(); b.synchronize()
            want = np.stack([lyra_oracle.Resampler(in_rate, out_rate).Resample(r) for r in x])
            dc.same_samples(f"{in_rate} -> {out_rate}, aligned rows", out_a.cpu().numpy(), want)
            dc.same_samples(f"{in_rate} -> {out_rate}, rows one int16 off", out_b.cpu().numpy(), want)
    finally:
        a.close()
        b.close()


def test_resample_refusals_leave_the_stream_untouched():
    """n_in = 0, 961, no multiple of the decimation factor, more than 960 outputs, a rate that is no codec rate, a pair with
    neither side at 16 kHz: LyraHipError, and the next valid chunk of the same stream still equals the oracle's.  16000 -> 16000
    is no refusal: include/lyra_hip.h admits it ("one of them 16000") and the reference's own test creates that resampler
    (lyra/resampler_test.cc:45-48) -- the 1:1 pass through the filter bank is held to the oracle's like the six designs."""
    import lyra_amd
    ctx = lyra_amd.LyraHip(max_streams=64)
    ids = np.array([9, 40], np.int32)
    try:
        for side, (in_rate, out_rate), refused in (
                ("encoder", (32000, 16000), [(0, 32000, 16000), (961, 32000, 16000), (3, 32000, 16000), (882, 44100, 16000),
                                             (960, 48000, 8000)]),
                ("decoder", (16000, 48000), [(0, 16000, 48000), (961, 16000, 48000), (321, 16000, 48000), (320, 16000, 44100),
                                             (160, 8000, 48000)])):
            down = dc.up_down(in_rate, out_rate)[1]
            first, hop = 17 * down, in_rate // 50
            x = np.stack([dc.resampler_input(first + hop, seed=5 + b, down=down, burst_at=10) for b in range(2)])
            refs = [lyra_oracle.Resampler(in_rate, out_rate) for _ in range(2)]
            got = ctx.resample(x[:, :first], in_rate, out_rate, ids, side=side)
            dc.same_samples(f"{side}: first chunk", got, np.stack([r.Resample(row[:first]) for r, row in zip(refs, x)]))
            for n_in, a, b in refused:
                with pytest.raises(lyra_amd.LyraHipError):
                    ctx.resample(np.full((2, n_in), 12345, np.int16), a, b, ids, side=side)
            got = ctx.resample(x[:, first:], in_rate, out_rate, ids, side=side)
            dc.same_samples(f"{side}: the chunk behind the refused calls", got,
                            np.stack([r.Resample(row[first:]) for r, row in zip(refs, x)]))
        ids = np.array([11, 62], np.int32)
        x = np.stack([dc.resampler_input(17 + 320, seed=15 + b, burst_at=10) for b in range(2)])
        refs = [lyra_oracle.Resampler(16000, 16000) for _ in range(2)]
        for lo, hi in ((0, 17), (17, 337)):
            got = ctx.resample(x[:, lo:hi], 16000, 16000, ids, side="decoder")
            dc.same_samples(f"16000 -> 16000, samples {lo}..{hi}", got, np.stack([r.Resample(row[lo:hi]) for r, row in zip(refs, x)]))
    finally:
        ctx.close()


# ---- comfort noise -----------------------------------------------------------------------------------------------------------------
def test_comfort_noise_on_the_rails(fresh, oracle_exact):
    """constant features 0.6215 / 1.0 / 1.3 / 1.5 and the estimate of full-scale white noise, B = 5 in one call, 8 hops: every
    sample within 1 LSB of the oracle, the loud rows on both rails on the device itself, the quiet row below 100"""
    feats = dc.cng_features(oracle_exact)
    ids = np.array([7, 0, 33, 12, 5], np.int32)
    want = dc.oracle_cng(oracle_exact, feats, ids)
    got = np.stack([fresh.comfort_noise(feats, ids) for _ in range(dc.CNG_HOPS)])
    for t in range(dc.CNG_HOPS):
        dc.within_one_lsb(f"hop {t}", got[t], want[t])
    for r in dc.CNG_LOUD:
        lo, hi = dc.rails(got[:, r])
        assert lo > 0 and hi > 0, f"feature row {r}: {lo} device samples at -32768, {hi} at 32767"
    assert np.abs(got[:, 0].astype(int)).max() < 100


def test_comfort_noise_from_a_loud_noise_estimate(fresh, oracle_exact):
    """features = None: 40 hops of full-scale white noise through noise_receive on the decoder side, then 8 hops of comfort
    noise from each stream's own estimate -- against the oracle's estimator feeding the oracle's generator"""
    ids = np.array([21, 3, 40], np.int32)
    pcm = np.stack([dc.white_hops(seed=77 + b) for b in range(ids.size)], axis=1)        # [40][3][320]
    refs = [lyra_oracle.NoiseEstimator(oracle_exact) for _ in ids]
    for t in range(dc.NOISE_HOPS):
        flags = fresh.noise_receive(pcm[t], ids, side="decoder")
        want = [int(r.ReceiveSamples(pcm[t, b])[0]) for b, r in enumerate(refs)]
        assert list(flags) == want, (t, flags, want)
    est = np.stack([r.noise_estimate() for r in refs])
    want = dc.oracle_cng(oracle_exact, est, ids)
    got = np.stack([fresh.comfort_noise(None, ids) for _ in range(dc.CNG_HOPS)])
    for t in range(dc.CNG_HOPS):
        dc.within_one_lsb(f"hop {t}", got[t], want[t])
    for b in range(ids.size):
        lo, hi = dc.rails(got[:, b])
        assert lo > 0 and hi > 0, f"row {b}: {lo} device samples at -32768, {hi} at 32767"
