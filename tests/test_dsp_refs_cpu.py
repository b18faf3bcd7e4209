"""The references tests/test_gpu_dsp_edges.py holds the DSP kernels to, checked on the CPU (helpers: tests/dsp_cases.py): the
oracle's log-mel against the float64 one at all four filterbank rates -- which measures the bounds table --, the oracle's
ReceiveMel entry point, the resampler chunk by chunk, the comfort noise on its rails, and the mutants that the comparisons
used on the device have to reject."""
import numpy as np
import pytest

import dsp_cases as dc
from oracle import lyra_oracle


# ---- log-mel: the oracle against the float64 reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("rate", dc.RATES)
def test_oracle_logmel_within_the_table(golden_dir, oracle_default, rate):
    x = dc.signals(golden_dir)
    worst = {}
    for k, name in enumerate(dc.KINDS):
        got = dc.oracle_logmel(oracle_default, x[k], rate)
        worst[name] = dc.check_logmel(f"oracle, {rate} Hz, {name}", got, dc.logmel64(x[k], rate), dc.LOGMEL_ORACLE_ULP[rate])
        if name in ("zeros", "pm1"):
            assert (got == dc.SILENCE).all(), f"{name}: not every band at the floor"
    measured = max(worst.values())
    print(f"{rate} Hz: oracle within {measured:.4f} ULP of the float64 log-mel; per kind {worst}")
    assert measured >= 0.8 * dc.LOGMEL_ORACLE_ULP[rate], f"stale table: {measured:.4f} measured, {dc.LOGMEL_ORACLE_ULP[rate]} listed"
    assert dc.device_bound(rate) <= dc.PARITY_ULP


def test_signal_kinds_cover_floor_and_full_scale(golden_dir, oracle_default):
    x = dc.signals(golden_dir)
    assert x.shape == (14, dc.T, 320) and not x.flags.writeable
    feats = np.stack([dc.oracle_logmel(oracle_default, x[k], 16000) for k in range(len(dc.KINDS))])
    assert feats.min() == dc.SILENCE and abs(float(dc.SILENCE) - 0.6215) < 1e-4 and 1.58 < feats.max() < 1.60
    floored = (feats[dc.K["pm40"]] == dc.SILENCE).mean()
    assert 0.2 < floored < 0.5, f"+-40 noise: {floored:.2f} of the bands at the floor"
    assert not (feats[dc.K["white"]] == dc.SILENCE).any()


# ---- log-mel mutants ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", dc.RATES)
@pytest.mark.parametrize("mutant", ["edge_moved", "weight_changed"])
def test_logmel_comparison_rejects_mutant(golden_dir, rate, mutant):
    """One band edge moved by one bin / one mel weight changed by 2^-12, on the full-scale white-noise row, at the widest bound
    the device tests use (device bound + 1, the estimate after the first hop); on the first hop alone too, which is all the
    per-rate device tests see."""
    white = dc.signals(golden_dir)[dc.K["white"]]
    want = dc.logmel64(white, rate)
    bound = dc.device_bound(rate) + 1
    dc.check_logmel("no mutant", want.astype(np.float32), want, bound)
    got = dc.logmel64(white, getattr(dc.filterbank(rate), mutant)()).astype(np.float32)
    with pytest.raises(AssertionError, match="ULP"):
        dc.check_logmel("mutant", got, want, bound)
    with pytest.raises(AssertionError, match="ULP"):
        dc.check_logmel("mutant, first hop", got[:1], want[:1], bound)


# ---- the estimator's second half ------------------------------------------------------------------------------------------------
def test_receive_mel_equals_receive_samples(golden_dir, oracle_default):
    """ReceiveSamples(pcm) == ReceiveMel(logmel(pcm)) bit for bit over 100 hops, both branches taken"""
    streams = dc.estimator_streams(golden_dir, 100)
    n_noise = n_update = 0
    for name in ("speech", "noise", "noise_then_speech", "swell", "zeros"):
        a, b = lyra_oracle.NoiseEstimator(oracle_default), lyra_oracle.NoiseEstimator(oracle_default)
        stream = lyra_oracle.Stream(oracle_default)
        for t, hop in enumerate(streams[name]):
            flag, mel = a.ReceiveSamples(hop)
            mel2 = stream.logmel(hop)
            assert np.array_equal(mel.view(np.uint32), mel2.view(np.uint32)), (name, t)
            assert b.ReceiveMel(mel2) == flag, (name, t)
            assert np.array_equal(a.noise_estimate().view(np.uint32), b.noise_estimate().view(np.uint32)), (name, t)
            assert np.array_equal(a.noise_bound().view(np.uint32), b.noise_bound().view(np.uint32)), (name, t)
            n_noise += flag
            n_update += not flag
    assert n_noise > 0 and n_update > 0, (n_noise, n_update)


# ---- resampler -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_rate,out_rate", dc.DESIGNS)
def test_resampler_chunked_equals_one_shot(in_rate, out_rate):
    """the oracle fed the chunk plan == the oracle fed everything at once == the numpy restatement chunk by chunk; both rails in
    the output; and the comparison used on the device rejects a dropped tap and a clip at -32767"""
    plan = dc.chunk_plan(in_rate, out_rate)
    up, down = dc.up_down(in_rate, out_rate)
    assert all(n % down == 0 and 1 <= n <= 960 and n * up // down <= 960 for n in plan) and plan[-1] == in_rate // 50
    x = dc.resampler_input(sum(plan), seed=in_rate + out_rate, down=down)
    one = lyra_oracle.Resampler(in_rate, out_rate).Resample(x)
    assert one.size == x.size * up // down
    lo, hi = dc.rails(one)
    assert lo > 0 and hi > 0, f"{in_rate} -> {out_rate}: {lo} samples at -32768, {hi} at 32767"
    ora, ref = lyra_oracle.Resampler(in_rate, out_rate), dc.ResamplerNp(in_rate, out_rate)
    mutants = {"tap 0 dropped": dc.ResamplerNp(in_rate, out_rate, drop_tap=0),
               "tap 17 dropped": dc.ResamplerNp(in_rate, out_rate, drop_tap=17),
               "clip at -32767": dc.ResamplerNp(in_rate, out_rate, clip_lo=-32767.0)}
    rejected = dict.fromkeys(mutants, 0)
    chunks = []
    for i, c in enumerate(dc.split(x, plan)):
        want = ora.Resample(c)
        assert want.size == c.size * up // down
        dc.same_samples(f"numpy resampler, chunk {i} of {c.size}", ref.Resample(c), want)
        for name, m in mutants.items():
            try:
                dc.same_samples(name, m.Resample(c), want)
            except AssertionError:
                rejected[name] += 1
        chunks.append(want)
    dc.same_samples("chunked against one shot", np.concatenate(chunks), one)
    assert all(n > 0 for n in rejected.values()), rejected


# ---- comfort noise ---------------------------------------------------------------------------------------------------------------
def test_comfort_noise_rails(oracle_exact):
    feats = dc.cng_features(oracle_exact)
    assert feats.shape == (5, 160) and 1.0 < feats[4].min() and feats[4].max() < 1.5
    ids = np.array([7, 0, 33, 12, 5], np.int32)
    want = dc.oracle_cng(oracle_exact, feats, ids)                      # [8][5][320]
    for r in dc.CNG_LOUD:
        lo, hi = dc.rails(want[:, r])
        assert lo > 0 and hi > 0, f"feature row {r}: {lo} samples at -32768, {hi} at 32767"
    assert dc.rails(want[:, 2])[0] > 0, "constant 1.3 does not reach -32768"
    assert np.abs(want[:, 0].astype(int)).max() < 100
    # the numpy restatement under the device's bound, and its mutant without the clip on the loud rows
    for r in range(5):
        g = dc.CngNp(dc.CNG_SEED ^ int(ids[r]))
        dc.within_one_lsb(f"numpy comfort noise, row {r}", np.stack([g.generate(feats[r]) for _ in range(dc.CNG_HOPS)]), want[:, r])
    for r in dc.CNG_LOUD:
        g = dc.CngNp(dc.CNG_SEED ^ int(ids[r]), clip=False)
        with pytest.raises(AssertionError, match="LSB"):
            dc.within_one_lsb("mutant", np.stack([g.generate(feats[r]) for _ in range(dc.CNG_HOPS)]), want[:, r])
