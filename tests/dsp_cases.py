"""Inputs, references and comparisons for the four DSP kernels beside the networks -- log-mel with its estimator tail, the
resampler, the comfort noise -- shared by tests/test_dsp_refs_cpu.py and tests/test_gpu_dsp_edges.py.  No tests here.

LOGMEL_ORACLE_ULP: per filterbank rate, the oracle's worst distance from the float64 log-mel (logmel64) over the 14 signal
kinds of signals(), in float32 ULP of the real value, measured on the oracle alone and rounded up to two decimals
(test_dsp_refs_cpu.py asserts measured <= constant and >= 0.8 constant, so a stale table fails).  Where the figure comes
from: the oracle rounds the band sum to float32 (worth <= 0.05 ULP of the result: d log(m) / 10 of half an ULP of m), rounds
log() once to float32 (<= 1/2 ULP of a value near 12, which is up to 0.8 ULP of a result near 1.2 in its own binade after the
division) and rounds the division by 10.f (<= 1/2 ULP).
device_bound(rate) = ceil(LOGMEL_ORACLE_ULP[rate]) + 1: the device runs the oracle's float32 tail on a band sum that its
radix-4 FFT and its paired spectra form in another order; each is accurate to about 1e-13 relative, which can flip the one
float32 rounding of the band sum.  Never above the 4 ULP of tests/test_gpu_parity.py::test_logmel."""
import functools
import math
import os

import numpy as np

from oracle.logmel_np import MelFilterbank

RATES = (8000, 16000, 32000, 48000)
HOP, WINDOW, FFT, BINS, BANDS = 320, 640, 1024, 513, 160
T = 24
FLOOR = 500.0
SILENCE = np.float32(np.float32(np.log(np.float64(FLOOR))) / np.float32(10.0))     # the floored bands, as the float32 tail forms it

KINDS = ("white", "speech", "speech64", "dc_hi", "dc_lo", "square", "alternating", "zeros", "impulses", "pm1", "pm12", "pm40",
         "sine", "gated")
K = {name: i for i, name in enumerate(KINDS)}

LOGMEL_ORACLE_ULP = {8000: 1.26, 16000: 1.28, 32000: 1.29, 48000: 1.25}
PARITY_ULP = 4          # what the suite allowed before (test_gpu_parity.py::test_logmel)


def device_bound(rate):
    b = math.ceil(LOGMEL_ORACLE_ULP[rate]) + 1
    assert b <= PARITY_ULP, (rate, b)
    return b


# ---- signals ----------------------------------------------------------------------------------------------------------------
def _speech(golden_dir, n, at=4000):
    sp = np.load(os.path.join(golden_dir, "sample_wavs.npz"))["sample1_16kHz"].astype(np.int16)
    return sp[(at + np.arange(n)) % sp.size]


@functools.lru_cache(maxsize=None)
def signals(golden_dir, hops=T):
    """[14][hops][320] int16 in the order of KINDS, read-only: full-scale white noise, speech, speech // 64, DC at both rails,
    a +-full-scale square wave of period 160, +-full-scale alternating every sample, zeros, 40 impulses, uniform +-1 / +-12 /
    +-40 (the last straddles the 500 floor), a full-scale 1 kHz sine, full-scale noise gated on and off every other hop"""
    rng = np.random.default_rng(1848)
    n = hops * HOP
    i = np.arange(n)
    sp = _speech(golden_dir, n)
    imp = np.zeros(n, np.int16)
    at = np.sort(rng.choice(n, size=40, replace=False))
    imp[at] = rng.choice(np.array([32767, -32768, 1, -1, 12345], np.int16), size=at.size)
    gated = rng.integers(-32768, 32768, size=n, dtype=np.int16)
    gated[(i // HOP) % 2 == 1] = 0
    rows = [rng.integers(-32768, 32768, size=n, dtype=np.int16), sp, (sp.astype(np.int32) // 64).astype(np.int16),
            np.full(n, 32767, np.int16), np.full(n, -32768, np.int16),
            np.where((i // 80) % 2 == 0, 32767, -32768).astype(np.int16), np.where(i % 2 == 0, 32767, -32768).astype(np.int16),
            np.zeros(n, np.int16), imp, rng.integers(-1, 2, size=n).astype(np.int16), rng.integers(-12, 13, size=n).astype(np.int16),
            rng.integers(-40, 41, size=n).astype(np.int16),
            np.round(32767 * np.sin(2 * np.pi * 1000 * i / 16000)).astype(np.int16), gated]
    x = np.ascontiguousarray(np.stack(rows).reshape(len(KINDS), hops, HOP))
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def estimator_streams(golden_dir, hops):
    """dict name -> [hops][320] int16, read-only: what drives both branches of the estimator -- speech, stationary noise, white
    full scale, zeros, speech // 64, 60 hops of noise then speech, noise whose level swells from 0.2x to 6x over the run"""
    rng = np.random.default_rng(515)
    n = hops * HOP
    sp = _speech(golden_dir, n, at=0)
    noise = rng.normal(0, 300, n)
    swell = rng.normal(0, 300, n) * np.linspace(0.2, 6.0, n)
    out = {"speech": sp, "noise": noise, "white": rng.integers(-32768, 32768, size=n), "zeros": np.zeros(n),
           "speech64": sp.astype(np.int32) // 64, "noise_then_speech": np.concatenate([rng.normal(0, 300, 60 * HOP), sp[:n - 60 * HOP]]),
           "swell": swell}
    for k in out:
        out[k] = np.clip(out[k], -32768, 32767).astype(np.int16).reshape(hops, HOP)
        out[k].flags.writeable = False
    return out


# ---- the float64 log-mel ----------------------------------------------------------------------------------------------------
class Filterbank:
    """oracle/logmel_np.MelFilterbank of one rate as band / weight per bin; mutants are copies with one entry changed"""

    def __init__(self, rate):
        fb = MelFilterbank(BINS, rate, BANDS, 0.0, 0.495 * rate)
        self.rate, self.start, self.end = rate, fb.start, fb.end
        self.band, self.weight = fb.band.copy(), fb.weight.copy()

    def copy(self):
        c = object.__new__(Filterbank)
        c.rate, c.start, c.end, c.band, c.weight = self.rate, self.start, self.end, self.band.copy(), self.weight.copy()
        return c

    def matrix(self):
        """[160][513]: band c takes weight w of the bins whose lower band is c and 1 - w of those whose lower band is c - 1"""
        W = np.zeros((BANDS, BINS))
        for i in range(self.start, self.end + 1):
            ch = int(self.band[i])
            if ch >= 0:
                W[ch, i] += self.weight[i]
            if ch + 1 < BANDS:
                W[ch + 1, i] += 1.0 - self.weight[i]
        return W

    def edge_moved(self, band=80):
        """the first bin of `band` counted to the band below: one band edge off by one bin"""
        c = self.copy()
        i = int(np.flatnonzero(c.band == band)[0])
        c.band[i] = band - 1
        return c

    def weight_changed(self, delta=2.0 ** -12):
        """the weight of the middle bin changed by delta"""
        c = self.copy()
        c.weight[(c.start + c.end) // 2] += delta
        return c


@functools.lru_cache(maxsize=None)
def filterbank(rate):
    return Filterbank(rate)


_HANN = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WINDOW) / WINDOW)


def logmel64(hops, fb):
    """[n][320] int16, the hops of ONE stream from its start -> [n][160] float64: oracle/logmel_np.py carried in float64 to the
    end, log(max(mel, 500)) / 10 with no float32 rounding, for the filterbank fb (a Filterbank or a rate)"""
    fb = filterbank(fb) if isinstance(fb, int) else fb
    hops = np.asarray(hops)
    x = np.concatenate([np.zeros(HOP), hops.reshape(-1).astype(np.float64)])
    frames = np.stack([x[t * HOP:t * HOP + WINDOW] for t in range(hops.shape[0])]) * _HANN
    mag = np.abs(np.fft.rfft(frames, n=FFT, axis=1))
    return np.log(np.maximum(mag @ fb.matrix().T, FLOOR)) / 10.0


def ulp32(r):
    """the float32 ULP of the binade of the real value r"""
    _, e = np.frexp(np.abs(np.asarray(r, np.float64)))
    return np.ldexp(1.0, e - 24)


def distance(a, r):
    """of a float32 result a from the real value r, in ULP of r"""
    return np.abs(np.asarray(a, np.float32).astype(np.float64) - r) / ulp32(r)


def check_logmel(where, got, want, bound):
    """every float32 value of got within `bound` ULP of the float64 want (same shape) -> the worst distance"""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, (where, got.dtype, got.shape, want.shape)
    d = distance(got, want)
    if not (d <= bound).all():      # (a NaN fails too)
        at = tuple(int(v) for v in np.argwhere(~(d <= bound))[0])
        raise AssertionError(f"{where}: log-mel at {at} is {got[at]!r}, float64 reference {want[at]!r}: {d[at]:.2f} ULP, "
                             f"bound {bound}; {int((~(d <= bound)).sum())} values over it, worst {np.nanmax(d):.2f}")
    return float(d.max())


def ulps_apart(a, b):
    """float32 arrays of positive values -> how many float32 values lie between, elementwise"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def oracle_logmel(oracle, hops, rate):
    """the oracle's float32 log-mel of one stream's hops with the filterbank of `rate` (its estimator's own extractor)"""
    from oracle import lyra_oracle
    ne = lyra_oracle.NoiseEstimator(oracle, sample_rate_hz=rate)
    return np.stack([ne.ReceiveSamples(h)[1] for h in hops])


# ---- comparisons of samples ---------------------------------------------------------------------------------------------------
def same_samples(where, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (where, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        at = tuple(int(v) for v in np.argwhere(got != want)[0])
        raise AssertionError(f"{where}: sample {at} is {got[at]}, oracle {want[at]}; {int((got != want).sum())} samples differ")


def within_one_lsb(where, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.int16, (where, got.shape, want.shape, got.dtype)
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    if d.max() > 1:
        at = tuple(int(v) for v in np.argwhere(d > 1)[0])
        raise AssertionError(f"{where}: sample {at} is {got[at]}, oracle {want[at]}; {int((d > 1).sum())} samples more than 1 LSB off")


def rails(x):
    x = np.asarray(x)
    return int((x == -32768).sum()), int((x == 32767).sum())


# ---- resampler ----------------------------------------------------------------------------------------------------------------
DESIGNS = ((8000, 16000), (32000, 16000), (48000, 16000), (16000, 8000), (16000, 32000), (16000, 48000))
CHUNKS = (1, 2, 3, 5, 7, 8, 16, 17, 33, 34, 35, 63, 64, 65, 100, 127, 129, 255, 257, 319, 320)
RS_TAPS = 35
MAX_SAMPLES = 960


def up_down(in_rate, out_rate):
    g = math.gcd(in_rate, out_rate)
    return out_rate // g, in_rate // g


def chunk_plan(in_rate, out_rate):
    """input samples per call: CHUNKS times the decimation factor, capped so that neither side of a call exceeds 960 samples,
    then one whole hop -- the 16-byte load path behind the scalar one on the same history"""
    up, down = up_down(in_rate, out_rate)
    cap = min(MAX_SAMPLES, MAX_SAMPLES * down // up) // down * down
    return [min(c * down, cap) for c in CHUNKS] + [in_rate // 50]


def resampler_input(n, seed, down=1, burst_at=700, burst=40):
    """[n] int16: full-scale white noise with a burst of 40 samples of +-full scale alternating every sample.  A decimator
    removes that burst whatever its length (it lies at the input's Nyquist rate) and full-scale noise behind its filter seldom
    reaches a rail, so for down > 1 a second burst alternates in runs of 2 * down samples, 40 runs long: a quarter of the output
    rate, inside the pass band, whose overshoot puts both rails in the output."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, size=n, dtype=np.int16)
    x[burst_at:burst_at + burst] = np.where(np.arange(burst) % 2 == 0, 32767, -32768)
    if down > 1:
        run, at = 2 * down, burst_at + 3 * burst
        x[at:at + burst * run] = np.where((np.arange(burst * run) // run) % 2 == 0, 32767, -32768)
    return x


def split(x, plan):
    at = np.concatenate([[0], np.cumsum(plan)])
    return [x[at[i]:at[i + 1]] for i in range(len(plan))]


class ResamplerNp:
    """oracle/lyra_oracle.c lo_resample in numpy float32: the oracle's coefficient table, taps oldest first, every product
    rounded, then the clip and the truncating conversion.  drop_tap / clip_lo: the mutants."""

    def __init__(self, in_rate, out_rate, drop_tap=None, clip_lo=-32768.0):
        import ctypes as C
        from oracle import lyra_oracle
        up, down, radius = C.c_int(), C.c_int(), C.c_int()
        coef = np.zeros((3, 40), np.float32)
        lyra_oracle.lib().lo_resampler_design(in_rate, out_rate, C.byref(up), C.byref(down), C.byref(radius), coef.ctypes.data)
        assert (up.value, down.value) == up_down(in_rate, out_rate) and 2 * radius.value + 1 == RS_TAPS
        self.up, self.down, self.coef = up.value, down.value, coef
        self.hist, self.in_pos = np.zeros(RS_TAPS - 1, np.float32), 0
        self.drop_tap, self.clip_lo = drop_tap, np.float32(clip_lo)

    def Resample(self, x):
        x = np.asarray(x, np.int16)
        buf = np.concatenate([self.hist, x.astype(np.float32)])
        ks = np.arange(x.size)
        if self.down > 1:
            ks = ks[(self.in_pos + ks) % self.down == 0]
        out = np.zeros((ks.size, self.up), np.int16)
        for p in range(self.up):
            acc = np.zeros(ks.size, np.float32)
            for j in range(RS_TAPS):
                if j != self.drop_tap:
                    acc = acc + self.coef[p, j] * buf[ks + j]
            out[:, p] = np.clip(acc, self.clip_lo, np.float32(32767.0)).astype(np.int16)
        self.hist = buf[x.size:]
        self.in_pos += x.size
        return out.reshape(-1)


# ---- comfort noise ------------------------------------------------------------------------------------------------------------
CNG_CONSTANT = (0.6215, 1.0, 1.3, 1.5)      # the span of the oracle's features over signals(): 0.6215 .. 1.59
CNG_HOPS, CNG_SEED = 8, 1234
CNG_LOUD = (3, 4)                           # rows of cng_features() that put samples on both rails
NOISE_HOPS = 40


def white_hops(hops=NOISE_HOPS, seed=77):
    return np.random.default_rng(seed).integers(-32768, 32768, size=(hops, HOP), dtype=np.int16)


def cng_features(oracle):
    """[5][160] float32: the four constant rows, then the oracle's noise estimate of 40 hops of full-scale white noise"""
    from oracle import lyra_oracle
    ne = lyra_oracle.NoiseEstimator(oracle)
    for h in white_hops():
        ne.ReceiveSamples(h)
    return np.stack([np.full(BANDS, c, np.float32) for c in CNG_CONSTANT] + [ne.noise_estimate()])


def oracle_cng(oracle, features, ids, hops=CNG_HOPS, seed=CNG_SEED):
    """[hops][B][320]: the oracle's generators of the streams `ids` of a context seeded `seed`, row b fed features[b] every hop"""
    from oracle import lyra_oracle
    gens = [lyra_oracle.ComfortNoiseGenerator(oracle, seed=seed ^ int(i)) for i in ids]
    return np.stack([np.stack([g.generate(f) for g, f in zip(gens, features)]) for _ in range(hops)])


_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


class CngNp:
    """oracle/lyra_oracle.c lo_cng_generate in numpy float64 (numpy's inverse FFT in place of the oracle's, so equal to it
    within the 1 LSB the device is held to, not bit for bit).  clip=False: the mutant, int16 wrap-around."""

    def __init__(self, seed, clip=True):
        self.seed, self.hop, self.clip = seed, 0, clip
        self.ola = np.zeros(FFT)
        fb = filterbank(16000)
        self.fb, self.W = fb, fb.matrix().sum(axis=1)
        self.win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(FFT) / FFT)

    def generate(self, features):
        f = np.asarray(features, np.float32)
        mel = np.exp((f * np.float32(10.0)).astype(np.float64)).astype(np.float32).astype(np.float64)
        gain = math.sqrt(1024.0 * 320.0 / (384.0 * 240.0))
        spec = np.zeros(BINS, np.complex128)
        fb = self.fb
        for i in range(fb.start, fb.end + 1):
            ch, w, v = int(fb.band[i]), fb.weight[i], 0.0
            if ch >= 0 and self.W[ch] > 0.0:
                v += w * mel[ch] / self.W[ch]
            if ch + 1 < BANDS and self.W[ch + 1] > 0.0:
                v += (1.0 - w) * mel[ch + 1] / self.W[ch + 1]
            r = _splitmix64(self.seed ^ _splitmix64((self.hop * 1024 + i) & _M64))
            ang = (r >> 11) * (1.0 / 9007199254740992.0) * 2.0 * math.pi
            spec[i] = v * gain * complex(math.cos(ang), math.sin(ang))
        spec[0] = spec[0].real
        spec[BINS - 1] = spec[BINS - 1].real
        self.ola += np.fft.irfft(spec, n=FFT) * self.win
        y = self.ola[:HOP]
        out = np.clip(y, -32768.0, 32767.0).astype(np.int16) if self.clip else y.astype(np.int64).astype(np.int16)
        self.ola = np.concatenate([self.ola[HOP:], np.zeros(HOP)])
        self.hop += 1
        return out
