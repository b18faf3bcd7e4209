"""Input signals (from tests/golden/sample_wavs.npz) and loss patterns shared by the tests: numpy only, no device, no tests."""
import os

import numpy as np

RATES = (8000, 16000, 32000, 48000)
EXT_ROW = 960                                  # LYRA_HIP_MAX_EXT_HOP: a row of external-rate samples
SHORT = (("S", (3, 6)), ("Z", (4, 7)), ("N", (2, 4)), ("Z", (3, 6)))      # segment kinds and lengths in hops [lo, hi)
LONG = (("S", (10, 18)), ("Z", (5, 11)), ("N", (3, 6)), ("Z", (4, 9)))


def _golden_pair(golden_dir):
    """both golden recordings one behind the other, as int32"""
    w = np.load(os.path.join(golden_dir, "sample_wavs.npz"))
    return np.concatenate([w["sample1_16kHz"], w["sample2_16kHz"]]).astype(np.int32)


def _looped(golden_dir, rng, n):
    """n samples of the golden pair times 3, looped from an offset drawn from rng (its first draw)"""
    src = _golden_pair(golden_dir)
    return src[(int(rng.integers(0, src.size)) + np.arange(n)) % src.size] * 3


def _segments(x, rng, pattern):
    """in place on [hops][.]: segments of speech (S, left alone), digital silence (Z) and +-12 noise (N), lengths from rng"""
    at = k = 0
    while at < len(x):
        kind, (lo, hi) = pattern[k % len(pattern)]
        n = int(rng.integers(lo, hi))
        if kind == "Z":
            x[at:at + n] = 0
        elif kind == "N":
            x[at:at + n] = rng.integers(-12, 13, x[at:at + n].shape)
        at += n; k += 1


# ---- per-stream speech for the per-row calls: [T][n][320] --------------------------------------------------------------------
def _speech(golden_dir, n, T, offset=0):
    sp = np.load(os.path.join(golden_dir, "sample_wavs.npz"))["sample1_16kHz"].astype(np.int16)
    out = np.empty((T, n, 320), np.int16)
    for s in range(n):
        start = (offset + 2357 * s) % (sp.size - T * 320)
        out[:, s] = sp[start:start + T * 320].reshape(T, 320)
    return out


def _pcm_rows(golden_dir, B, T, rates, silent_every, seed, fill):
    """[T][B][960] int16: row b holds rates[b] / 50 samples of speech at its rate (repeated / decimated 16 kHz samples:
    any int16 input is a valid hop), `fill` behind them; every silent_every-th stream is silent from hop 5 on."""
    pcm = _speech(golden_dir, B, T, offset=seed)
    if silent_every:
        pcm[5:, ::silent_every] = 0
    out = np.full((T, B, EXT_ROW), fill, np.int16)
    for b, r in enumerate(rates):
        if r in RATES:
            out[:, b, :r // 50] = np.repeat(pcm[:, b], r // 16000, axis=1) if r >= 16000 else pcm[:, b, ::2]
    return out


def synth(B, T, seed):
    """[T][B][320] full-scale white noise"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(-32768, 32768, size=(T, B, 320)).astype(np.int16)


# ---- one stream's hops for the span calls: [hops][rate / 50] -----------------------------------------------------------------
def _speech_hops(golden_dir, hops, seed, half_silent=False):
    """[hops][320] at 16 kHz from the golden recordings; half_silent: segments of speech, digital silence and +-12 noise"""
    rng = np.random.default_rng(seed)
    x = _looped(golden_dir, rng, hops * 320).reshape(hops, 320)
    if half_silent:
        _segments(x, rng, LONG)
    return np.clip(x, -32768, 32767).astype(np.int16)


def _audio_spans(golden_dir, hops, seed):
    """speech of the two golden recordings, looped from a seed-dependent offset, with a little noise on top: [hops][320]"""
    rng = np.random.default_rng(seed)
    src = _golden_pair(golden_dir)
    x = src[(int(rng.integers(0, src.size)) + np.arange(hops * 320)) % src.size] + rng.integers(-200, 201, hops * 320)
    return np.clip(x, -32768, 32767).astype(np.int16).reshape(hops, 320)


def _audio_dtx(golden_dir, hops, rate, seed):
    """[hops][rate / 50]: the golden recordings read as a signal at `rate` from a seed-dependent offset, in segments of speech
    (S), digital silence (Z) and +-12 noise (N)"""
    rng = np.random.default_rng(seed)
    hop = rate // 50
    x = _looped(golden_dir, rng, hops * hop).reshape(hops, hop)
    _segments(x, rng, SHORT if hops < 100 else LONG)
    return np.clip(x, -32768, 32767).astype(np.int16)


def _audio_ext(golden_dir, hops, rate, seed):
    """[hops][rate / 50]: the golden recordings' samples read as a signal at `rate`, looped from a seed-dependent offset, with
    noise and a few full-scale bursts on top (the resampler's clip is part of what is compared)"""
    rng = np.random.default_rng(seed)
    n = hops * (rate // 50)
    x = _looped(golden_dir, rng, n) + rng.integers(-300, 301, n)
    for at in rng.integers(0, max(n - 40, 1), 3 if n > 40 else 0):
        x[at:at + 40] = rng.choice([-40000, 40000], 40)
    return np.clip(x, -32768, 32767).astype(np.int16).reshape(hops, rate // 50)


def _plain(golden_dir, hops, rate, seed):
    """[hops][rate / 50]: the golden recordings read as a signal at `rate` from a seed-dependent offset"""
    hop = rate // 50
    x = _looped(golden_dir, np.random.default_rng(seed), hops * hop).reshape(hops, hop)
    return np.clip(x, -32768, 32767).astype(np.int16)


def _pattern(golden_dir, kinds, rate, seed):
    """_plain with the hops marked "Z" in `kinds` zeroed"""
    x = _plain(golden_dir, len(kinds), rate, seed)
    for h, kind in enumerate(kinds):
        if kind == "Z":
            x[h] = 0
    return x


# ---- loss patterns ----------------------------------------------------------------------------------------------------------
def _patterns(T):
    """[T][4] 0/1: loss from the first hop then bursts; single losses; bursts of 3; a 12-hop run (pure comfort noise),
    then 5 lost (recovery in the middle of the fade to comfort noise), then 7 lost (recovery inside the fade back)."""
    m = np.ones((T, 4), np.uint8)
    m[:3, 0] = 0; m[9:11, 0] = 0; m[20:24, 0] = 0
    m[4::6, 1] = 0
    for a in (2, 11, 20, 29):
        m[a:a + 3, 2] = 0
    m[1:13, 3] = 0; m[15:20, 3] = 0; m[21:28, 3] = 0
    return m


def _gilbert(rng, T, B, p_loss=0.1, p_stay=0.75):
    """[T][B] 0/1 received; bursty loss, and rows 0..15 lose ticks 4..15 (comfort noise, then the fade back)."""
    m = np.ones((T, B), np.uint8)
    lost = rng.random(B) < p_loss
    for t in range(T):
        lost = np.where(lost, rng.random(B) < p_stay, rng.random(B) < p_loss * (1 - p_stay) / (1 - p_loss))
        m[t] = ~lost
    m[4:16, :min(16, B)] = 0
    m[20:27, 16:min(24, B)] = 0
    return m


def _gilbert_ticks(rng, n, recover_from=0.05):
    """[n] bool received: one two-state chain whose loss and recovery probabilities are drawn from rng first"""
    p_loss, p_recover = rng.uniform(0.02, 0.5), rng.uniform(recover_from, 0.9)
    lost, out = rng.random() < 0.3, []
    for _ in range(n):
        lost = (rng.random() >= p_recover) if lost else (rng.random() < p_loss)
        out.append(not lost)
    return np.array(out, bool)


def _random_packets(rng, T, B):
    """[T][B][23] random packets, sizes 0 / 8 / 15 / 23 from a bursty loss pattern; streams 0..15 lose ticks 4..15."""
    rx = _gilbert(rng, T, B)
    sizes = rng.choice((8, 15, 23), size=(T, B)).astype(np.int32) * rx
    return rng.integers(0, 256, size=(T, B, 23)).astype(np.uint8), sizes


def _bursts(n, *at_len):
    """[n] bool received, False on the bursts (first, length)"""
    rx = np.ones(n, bool)
    for at, length in at_len:
        rx[at:at + length] = False
    return rx


def _stretches(mask):
    """[(first, one past last)] of the runs of True"""
    edges = np.flatnonzero(np.diff(np.concatenate([[0], mask.astype(np.int8), [0]])))
    return list(zip(edges[::2], edges[1::2]))


def _long_trace(plan_of):
    """350 frames: isolated losses, bursts of 3, 4, 5 (both sides of the 4-hop concealment limit), 8, 12 and 20 (run_gen == 0
    ticks, full comfort noise), then -- placed on the call's plan (plan_of(trace) -> (plan, the span's first buffer frame); the
    span is the call's first), which bursts of at most 6 do not move -- a burst of 5 that starts inside a lane chunk's warm-up
    and one that straddles a chunk boundary"""
    import lyra_amd.codec as codec
    n = 350
    rx = _bursts(n, (30, 1), (34, 1), (45, 3), (60, 4), (75, 5), (95, 8), (140, 12), (200, 20), (260, 1), (300, 9))
    plan, first = plan_of(rx)
    W = codec.span_warmup_frames("decoder")
    lane_chunks = [c for c in plan["chunks"] if c["span"] == 0 and c["n_warmup"] > 0]
    assert len(lane_chunks) >= 2, "the long span is not cut into lane chunks"
    gen = plan["gen_frames"] - first   # compacted index -> frame of the span
    def clear(f):   # ten received frames on either side: the new burst merges with no other
        return f - 10 >= 0 and f + 15 <= n and rx[f - 10:f + 15].all()
    warm = [int(gen[g]) for c in lane_chunks for g in range(int(c["first_frame"]) - W + 2, int(c["first_frame"]) - 8)
            if clear(int(gen[g]))]
    assert warm, "no room for a burst inside a warm-up"
    rx[warm[0]:warm[0] + 5] = False
    edge = [int(gen[int(c["first_frame"])]) - 2 for c in lane_chunks if clear(int(gen[int(c["first_frame"])]) - 2)]
    assert edge, "no room for a burst across a chunk boundary"
    rx[edge[-1]:edge[-1] + 5] = False
    return rx


# ---- WAV files --------------------------------------------------------------------------------------------------------------
def _write_wav(path, pcm, rate=16000):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
        w.writeframes(np.asarray(pcm, np.int16).tobytes())


def _read_wav(path, want_rate=None):
    """-> (samples, rate) of a mono 16-bit file; want_rate: asserted, and the samples alone are returned"""
    import wave
    with wave.open(str(path), "rb") as w:
        assert w.getnchannels() == 1 and w.getsampwidth() == 2, f"{path}: {w.getnchannels()} channels of {w.getsampwidth()} bytes"
        pcm, rate = np.frombuffer(w.readframes(w.getnframes()), np.int16), w.getframerate()
    assert want_rate in (None, rate), f"{path}: {rate} Hz, not {want_rate}"
    return (pcm, rate) if want_rate is None else pcm
