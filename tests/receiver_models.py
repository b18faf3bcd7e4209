"""The receiver side of the reference model (oracle/lyra_codec_model.py) as the tests hold the device to it: CnReach, Tally, the
hop-synchronous receiver of decode_lossy_dev (LossyModel) and the receiver of any request size of decode_samples_dev (Device,
Model).  No tests here; torch and the oracle are imported inside the functions: a CPU test that needs CnReach loads neither."""
import numpy as np

from signals import _speech

BYTES = {64: 8, 120: 15, 184: 23}
ROW = 23      # LYRA_HIP_MAX_PACKET_BYTES
DEPTH = 4     # LYRA_HIP_DECODE_SAMPLES_FIFO
SEED = 0x4C797261   # the context's default comfort-noise seed; stream `id` draws from SEED ^ id
RS_REACH = 34   # an output sample of the codec's resampler reads the 35 newest input samples (radius 17, lyra_oracle.c)


def cn_flags(dec):
    """Per internal 16 kHz sample of dec's (RefLyraDecoder) last DecodeSamples call: True where comfort noise went into it,
    alone or cross-faded, from the model's per-segment record."""
    f = np.concatenate([np.full(max(g, c), c > 0) for g, c, _, _ in dec.last_segments] + [np.zeros(0, bool)])
    assert f.size == dec.last_internal.size, f"the model's segments cover {f.size} samples, its last call made {dec.last_internal.size}"
    return f


class CnReach:
    """The same per played sample, at any rate: which samples of DecodeSamples(n) comfort noise can reach -- at 16 kHz the
    ones it went into, at other rates the ones whose resampler window holds such a sample.  One per model decoder, called
    after each of its DecodeSamples calls; follows the model's resampler phase and its leftover."""

    def __init__(self, rate):
        self.rate, self.pos = rate, 0
        self.hist = np.zeros(RS_REACH, bool)
        self.pending = np.zeros(0, bool)

    def __call__(self, dec, n):
        f = cn_flags(dec)
        if self.rate == 16000:
            assert f.size == n, f"DecodeSamples({n}) at 16 kHz made {f.size} internal samples"
            return f
        buf = np.concatenate([self.hist, f])
        hit = np.array([buf[k:k + RS_REACH + 1].any() for k in range(f.size)], bool)
        if self.rate > 16000:
            ext = np.repeat(hit, self.rate // 16000)
        else:
            ext = hit[(self.pos + np.arange(f.size)) % (16000 // self.rate) == 0]
        self.hist, self.pos = buf[buf.size - RS_REACH:], self.pos + f.size
        self.pending = np.concatenate([self.pending, ext])
        out, self.pending = self.pending[:n], self.pending[n:]
        assert out.size == n, f"DecodeSamples({n}) at {self.rate} Hz: the reach of only {out.size} played samples is known"
        return out


class Tally:
    """Per-sample comparison against the reference model: EXACT where only the generative model speaks (no loss, and the
    concealment hops from zero features before any fade), within `cn_lsb` where comfort noise reaches (device
    fp64 sin / cos / exp against the host libm, test_resampler_cng.py: 1 LSB; behind a resampler a 1-LSB difference is
    spread over the samples of its window).  Counts what it saw, for the report and for the old overall bound."""

    def __init__(self, cn_lsb=1):
        self.cn_lsb = cn_lsb
        self.n_gen = self.n_cn = self.n_cn_diff = self.worst = 0

    def check(self, got, want, cn, where):
        got, want, cn = np.asarray(got), np.asarray(want), np.asarray(cn, bool)
        assert got.shape == want.shape == cn.shape, (where, "shapes of got, want, reach", got.shape, want.shape, cn.shape)
        d = np.abs(got.astype(np.int64) - want.astype(np.int64))
        bad = np.flatnonzero(d * ~cn)
        assert bad.size == 0, f"{where}: generative-only samples differ at {bad[:8].tolist()} by {d[bad[:8]].tolist()}"
        assert d.max(initial=0) <= self.cn_lsb, f"{where}: comfort-noise samples differ by {int(d.max())} LSB"
        self.n_gen += int((~cn).sum())
        self.n_cn += int(cn.sum())
        self.n_cn_diff += int((d > 0).sum())
        self.worst = max(self.worst, int(d.max(initial=0)))

    def exact_fraction(self):
        return 1.0 - self.n_cn_diff / max(1, self.n_gen + self.n_cn)

    def report(self, name):
        print(f"{name}: {self.n_gen} generative-only samples exact; {self.n_cn} comfort-noise samples, {self.n_cn_diff} "
              f"differ ({self.n_cn_diff / max(1, self.n_cn):.4%}), worst {self.worst} LSB")


# ---- the hop-synchronous receiver: decode_lossy_dev ---------------------------------------------------------------------------
def _lossy_run(ctx, ids, packets, mask, bits, rate):
    """decode_lossy_dev tick by tick; packets [T][B][bytes] uint8, mask [T][B] -> (pcm16, ext, is_noise, is_cn) per tick."""
    import torch
    dev = torch.device("cuda", 0)
    T, B = mask.shape
    n_ext = rate // 50
    d_ids = torch.from_numpy(np.asarray(ids, np.int32)).to(dev)
    pk = [torch.empty((B, BYTES[bits]), dtype=torch.uint8, device=dev) for _ in range(2)]
    nb = [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2)]
    o16 = [torch.empty((B, 320), dtype=torch.int16, device=dev) for _ in range(2)]
    oext = [torch.empty((B, n_ext), dtype=torch.int16, device=dev) for _ in range(2)]
    isn = [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2)]
    icn = [torch.empty(B, dtype=torch.int32, device=dev) for _ in range(2)]
    res = []
    for t in range(T):
        k = t & 1
        pk[k].copy_(torch.from_numpy(np.ascontiguousarray(packets[t])))
        nb[k].copy_(torch.from_numpy((mask[t].astype(np.int32) * BYTES[bits])))
        ctx.decode_lossy_dev(d_ids, pk[k], nb[k], bits, rate, o16[k], oext[k] if rate != 16000 else None, isn[k], icn[k])
        ctx.synchronize()
        res.append((o16[k].cpu().numpy().copy(), (oext[k] if rate != 16000 else o16[k]).cpu().numpy().copy(),
                    isn[k].cpu().numpy().copy(), icn[k].cpu().numpy().copy()))
    return res


class LossyModel:
    """B RefLyraDecoders driven as a hop-synchronous receiver, checked tick by tick against decode_lossy_dev's outputs
    (_lossy_run's tuple): the 16 kHz hop against the model's internal hop (Tally); at other rates the external hop bit for
    bit against the oracle resampler run over the device's OWN 16 kHz stream; is_comfort_noise() and the decoder-side
    estimator's is_noise at every tick."""

    def __init__(self, oracle, rate, ids):
        from oracle import lyra_codec_model as M, lyra_oracle
        self.rate, self.ids = rate, [int(i) for i in ids]
        self.decs = [M.RefLyraDecoder(oracle, rate, cng_seed=SEED ^ i) for i in self.ids]
        self.rs = [lyra_oracle.Resampler(16000, rate) for _ in self.ids] if rate != 16000 else None
        self.tally = Tally()
        self.saw_cn = self.saw_mix = self.saw_back = 0

    def tick(self, t, packets, mask, got):
        o16, ext, isn, icn = got
        for s, dec in enumerate(self.decs):
            if mask[s]:
                dec.SetEncodedPacket(packets[s])
            was_cn = dec.is_comfort_noise()
            dec.DecodeSamples(self.rate // 50)
            self.tally.check(o16[s], dec.last_internal, cn_flags(dec), f"tick {t}, row {s} (id {self.ids[s]}), 16 kHz")
            if self.rs is not None:
                assert np.array_equal(ext[s], self.rs[s].Resample(o16[s])), f"tick {t}, row {s}: {self.rate} Hz output"
            assert icn[s] == int(dec.is_comfort_noise()), f"tick {t}, row {s}: is_comfort_noise {icn[s]}, model {dec.is_comfort_noise()}"
            assert isn[s] == int(dec.is_noise), f"tick {t}, row {s}: is_noise"
            self.saw_cn += int(dec.is_comfort_noise())
            self.saw_mix += int(any(g and c for g, c, _, _ in dec.last_segments))
            self.saw_back += int(was_cn and not dec.is_comfort_noise())

    def check_estimates(self, ctx, where):
        est = ctx.noise_estimate(self.ids, side="decoder")
        for s, dec in enumerate(self.decs):
            assert np.allclose(est[s], dec.noise.noise_estimate(), rtol=1e-5, atol=1e-6), f"{where}, row {s}: estimate"


def _estimate_ticks(mask):
    """Every fifth tick, and the ticks that end a loss burst of some row."""
    back = np.zeros(mask.shape[0], bool)
    back[1:] = (mask[1:].astype(bool) & ~mask[:-1].astype(bool)).any(axis=1)
    return back | (np.arange(mask.shape[0]) % 5 == 4)


def _lossy_check(ctx, model, ids, packets, mask, bits):
    """_lossy_run tick by tick against LossyModel (and the decoder-side estimates on _estimate_ticks)."""
    est_at = _estimate_ticks(mask)
    for t in range(mask.shape[0]):
        got = _lossy_run(ctx, ids, packets[t:t + 1], mask[t:t + 1], bits, model.rate)[0]
        model.tick(t, packets[t], mask[t], got)
        if est_at[t]:
            model.check_estimates(ctx, f"tick {t}")


def _full_batch_mask(T, B, rng):
    """[T][B] 0/1 for a full batch: bursty random loss (two-state chains) everywhere, and on top
    - rows 0..7, the first four logmel_masked pairs: at every tick one pair each received / received, lost / received,
      received / lost and lost / lost (rotating every 6 ticks, so their runs of 12 lost reach pure comfort noise);
    - rows 8..11, one lossy_mix tile: all lost for 12 ticks, into comfort noise and back;
    - rows 12..15: 5 lost (recovery in the middle of the fade to comfort noise), later 8 lost, one received in the fade
      back, 3 lost again;
    - the last row (alone in the last logmel pair when B is odd) and the first row of each later plan block of 256: a
      12-hop run."""
    m = np.ones((T, B), np.uint8)
    state = rng.random(B) < 0.2
    for t in range(T):
        state = np.where(state, rng.random(B) < 0.6, rng.random(B) < 0.1)
        m[t] = ~state
    for t in range(T):
        for k in range(min(4, B // 2)):
            c = (k + t // 6) % 4
            m[t, 2 * k], m[t, 2 * k + 1] = c & 1 == 0, c & 2 == 0
    if B >= 16:
        m[:, 8:16] = 1
        m[10:22, 8:12] = 0
        m[3:8, 12:16] = 0; m[20:28, 12:16] = 0; m[29:32, 12:16] = 0
    for r in [B - 1] + list(range(256, B, 256)):
        m[:, r] = 1
        m[14:26, r] = 0
    return m


# ---- the receiver of any request size: decode_samples_dev ---------------------------------------------------------------------
def _model_packets(oracle, golden_dir, bits_per_stream, T, offset=0):
    """-> [T][n][23] uint8 rows and [n] sizes: every stream encoded at its own bitrate by the reference model's encoder"""
    from oracle import lyra_codec_model as M
    n = len(bits_per_stream)
    pcm = _speech(golden_dir, n, T, offset)
    rows = np.zeros((T, n, ROW), np.uint8)
    for s, bits in enumerate(bits_per_stream):
        enc = M.RefLyraEncoder(oracle, 16000, bits, False)
        for t in range(T):
            p = enc.Encode(pcm[t, s])
            rows[t, s, :p.size] = p
    return rows, np.array([BYTES[b] for b in bits_per_stream], np.int32)


class Device:
    """decode_samples_dev call by call on alternating device buffers (the calls of a run are NOT synchronised one by one
    unless the caller reads the result)."""

    def __init__(self, ctx, ids, rate):
        import torch
        self.torch, self.ctx, self.rate = torch, ctx, rate
        self.dev = torch.device("cuda", 0)
        self.set_ids(ids)
        self.k = 0

    def set_ids(self, ids):
        torch = self.torch
        self.ids = np.asarray(ids, np.int32)
        B = self.ids.size
        self.d_ids = torch.from_numpy(self.ids.copy()).to(self.dev)
        self.pk = [torch.zeros((B, ROW), dtype=torch.uint8, device=self.dev) for _ in range(2)]
        self.nb = [torch.zeros(B, dtype=torch.int32, device=self.dev) for _ in range(2)]
        self.isn = [torch.zeros(B, dtype=torch.int32, device=self.dev) for _ in range(2)]
        self.icn = [torch.zeros(B, dtype=torch.int32, device=self.dev) for _ in range(2)]

    def call(self, rows, nbytes, n, read=True):
        torch, k = self.torch, self.k & 1
        self.k += 1
        B = self.ids.size
        self.pk[k].copy_(torch.from_numpy(np.ascontiguousarray(rows, np.uint8)))
        self.nb[k].copy_(torch.from_numpy(np.ascontiguousarray(nbytes, np.int32)))
        out = torch.zeros((B, n), dtype=torch.int16, device=self.dev) if n else None
        self.ctx.decode_samples_dev(self.d_ids, self.pk[k], self.nb[k], n, self.rate, out, self.isn[k], self.icn[k])
        if not read:
            return out
        self.ctx.synchronize()
        pcm = out.cpu().numpy() if n else np.zeros((B, 0), np.int16)
        return pcm, self.isn[k].cpu().numpy().copy(), self.icn[k].cpu().numpy().copy()


class Model:
    """One RefLyraDecoder per stream id, with the bounded feature FIFO of the device call: a packet that finds DEPTH vectors
    waiting is not delivered.  seed: the comfort-noise seed of the context the streams were created in."""

    def __init__(self, oracle, rate, ids, seed=SEED):
        from oracle import lyra_codec_model as M
        self.M, self.oracle, self.rate, self.seed = M, oracle, rate, seed
        self.decs, self.reach = {}, {}
        for i in ids:
            self.reset(int(i))
        self.tally = Tally()
        self.saw_cn = self.saw_mix = self.saw_back = self.saw_two = self.dropped = 0

    def reset(self, i):
        self.decs[i] = self.M.RefLyraDecoder(self.oracle, self.rate, cng_seed=self.seed ^ i)
        self.reach[i] = CnReach(self.rate)

    def call(self, where, ids, rows, nbytes, n, got):
        pcm, isn, icn = got
        for r, i in enumerate(int(x) for x in ids):
            dec = self.decs[i]
            if nbytes[r] in (8, 15, 23):
                if len(dec.model.q) - (1 if dec.model.next > 0 else 0) >= DEPTH:
                    self.dropped += 1
                else:
                    dec.SetEncodedPacket(rows[r, :nbytes[r]])
            was_cn = dec.is_comfort_noise()
            want = dec.DecodeSamples(n)
            assert dec.leftover.size == 0, f"{where}, row {r}: the model holds {dec.leftover.size} samples back"
            self.tally.check(pcm[r], want, self.reach[i](dec, n), f"{where}, row {r} (id {i}), n {n}")
            assert icn[r] == int(dec.is_comfort_noise()), f"{where}, row {r}: is_comfort_noise {icn[r]}, model {dec.is_comfort_noise()}"
            assert isn[r] == int(dec.is_noise), f"{where}, row {r}: is_noise"
            self.saw_cn += int(dec.is_comfort_noise())
            self.saw_mix += int(any(g and c for g, c, _, _ in dec.last_segments))
            self.saw_back += int(was_cn and not dec.is_comfort_noise())
            self.saw_two += int(len(dec.last_segments) == 2)

    def check_estimates(self, ctx, where, ids):
        est = ctx.noise_estimate(np.asarray(ids, np.int32), side="decoder")
        for r, i in enumerate(int(x) for x in ids):
            assert np.allclose(est[r], self.decs[i].noise.noise_estimate(), rtol=1e-5, atol=1e-6), f"{where}, row {r}: estimate"
