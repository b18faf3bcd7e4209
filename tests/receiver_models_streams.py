"""receiver_models_any.DeviceAny / ModelAny for lyra_hip_decode_samples_streams_dev: a sample rate and a request size per
stream in one call.  ModelStreams keeps one ModelAny per rate over the ids at that rate; DeviceStreams drives the call with
packed (or any other) offsets; uniform_by_class is the same work as one decode_samples_any_dev call per (rate, size) class.
No tests here."""
import numpy as np

from receiver_models import ROW
from receiver_models_any import DeviceAny, ModelAny

STRIDE = 4 * 960      # LYRA_HIP_DECODE_SAMPLES_MAX_HOPS * LYRA_HIP_MAX_EXT_HOP: a row's place when no offsets are given
CANARY = -21555       # what DeviceStreams fills its output buffer with before every call
RATES = (8000, 16000, 32000, 48000)


def rounds(n, rate):
    """ds_any_rounds restated: hops of internal samples that n samples at `rate` can need"""
    return (-(-n * 16000 // rate) + 319) // 320


def batch_rounds(sizes, rates):
    """dss_batch_rounds restated: the rounds a batch needs, at least 1, over the rows that are valid requests"""
    return max([1] + [rounds(int(n), int(r)) for n, r in zip(sizes, rates) if r in RATES and 0 <= n <= 4 * r // 50])


def packed(sizes):
    """dss_packed_offsets restated -> (offsets, total)"""
    sizes = np.maximum(np.asarray(sizes, np.int64), 0)
    return np.concatenate([[0], np.cumsum(sizes)[:-1]]), int(sizes.sum())


class DeviceStreams:
    """decode_samples_streams_dev call by call.  call() -> (list of B int16 arrays, is_noise, is_comfort_noise); .last is the
    whole output buffer of the last call as numpy, CANARY wherever nothing was written."""

    def __init__(self, ctx, ids, rates):
        import torch
        self.torch, self.ctx = torch, ctx
        self.dev = torch.device("cuda", 0)
        self.ids = np.asarray(ids, np.int32)
        assert 0 <= self.ids.min() and self.ids.max() < ctx.max_streams, "the _dev calls do not check stream ids"
        self.rates = np.asarray(rates, np.int32)
        self.d_ids = torch.from_numpy(self.ids.copy()).to(self.dev)
        self.k = 0

    def call(self, rows, nbytes, sizes, offsets="packed", max_hops=None, n_pcm=None, rates=None, buffer_samples=None):
        """offsets: "packed" (rows back to back), None (the call's default stride) or an int array; n_pcm: how much of the
        buffer the call is told about (default: all of it); buffer_samples: the buffer's real size (default: what the layout
        needs)"""
        torch, B = self.torch, self.ids.size
        sizes = np.asarray(sizes, np.int32)
        rates = self.rates if rates is None else np.asarray(rates, np.int32)
        if isinstance(offsets, str):
            offs, total = packed(sizes)
        elif offsets is None:
            offs, total = np.arange(B, dtype=np.int64) * STRIDE, B * STRIDE
        else:
            offs = np.asarray(offsets, np.int64)
            total = int(max([0] + [o + max(int(n), 0) for o, n in zip(offs, sizes)]))
        size = max(1, total if buffer_samples is None else buffer_samples)
        out = torch.full((size,), CANARY, dtype=torch.int16, device=self.dev)
        to = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(self.dev)
        isn = torch.full((B,), -7, dtype=torch.int32, device=self.dev)
        icn = torch.full((B,), -7, dtype=torch.int32, device=self.dev)
        self.ctx.decode_samples_streams_dev(self.d_ids, to(rows, np.uint8), to(nbytes, np.int32), to(rates, np.int32),
                                            to(sizes, np.int32), batch_rounds(sizes, rates) if max_hops is None else max_hops,
                                            out, None if offsets is None else to(offs, np.int32), isn, icn,
                                            n_pcm_samples=total if n_pcm is None and buffer_samples is None else n_pcm)
        self.ctx.synchronize()
        self.last = out.cpu().numpy()
        self.offs = offs
        pcm = [self.last[o:o + n].copy() if n > 0 and 0 <= o and o + n <= self.last.size else np.zeros(0, np.int16)
               for o, n in zip(offs, sizes)]
        return pcm, isn.cpu().numpy(), icn.cpu().numpy()


def uniform_by_class(ctx, ids, rates, rows, nbytes, sizes):
    """The same request as one decode_samples_any_dev call per (rate, size) class -> what DeviceStreams.call returns"""
    ids, rates, sizes = np.asarray(ids, np.int32), np.asarray(rates), np.asarray(sizes)
    rows, nbytes = np.asarray(rows), np.asarray(nbytes)
    B = ids.size
    assert 0 <= ids.min() and ids.max() < ctx.max_streams, "the _dev calls do not check stream ids"
    pcm, isn, icn = [None] * B, np.zeros(B, np.int32), np.zeros(B, np.int32)
    for rate, n in sorted({(int(r), int(n)) for r, n in zip(rates, sizes)}):
        sel = np.flatnonzero((rates == rate) & (sizes == n))
        p, a, b = DeviceAny(ctx, ids[sel], rate).call(rows[sel], nbytes[sel], n)
        for k, s in enumerate(sel):
            pcm[s] = p[k]
        isn[sel], icn[sel] = a, b
    return pcm, isn, icn


class ModelStreams:
    """One ModelAny per rate over the ids at that rate."""

    def __init__(self, oracle, ids, rates):
        self.ids = [int(i) for i in ids]
        self.rate_of = {int(i): int(r) for i, r in zip(ids, rates)}
        self.models = {r: ModelAny(oracle, r, [i for i in self.ids if self.rate_of[i] == r]) for r in sorted(set(self.rate_of.values()))}

    def call(self, where, ids, rows, nbytes, sizes, got):
        """Every row through its rate's model, one row at a time: rows of one rate may differ in size."""
        pcm, isn, icn = got
        for r, i in enumerate(int(x) for x in ids):
            m = self.models[self.rate_of[i]]
            m.call(where, [i], rows[r:r + 1], nbytes[r:r + 1], int(sizes[r]), (pcm[r][None], isn[r:r + 1], icn[r:r + 1]))

    def leftover(self, i):
        return self.models[self.rate_of[int(i)]].decs[int(i)].leftover.size

    def check_estimates(self, ctx, where):
        for r, m in self.models.items():
            m.check_estimates(ctx, f"{where}, {r} Hz", [i for i in self.ids if self.rate_of[i] == r])

    @property
    def dropped(self):
        return sum(m.dropped for m in self.models.values())
