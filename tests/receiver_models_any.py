"""receiver_models.Device / Model for lyra_hip_decode_samples_any_dev: requests of any size up to four hops, where the model's
BufferedResampler holds samples back between calls (Model.call asserts that it never does).  No tests here."""
import numpy as np

from receiver_models import DEPTH, Device, Model


class DeviceAny(Device):
    """decode_samples_any_dev call by call, on receiver_models.Device's alternating buffers."""

    def call(self, rows, nbytes, n, read=True):
        torch, k = self.torch, self.k & 1
        self.k += 1
        B = self.ids.size
        self.pk[k].copy_(torch.from_numpy(np.ascontiguousarray(rows, np.uint8)))
        self.nb[k].copy_(torch.from_numpy(np.ascontiguousarray(nbytes, np.int32)))
        out = torch.zeros((B, n), dtype=torch.int16, device=self.dev) if n else None
        self.ctx.decode_samples_any_dev(self.d_ids, self.pk[k], self.nb[k], n, self.rate, out, self.isn[k], self.icn[k])
        if not read:
            return out
        self.ctx.synchronize()
        pcm = out.cpu().numpy() if n else np.zeros((B, 0), np.int16)
        return pcm, self.isn[k].cpu().numpy().copy(), self.icn[k].cpu().numpy().copy()


class ModelAny(Model):
    """Model without the empty-leftover rule; CnReach follows the model's leftover.  Counts what the calls went through."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.saw_rounds = [0] * 5        # calls (per row) whose internal length needed 0 .. 4 rounds
        self.saw_left = [0] * 3          # rows that ended a call holding 0 / 1 / 2 samples
        self.saw_left_only = 0           # rows served from the leftover alone

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
            n_int = dec.last_internal.size
            self.tally.check(pcm[r], want, self.reach[i](dec, n), f"{where}, row {r} (id {i}), n {n}")
            assert icn[r] == int(dec.is_comfort_noise()), f"{where}, row {r}: is_comfort_noise {icn[r]}, model {dec.is_comfort_noise()}"
            assert isn[r] == int(dec.is_noise), f"{where}, row {r}: is_noise"
            self.saw_cn += int(dec.is_comfort_noise())
            self.saw_mix += int(any(g and c for g, c, _, _ in dec.last_segments))
            self.saw_back += int(was_cn and not dec.is_comfort_noise())
            self.saw_two += int(len(dec.last_segments) >= 2)
            self.saw_rounds[(n_int + 319) // 320] += 1
            self.saw_left[dec.leftover.size] += 1
            self.saw_left_only += int(n > 0 and n_int == 0)
