"""The oracle's side of the stream-state comparisons, beside tests/state_bridge.py: oracle streams driven like the device, the
same hop on the device, blobs against oracle state tensor by tensor, and the directed states.  No tests here.

A_T: the largest magnitude each fp32 tensor reaches in the oracle (mode xnnpack) during the 37 hops of the full-scale
white-noise stream (stream 0 of _inputs), measured on the reference only and rounded up to three digits
(tests/test_gpu_state_vs_oracle.py asserts it).  The directed states draw fp32 state uniform in +-k A_t, k = 1 or 8."""
import os

import numpy as np

import state_bridge

BITS, NBYTES = 184, 23
MODES = ["xnnpack", "exact", "gemmlowp_double", "builtin_mixed"]
TRACE_CAP = 16384
ENC_INT8_TAPS, DEC_INT8_TAPS = (10, 11, 12, 13), (2, 3, 4)      # positions of the int8 taps among a frame's trace taps

A_T = {"e_first": 1, "e_r0[0]": 9.3, "e_r0[1]": 86.1, "e_r0[2]": 119, "e_d0": 95.1, "e_r1[0]": 364, "e_r1[1]": 368,
       "e_r1[2]": 757, "e_d1": 747, "e_r2[0]": 2000, "d_head": 41.3, "d_up0[0]": 15.2, "d_up0[1]": 6.33, "d_up0[2]": 13.7,
       "d_up0[3]": 20.4, "d_up1[0]": 5.37, "d_up1[1]": 22.2, "d_r1[0]": 22.1, "d_r1[1]": 45.9, "d_r1[2]": 43.6, "d_up2":
       2.74, "d_r2[0]": 5.93, "d_r2[1]": 6.81, "d_r2[2]": 26.5, "d_up3": 0.737}
K_EVEN, K_ODD = 1, 8
N_DIRECTED = 32


def _inputs(golden_dir, hops):
    """[hops][8][320] int16, one input kind per stream: full-scale white noise, speech, speech / 64, DC +32767, DC -32768,
    a +-full-scale square wave of period 160 samples, digital silence, impulses"""
    rng = np.random.default_rng(1848)
    n = hops * 320
    sp = np.load(os.path.join(golden_dir, "sample_wavs.npz"))["sample1_16kHz"].astype(np.int16)[4000:4000 + n]
    assert sp.size == n, f"the golden recording holds {sp.size} samples behind sample 4000, {n} wanted"
    imp = np.zeros(n, np.int16)
    at = np.sort(rng.choice(n, size=3 * hops, replace=False))
    imp[at] = rng.choice(np.array([32767, -32768, 1, -1, 12345], np.int16), size=at.size)
    sq = np.where((np.arange(n) // 80) % 2 == 0, 32767, -32768).astype(np.int16)
    x = np.stack([rng.integers(-32768, 32768, size=n, dtype=np.int16), sp, (sp.astype(np.int32) // 64).astype(np.int16),
                  np.full(n, 32767, np.int16), np.full(n, -32768, np.int16), sq, np.zeros(n, np.int16), imp])
    return np.ascontiguousarray(x.reshape(8, hops, 320).transpose(1, 0, 2))


class OracleSide:
    """n oracle streams driven like the device: per hop log-mel + encode at 184 bits on the rows that encode, decode of the
    given packets on every row"""

    def __init__(self, oracle, n, trace=False):
        from oracle import lyra_oracle
        self.o = oracle
        self.s = [lyra_oracle.Stream(oracle, trace_cap=TRACE_CAP if trace else 0) for _ in range(n)]
        self.enc_taps = self.dec_taps = None

    def encode(self, pcm, rows):
        out = np.zeros((len(rows), NBYTES), np.uint8)
        self.enc_taps = []
        for k, r in enumerate(rows):
            self.s[r].logmel(pcm[k])
            out[k] = self.o.pack(self.o.rvq_encode(self.s[r].encode(pcm[k]), 46), 46)[0]
            if self.s[r].trace is not None:
                self.enc_taps.append(self.s[r].taps())
        return out

    def decode(self, packets):
        out = np.zeros((len(self.s), 320), np.int16)
        self.dec_taps = []
        for r, s in enumerate(self.s):
            out[r] = s.decode(self.o.rvq_decode(self.o.unpack(packets[r], 46))[0])
            if s.trace is not None:
                self.dec_taps.append(s.taps())
        return out

    def states(self):
        return [s.state() for s in self.s]


def _device_hop(ctx, ids, enc_rows, pcm, packets_for_the_rest):
    """the same hop on the device -> (packets of the encoding rows, PCM of every row)"""
    enc_ids = [ids[r] for r in enc_rows]
    pk = np.zeros((0, NBYTES), np.uint8)
    if enc_rows:
        ctx.logmel(pcm, enc_ids)
        pk = ctx.encode(pcm, BITS, enc_ids)
    allpk = np.concatenate([pk, packets_for_the_rest]) if len(packets_for_the_rest) else pk
    return pk, allpk, ctx.decode(allpk, BITS, ids)


def _compare_states(bridge, blobs, want, frames_enc, frames_dec, where):
    """every blob row against the oracle stream of the same row: tensors, padding, phase words"""
    pad = bridge.padding()
    for r, (blob, st) in enumerate(zip(blobs, want)):
        d = bridge.first_difference(bridge.from_blob(blob), st)
        assert d is None, f"{where}, stream row {r}: {d}"
        assert not blob[pad].any(), f"{where}, stream row {r}: padding byte {int(np.flatnonzero((blob != 0) & pad)[0])} is not zero"
        fe, fd = frames_enc[r] % 18, frames_dec[r] % 18
        assert bridge.phases(blob) == {state_bridge.R_E1: fe, state_bridge.R_E2: fe, state_bridge.R_D0: fd,
                                       state_bridge.R_D1: fd}, f"{where}, stream row {r}: phase words {bridge.phases(blob)}"


def _same_rows(where, what, got, want):
    if not np.array_equal(got, want):
        r = int(np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))[0])
        c = int(np.flatnonzero(got[r] != want[r])[0])
        raise AssertionError(f"{where}: {what} of stream row {r} differs first at {c}: device {got[r][c]}, oracle {want[r][c]}")


def directed_states(bridge, seed=424242):
    """-> (states [32] of dicts, phase_enc [32], phase_dec [32]).  int8 tensors: codes uniform over all 256 values (streams
    0-23); streams 24-31 hold every int8 tensor constant at -128, at 127, at its zero point, or alternating -128 / 127 by row
    (two streams each); fp32 tensors uniform in +-k A_t, k = 1 on even and 8 on odd streams; mel_prev any int16; phases 0..17"""
    rng = np.random.default_rng(seed)
    states = []
    for s in range(N_DIRECTED):
        k = K_EVEN if s % 2 == 0 else K_ODD
        st = {}
        for t in bridge.tensors:
            if t.dtype == "i8":
                if s < 24:
                    c = rng.integers(-128, 128, size=(t.R, t.C))
                else:
                    kind = (s - 24) % 4
                    c = np.full((t.R, t.C), (-128, 127, t.zero, 0)[kind])
                    if kind == 3:
                        c[:] = np.where(np.arange(t.R) % 2 == 0, -128, 127)[:, None]
                st[t.name] = state_bridge.dequantize(c, t.scale, t.zero).ravel()
            elif t.dtype == "i16":
                st[t.name] = rng.integers(-32768, 32768, size=t.R * t.C).astype(np.float64)
            else:
                a = np.float32(k * A_T[t.name])
                st[t.name] = (rng.uniform(-1.0, 1.0, size=t.R * t.C) * a).astype(np.float32)
        states.append(st)
    return states, rng.integers(0, 18, size=N_DIRECTED), rng.integers(0, 18, size=N_DIRECTED)


def directed_oracle_run(bridge, oracle, hops=3):
    """the oracle's side of the directed test, with the conditions it has to meet ON ITS OWN: every state element and output
    finite, each of the seven int8 taps at both rails on hop 1 somewhere in the batch, PCM at both rails.
    -> (states0, phase_enc, phase_dec, pcm_in, packets_in, per hop (packets, pcm, states), saturation counts)"""
    states0, pe, pd = directed_states(bridge)
    rng = np.random.default_rng(99)
    pcm_in = rng.integers(-32768, 32768, size=(hops, N_DIRECTED, 320), dtype=np.int16)
    packets_in = rng.integers(0, 256, size=(hops, N_DIRECTED, NBYTES), dtype=np.uint8)
    ora = OracleSide(oracle, N_DIRECTED, trace=True)
    for s, st in zip(ora.s, states0):
        s.set_state(st)
    per_hop, counts = [], None
    lo_rail = hi_rail = 0
    for t in range(hops):
        pk = ora.encode(pcm_in[t], list(range(N_DIRECTED)))
        out = ora.decode(packets_in[t])
        st = ora.states()
        for r, one in enumerate(st):
            for name, v in one.items():
                assert np.isfinite(v).all(), f"oracle, directed hop {t + 1}, stream {r}: {name} is not finite"
        if t == 0:
            counts = {}
            for i, pos in enumerate(ENC_INT8_TAPS):
                v = np.concatenate([taps[pos] for taps in ora.enc_taps])
                counts[f"enc tap {i}"] = (int((v == -128).sum()), int((v == 127).sum()), v.size)
            for i, pos in enumerate(DEC_INT8_TAPS):
                v = np.concatenate([taps[pos] for taps in ora.dec_taps])
                counts[f"dec tap {i}"] = (int((v == -128).sum()), int((v == 127).sum()), v.size)
        lo_rail += int((out == -32768).sum())
        hi_rail += int((out == 32767).sum())
        per_hop.append((pk, out, st))
    for name, (lo, hi, _) in counts.items():
        assert lo > 0 and hi > 0, f"oracle, directed hop 1: {name} holds {lo} codes at -128 and {hi} at 127"
    assert lo_rail > 0 and hi_rail > 0, f"oracle, directed run: PCM at -32768 {lo_rail} times, at 32767 {hi_rail} times"
    counts["pcm rails"] = (lo_rail, hi_rail, hops * N_DIRECTED * 320)
    return states0, pe, pd, pcm_in, packets_in, per_hop, counts
