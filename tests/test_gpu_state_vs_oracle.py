"""What the stage kernels leave in HBM, held to the CPU oracle tensor by tensor: every export of a stream's blob is turned
into oracle state by tests/state_bridge.py and compared bit for bit -- fp32 tensors included -- with the state of an oracle
stream that saw the same input; blobs BUILT from oracle state are imported and continued on the device; and directed states
(every int8 code, both rails, every ring phase) are run one hop at a time on both sides.

The C ABI returns PCM as int16 only, so PCM is compared as int16; the float the last layer produced is seen through the
overlap tail d_up3, which is compared bit for bit with the rest of the state.

A_T below: the largest magnitude each fp32 tensor reaches in the oracle (mode xnnpack) during the 37 hops of the
full-scale white-noise stream of test_state_after_n_hops_equals_the_oracle (stream 0 of _inputs), measured on the reference
only and rounded up to three digits; the first test asserts that the oracle still stays inside them.  The directed test
draws fp32 state uniform in +-k A_t with k = 1 (even streams) and k = 8 (odd streams).

    tensor    max |x|      tensor    max |x|      tensor    max |x|      tensor    max |x|
    e_first   1            e_r1[0]   364          d_head    41.3         d_r1[0]   22.1
    e_r0[0]   9.3          e_r1[1]   368          d_up0[0]  15.2         d_r1[1]   45.9
    e_r0[1]   86.1         e_r1[2]   757          d_up0[1]  6.33         d_r1[2]   43.6
    e_r0[2]   119          e_d1      747          d_up0[2]  13.7         d_up2     2.74
    e_d0      95.1         e_r2[0]   2000         d_up0[3]  20.4         d_r2[0]   5.93
                                                  d_up1[0]  5.37         d_r2[1]   6.81
                                                  d_up1[1]  22.2         d_r2[2]   26.5
                                                                         d_up3     0.737
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import state_bridge                                                                    # noqa: E402

pytestmark = pytest.mark.gpu
BITS, NBYTES = 184, 23
MODES = ["xnnpack", "exact", "gemmlowp_double", "builtin_mixed"]
EXPORT_AFTER = (1, 2, 8, 9, 10, 17, 18, 19, 37)
TRACE_CAP = 16384
ENC_INT8_TAPS, DEC_INT8_TAPS = (10, 11, 12, 13), (2, 3, 4)      # positions of the int8 taps among a frame's trace taps

A_T = {"e_first": 1, "e_r0[0]": 9.3, "e_r0[1]": 86.1, "e_r0[2]": 119, "e_d0": 95.1, "e_r1[0]": 364, "e_r1[1]": 368,
       "e_r1[2]": 757, "e_d1": 747, "e_r2[0]": 2000, "d_head": 41.3, "d_up0[0]": 15.2, "d_up0[1]": 6.33, "d_up0[2]": 13.7,
       "d_up0[3]": 20.4, "d_up1[0]": 5.37, "d_up1[1]": 22.2, "d_r1[0]": 22.1, "d_r1[1]": 45.9, "d_r1[2]": 43.6, "d_up2":
       2.74, "d_r2[0]": 5.93, "d_r2[1]": 6.81, "d_r2[2]": 26.5, "d_up3": 0.737}
K_EVEN, K_ODD = 1, 8


@pytest.fixture(scope="module")
def bridge(tmp_path_factory):
    return state_bridge.Bridge(state_bridge.compile_tool(tmp_path_factory.mktemp("blob_tool")))


@pytest.fixture(scope="module")
def oracles(oracle_default, oracle_exact, oracle_double, oracle_mixed):
    return {"xnnpack": oracle_default, "exact": oracle_exact, "gemmlowp_double": oracle_double, "builtin_mixed": oracle_mixed}


def _ctx(mode, max_streams=64):
    import lyra_amd
    return lyra_amd.LyraHip(device=0, max_streams=max_streams, requant=mode)


def _inputs(golden_dir, hops):
    """[hops][8][320] int16, one input kind per stream: full-scale white noise, speech, speech / 64, DC +32767, DC -32768,
    a +-full-scale square wave of period 160 samples, digital silence, impulses"""
    rng = np.random.default_rng(1848)
    n = hops * 320
    sp = np.load(os.path.join(golden_dir, "sample_wavs.npz"))["sample1_16kHz"].astype(np.int16)[4000:4000 + n]
    assert sp.size == n
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


@pytest.mark.parametrize("mode", MODES)
def test_state_after_n_hops_equals_the_oracle(golden_dir, bridge, oracles, mode):
    hops = max(EXPORT_AFTER)
    ids = [5, 17, 2, 40, 9, 33, 21, 63, 1, 60, 12, 44, 8, 61, 30, 0]      # rows 0-7 encode and decode, rows 8-15 only decode
    pcm = _inputs(golden_dir, hops)
    rand = np.random.default_rng(77).integers(0, 256, size=(hops, 8, NBYTES), dtype=np.uint8)   # any bytes are a packet
    ora = OracleSide(oracles[mode], 16)
    peak = {name: 0.0 for name in A_T}
    ctx = _ctx(mode)
    try:
        for t in range(hops):
            pk, allpk, out = _device_hop(ctx, ids, list(range(8)), pcm[t], rand[t])
            want_pk = ora.encode(pcm[t], list(range(8)))
            _same_rows(f"{mode} hop {t + 1}", "the packet", pk, want_pk)
            _same_rows(f"{mode} hop {t + 1}", "the PCM", out, ora.decode(np.concatenate([want_pk, rand[t]])))
            st = ora.states()
            for name in A_T:
                peak[name] = max(peak[name], float(np.abs(st[0][name]).max()))
            if t + 1 in EXPORT_AFTER:
                _compare_states(bridge, ctx.export_streams(ids), st, [t + 1] * 8 + [0] * 8, [t + 1] * 16,
                                f"{mode}, export after hop {t + 1}")
    finally:
        ctx.close()
    print(f"{mode}: max |x| of the white-noise stream on the oracle:", {k: float(f"{v:.4g}") for k, v in peak.items()})
    if mode == "xnnpack":             # the A_t table is the reference's own reach in this mode, rounded up to three digits
        for name, v in peak.items():
            assert 0.99 * A_T[name] <= v <= A_T[name], (name, v)


@pytest.mark.parametrize("mode", ["xnnpack", "builtin_mixed"])
@pytest.mark.parametrize("side", ["encoder", "decoder"])
def test_oracle_made_blob_continues_on_the_device(golden_dir, bridge, oracles, mode, side):
    from lyra_amd import codec
    sides = codec.STATE_ENCODER if side == "encoder" else codec.STATE_DECODER
    k, more, n = 13, 25, 4
    src_rows = [0, 1, 5, 7]                            # white noise, speech, square wave, impulses
    ids = [41, 3, 28, 16]
    pcm = _inputs(golden_dir, k + more)[:, src_rows]
    ora = OracleSide(oracles[mode], n)
    for t in range(k):                                 # the oracle alone: mid-ring at phase 13
        ora.decode(ora.encode(pcm[t], list(range(n))))
    ctx = _ctx(mode)
    try:
        fresh = ctx.export_streams(ids)                # reset exports of the targets: header, and the regions out of scope
        blobs = np.stack([bridge.to_blob(st, k, k, mode, fresh[r]) for r, st in enumerate(ora.states())])
        ctx.import_streams(ids, blobs, sides=sides)
        # the twin on the oracle: the imported side continues, the other side is a fresh stream's
        region_side = bridge.L["region_side"]
        twin = OracleSide(oracles[mode], n)
        for r in range(n):
            twin.s[r].set_state({t.name: v for t, v in ((bridge.by_name[nm], v) for nm, v in ora.s[r].state().items())
                                 if region_side[t.region] & sides})
        got = ctx.export_streams(ids)
        for r in range(n):
            for reg in range(len(region_side)):
                o, nb = bridge.region(reg)
                want = blobs[r] if region_side[reg] & sides else fresh[r]
                assert np.array_equal(got[r, o:o + nb], want[o:o + nb]), \
                    f"{mode} {side}: region {reg} of row {r} after the import is not the {'imported' if region_side[reg] & sides else 'reset'} one"
        fe = k if side == "encoder" else 0
        fd = k if side == "decoder" else 0
        _compare_states(bridge, got, twin.states(), [fe] * n, [fd] * n, f"{mode} {side}, right after the import")
        for t in range(k, k + more):
            pk, allpk, out = _device_hop(ctx, ids, list(range(n)), pcm[t], [])
            want_pk = twin.encode(pcm[t], list(range(n)))
            _same_rows(f"{mode} {side} hop {t + 1}", "the packet", pk, want_pk)
            _same_rows(f"{mode} {side} hop {t + 1}", "the PCM", out, twin.decode(want_pk))
        _compare_states(bridge, ctx.export_streams(ids), twin.states(), [fe + more] * n, [fd + more] * n,
                        f"{mode} {side}, {more} hops after the import")
    finally:
        ctx.close()


# ---- directed states ------------------------------------------------------------------------------------------------------
N_DIRECTED = 32


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


@pytest.mark.parametrize("mode", MODES)
def test_directed_states_one_hop_at_a_time(bridge, oracles, mode):
    states0, pe, pd, pcm_in, packets_in, per_hop, counts = directed_oracle_run(bridge, oracles[mode])
    print(f"{mode}: (codes at -128, at 127, of) per int8 tap on hop 1 of the directed run, oracle:", counts)
    ids = [int(v) for v in np.random.default_rng(5).permutation(64)[:N_DIRECTED]]
    ctx = _ctx(mode)
    try:
        fresh = ctx.export_streams(ids)
        blobs = np.stack([bridge.to_blob(st, int(pe[r]), int(pd[r]), mode, fresh[r]) for r, st in enumerate(states0)])
        ctx.import_streams(ids, blobs)
        _compare_states(bridge, ctx.export_streams(ids), states0, pe, pd, f"{mode}, right after the import")
        for t, (want_pk, want_out, want_st) in enumerate(per_hop):
            ctx.logmel(pcm_in[t], ids)
            pk = ctx.encode(pcm_in[t], BITS, ids)
            out = ctx.decode(packets_in[t], BITS, ids)
            _same_rows(f"{mode} directed hop {t + 1}", "the packet", pk, want_pk)
            _same_rows(f"{mode} directed hop {t + 1}", "the PCM", out, want_out)
            _compare_states(bridge, ctx.export_streams(ids), want_st, pe + t + 1, pd + t + 1, f"{mode}, directed hop {t + 1}")
    finally:
        ctx.close()
