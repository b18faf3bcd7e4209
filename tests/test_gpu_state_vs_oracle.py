"""What the stage kernels leave in HBM, held to the CPU oracle tensor by tensor: every export of a stream's blob is turned
into oracle state by tests/state_bridge.py and compared bit for bit -- fp32 tensors included -- with the state of an oracle
stream that saw the same input; blobs BUILT from oracle state are imported and continued on the device; and directed states
(every int8 code, both rails, every ring phase) are run one hop at a time on both sides.

The C ABI returns PCM as int16 only, so PCM is compared as int16; the float the last layer produced is seen through the
overlap tail d_up3, which is compared bit for bit with the rest of the state.

The table of the fp32 tensors' reach (A_T) and the directed states drawn from it are in tests/oracle_states.py.
"""
import numpy as np
import pytest

import state_bridge
from gpu_plumbing import make_ctx
from oracle_states import (A_T, BITS, MODES, N_DIRECTED, NBYTES, OracleSide, _compare_states, _device_hop, _inputs, _same_rows,
                           directed_oracle_run)

pytestmark = pytest.mark.gpu
EXPORT_AFTER = (1, 2, 8, 9, 10, 17, 18, 19, 37)


@pytest.fixture(scope="module")
def bridge(tmp_path_factory):
    return state_bridge.Bridge(state_bridge.compile_tool(tmp_path_factory.mktemp("blob_tool")))


@pytest.fixture(scope="module")
def oracles(oracle_default, oracle_exact, oracle_double, oracle_mixed):
    return {"xnnpack": oracle_default, "exact": oracle_exact, "gemmlowp_double": oracle_double, "builtin_mixed": oracle_mixed}


def _ctx(mode, max_streams=64):
    return make_ctx(max_streams, mode)


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
