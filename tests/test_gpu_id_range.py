"""The whole stream-id range include/lyra_hip.h documents -- max_streams up to 289,262 per context -- on the GPU: every test
here runs on a context of exactly that many streams (24 GB of state) and drives the ids tests/id_probes.py picks from the
regions' slot sizes: both sides of every region's first offset with bit 31 set, the last two slots under the cap (the last
one ends 5,120 B short of 2^32 in R_D1), the old tested edge 32,767 / 32,768, 0 and 1, and seeded ids in between, shuffled so
that every 8-stream tile mixes both ends of the arena.

How each kernel forms `stream id x slot size` (lyra_amd/csrc, read before the first run; there are two forms and no third:
no product is taken in `int`, and no sum can pass 2^32 at id cap - 1, because every `soff(s) + offset` has offset < slot
bytes and (cap - 1 + 1) x slot bytes <= 2^32 for the widest slot):

  uint32_t product, added to a wave-uniform 64-bit base as an UNSIGNED 32-bit per-lane byte offset (lyra_dev.h goff,
  TileCtx::at; the hardware form is global_load v, v_off, s[base:base+1]):
      enc_stages.h    enc_s0 (R_E0) and enc_s1 (R_E1): the lambdas soff / gat: E_FIRST, E_D0, E_D1, the phase word's store
      resblocks.h     TileCtx::soff: state_touch, resblock64 / resblock128 histories (hb0, hb1, hp) of enc_s0, enc_s1, dec_s1,
                      dec_s2
      resblock_q.h    the int8 histories of enc_s2 and dec_s0 (hp)
      enc_s2_stage.h  E_R2_0, E_D2, E_BOTT, the phase word's store (all four arithmetic modes: enc_s2_*_kernel)
      dec_stages.h    dec_s0 (D_HEAD, D_UP0, D_R0_0, D_UP1, phase store; dec_s0_*_kernel), dec_s1 (D_UP2, phase store),
                      dec_s2 (D_UP3)
  (size_t) product added to a pointer:
      the stage kernels' own read of the phase word into LDS (enc_stages.h:203, enc_s2_stage.h:74, dec_stages.h:78 and :468)
      and TileCtx::sbase -- so a stage kernel reads its phase through one form and writes it through the other;
      stream_state_kernels.hip (export / import), misc_kernels.hip (reset_kernel, log-mel M_PREV, noise estimator, resampler,
      comfort noise), lossy_kernels.hip, lossy_plan_tile.inc, decode_samples_kernels.hip, spans_kernels.hip
      (span_lane_init_kernel, span_handover_kernel), spans_dtx_kernels.hip, spans_lossy_kernels.hip; api.hip lays the regions
      out with (size_t)max_streams x slot bytes.

A stage kernel that formed its offsets wrongly but CONSISTENTLY (sign-extended, masked, wrapped) would still give the right
packets and PCM from the wrong place.  It cannot pass here: the state is read back through export_streams, which addresses
with (size_t) -- a stream living elsewhere exports the reset state, not the oracle's; the slot it lives in instead belongs
to another id, and either that id is a witness (never given to a codec call, exported before and after: any write shows) or,
in test_one_call_over_every_stream, it is live with other audio in the same call, so two streams share one slot and at most
one of them can still agree with its base stream and with the oracle's state.  Masking soff to 31 bits, for example, moves
id 262,144 of R_E0 onto id 0 -- a probe of the same call with another signal -- and id 144,632 of R_D1 onto id 0 as well.

Creation of a context is refused with LYRA_HIP_ENOMEM only when the card lacks the memory; only then do the tests skip."""
import re
import time

import numpy as np
import pytest

import id_probes
from oracle_states import MODES, OracleSide, _compare_states, _device_hop, _inputs, _same_rows
from receiver_models import LossyModel, _full_batch_mask, _lossy_check
from signals import _audio_spans as _audio, _speech, synth
from span_cases import _sequential
import state_bridge

pytestmark = pytest.mark.gpu
ENOMEM = -5                  # LYRA_HIP_ENOMEM


@pytest.fixture(scope="module")
def bridge(tmp_path_factory):
    return state_bridge.Bridge(state_bridge.compile_tool(tmp_path_factory.mktemp("blob_tool")))


@pytest.fixture(scope="module")
def oracles(oracle_default, oracle_exact, oracle_double, oracle_mixed):
    return {"xnnpack": oracle_default, "exact": oracle_exact, "gemmlowp_double": oracle_double, "builtin_mixed": oracle_mixed}


@pytest.fixture(scope="module")
def layout(bridge):
    """(cap, the probe plan) of the product's own slot sizes"""
    n = len(bridge.L["region_bytes"])
    cap = id_probes.cap_of(bridge.region(r)[1] for r in range(n))
    return cap, id_probes.probe_plan([bridge.region(r)[1] for r in range(id_probes.N_STAGE_REGIONS)], cap)


class _CapContexts:
    """At most ONE cap-sized context alive: get(mode) hands out the current one when its mode fits (every stream reset),
    else -- or when a fresh one is asked for -- closes it first and creates the next.  Creation takes 0.01 .. 2 s."""

    def __init__(self):
        self.ctx = self.mode = None

    def close(self):
        if self.ctx is not None:
            self.ctx.close()
        self.ctx = self.mode = None

    def get(self, mode, cap, fresh=False):
        import torch
        import lyra_amd
        if self.mode == mode and not fresh:
            self.ctx.synchronize()
            self.ctx.reset()
            return self.ctx
        self.close()
        free, total = torch.cuda.mem_get_info()
        t0 = time.perf_counter()
        try:
            ctx = lyra_amd.LyraHip(device=0, max_streams=cap, requant=mode)
        except lyra_amd.LyraHipError as e:
            m = re.search(r"lyra_hip_create failed \((-?\d+)\)", str(e))
            if m and int(m.group(1)) == ENOMEM:
                want = cap * lyra_amd.codec._load().lyra_hip_state_bytes_per_stream()
                pytest.skip(f"LYRA_HIP_ENOMEM: {want} bytes of state asked for, torch.cuda.mem_get_info() = {(free, total)}: {e}")
            raise
        print(f"context of {cap} streams, mode {mode}: created in {time.perf_counter() - t0:.2f} s; "
              f"torch.cuda.mem_get_info() before = {(free, total)}, after = {torch.cuda.mem_get_info()}")
        self.ctx, self.mode = ctx, mode
        return ctx


@pytest.fixture(scope="module")
def contexts():
    c = _CapContexts()
    try:
        yield c
    finally:
        c.close()


def _row_inputs(golden_dir, hops, n):
    """[hops][n][320] int16, no two rows alike: the eight input kinds of _inputs cycled over the rows; from the second cycle on
    a noise row draws from a seed of its own and every other kind gets seeded noise of +-16 LSB per cycle added (clipped: a
    rail stays mostly a rail, silence becomes a whisper)"""
    base = _inputs(golden_dir, hops)
    out = np.empty((hops, n, 320), np.int16)
    for r in range(n):
        kind, cycle = r % 8, r // 8
        x = base[:, kind].astype(np.int32)
        if cycle:
            rng = np.random.default_rng(9000 + r)
            if kind == 0:
                x = rng.integers(-32768, 32768, size=x.shape)
            else:
                x = x + rng.integers(-16 * cycle, 16 * cycle + 1, size=x.shape)
        out[:, r] = np.clip(x, -32768, 32767).astype(np.int16)
    assert len({out[:, r].tobytes() for r in range(n)}) == n
    return out


def _payload(bridge, blobs):
    """the blobs without their headers (a header names the source id and its comfort-noise key; blobs of equal stream state
    are byte-identical from there on, whichever id they came from: stream_blob.h)"""
    return np.asarray(blobs)[..., bridge.L["header_bytes"]:]


def _witnesses_untouched(where, ctx, ids, before):
    after = ctx.export_streams(ids)
    bad = [int(ids[k]) for k in range(len(ids)) if not np.array_equal(after[k], before[k])]
    assert not bad, f"{where}: streams {bad}, which no call was given, no longer hold what they held after creation"


# ---- (b) ------------------------------------------------------------------------------------------------------------------
def test_imported_state_at_the_top_of_the_arena(golden_dir, bridge, oracles, layout, contexts):
    """Blobs BUILT from oracle state after 9 hops, imported at cap - 1, cap - 2 and both sides of R_D1's crossing, continued
    for 10 hops on both sides; then two of them reset: their next hop is a fresh oracle stream's and the others keep theirs."""
    cap, plan = layout
    mode, k, more = "xnnpack", 9, 10
    kd1 = plan["cross"][state_bridge.R_D1]
    ids = [cap - 1, kd1 - 1, cap - 2, kd1]
    n = len(ids)
    wit = id_probes.witnesses_of(ids, cap)
    pcm = _inputs(golden_dir, k + more + 1)[:, [0, 1, 5, 7]]           # white noise, speech, square wave, impulses
    ora = OracleSide(oracles[mode], n)
    for t in range(k):
        ora.decode(ora.encode(pcm[t], list(range(n))))
    ctx = contexts.get(mode, cap)
    wit0 = ctx.export_streams(wit)
    fresh = ctx.export_streams(ids)
    blobs = np.stack([bridge.to_blob(st, k, k, mode, fresh[r]) for r, st in enumerate(ora.states())])
    ctx.import_streams(ids, blobs)
    _compare_states(bridge, ctx.export_streams(ids), ora.states(), [k] * n, [k] * n, "right after the import")
    for t in range(k, k + more):
        pk, _, out = _device_hop(ctx, ids, list(range(n)), pcm[t], [])
        want_pk = ora.encode(pcm[t], list(range(n)))
        _same_rows(f"hop {t + 1}", "the packet", pk, want_pk)
        _same_rows(f"hop {t + 1}", "the PCM", out, ora.decode(want_pk))
    kept = ctx.export_streams(ids)
    _compare_states(bridge, kept, ora.states(), [k + more] * n, [k + more] * n, f"{more} hops after the import")
    # reset two of them: the stream at the very top and the first one of R_D1 with bit 31 set
    again, others = [0, 3], [1, 2]
    ctx.reset([ids[r] for r in again])
    got = ctx.export_streams(ids)
    assert np.array_equal(got[others], kept[others]), "reset_streams of two ids touched the others"
    assert np.array_equal(_payload(bridge, got[again]), _payload(bridge, fresh[again])), "reset_streams left state behind"
    t = k + more
    new = OracleSide(oracles[mode], len(again))
    pk, _, out = _device_hop(ctx, [ids[r] for r in again], [0, 1], pcm[t][again], [])
    want_pk = new.encode(pcm[t][again], [0, 1])
    _same_rows("first hop after the reset", "the packet", pk, want_pk)
    _same_rows("first hop after the reset", "the PCM", out, new.decode(want_pk))
    got = ctx.export_streams(ids)
    _compare_states(bridge, got[again], new.states(), [1, 1], [1, 1], "first hop after the reset")
    assert np.array_equal(got[others], kept[others]), "a hop on the reset streams touched the others"
    _witnesses_untouched("imported state", ctx, wit, wit0)


# ---- (c) ------------------------------------------------------------------------------------------------------------------
def test_one_call_over_every_stream(bridge, oracle_default, layout, contexts):
    """ids = a seeded permutation of every id of the context in ONE call per hop, 120 bits, 3 hops, 64 base streams replicated
    (as test_config5_32768_streams_one_gpu): rows 0..63 against the oracle, every replica against its base row on the device,
    and afterwards the probe ids' exported state against the oracle state of the base stream each replays -- every slot of
    the arena is live, so an offset that collapses onto another slot has two streams writing one place."""
    import torch
    import lyra_amd
    from oracle import lyra_oracle
    cap, plan = layout
    R, T, bits = 64, 3, 120
    nq = bits // 4
    base = synth(R, T, seed=289262)
    base[7:9] //= 50
    streams = [lyra_oracle.Stream(oracle_default) for _ in range(R)]
    want_pk = np.zeros((T, R, bits // 8), np.uint8)
    want_out = np.zeros((T, R, 320), np.int16)
    for t in range(T):
        for r, s in enumerate(streams):
            want_pk[t, r] = oracle_default.pack(oracle_default.rvq_encode(s.encode(base[t, r]), nq), nq)[0]
            want_out[t, r] = s.decode(oracle_default.rvq_decode(oracle_default.unpack(want_pk[t, r], nq))[0])
    dev = torch.device("cuda", 0)
    ctx = contexts.get("xnnpack", cap)
    t0 = time.perf_counter()
    perm = np.random.default_rng(5).permutation(cap).astype(np.int32)
    row_of = np.empty(cap, np.int64)
    row_of[perm] = np.arange(cap)
    ids = torch.from_numpy(perm).to(dev)
    rep = torch.arange(cap, device=dev) % R
    d_base = torch.from_numpy(base).to(dev)
    pk = torch.empty((cap, lyra_amd.packet_size(bits)), device=dev, dtype=torch.uint8)
    out = torch.empty((cap, 320), device=dev, dtype=torch.int16)
    for t in range(T):
        pcm = d_base[t][rep].contiguous()
        ctx.encode_dev(ids, pcm, bits, pk)
        ctx.decode_dev(ids, pk, bits, out)
        ctx.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(pk[:R].cpu().numpy(), want_pk[t]), f"packets differ from the oracle at hop {t}"
        assert np.array_equal(out[:R].cpu().numpy(), want_out[t]), f"PCM differs from the oracle at hop {t}"
        if not torch.equal(pk, pk[:R][rep]):
            bad = (pk != pk[:R][rep]).any(dim=1).nonzero().flatten()[:8].cpu().numpy()
            raise AssertionError(f"hop {t}: packets of rows {bad.tolist()} (ids {perm[bad].tolist()}) differ from their base rows")
        if not torch.equal(out, out[:R][rep]):
            bad = (out != out[:R][rep]).any(dim=1).nonzero().flatten()[:8].cpu().numpy()
            raise AssertionError(f"hop {t}: PCM of rows {bad.tolist()} (ids {perm[bad].tolist()}) differs from its base row")
    probes = plan["order"]
    states = [s.state() for s in streams]
    _compare_states(bridge, ctx.export_streams(probes), [states[int(row_of[p]) % R] for p in probes], [T] * len(probes),
                    [T] * len(probes), f"{cap} streams in one call, after hop {T}")
    print(f"one call over {cap} streams: {T} hops, checks and the probes' export in {time.perf_counter() - t0:.2f} s")
    del pk, out, d_base, ids, rep
    torch.cuda.empty_cache()


# ---- (d) ------------------------------------------------------------------------------------------------------------------
def test_side_kernels_at_the_probe_ids(golden_dir, bridge, oracle_default, layout, contexts):
    """decode_lossy_dev at 48 kHz and 120 bits over the probe ids against the reference model (comfort noise keyed by id): the
    noise estimator, the comfort-noise generator, the resampler and the loss control word at offsets up to 2.4 GB; then
    encode at 48 kHz with DTX on the probes against the same calls on a 64-stream context at ids 0 .. n-1."""
    import torch
    import lyra_amd
    from oracle import lyra_codec_model as M
    cap, plan = layout
    ids = np.array(plan["order"], np.int32)
    B, T, rate, bits = len(ids), 44, 48000, 120
    assert B <= 64
    mask = _full_batch_mask(T, B, np.random.default_rng(rate + B))
    for t in range(T):
        pairs = {(int(mask[t, 2 * k]), int(mask[t, 2 * k + 1])) for k in range(B // 2)}
        assert pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}, t
    assert any((mask[t, 4 * j:4 * j + 4] == 0).all() for t in range(T) for j in range(B // 4))
    pcm = _speech(golden_dir, B, T, offset=4321)
    encs = [M.RefLyraEncoder(oracle_default, 16000, bits, False) for _ in range(B)]
    packets = np.stack([np.stack([encs[s].Encode(pcm[t, s]) for s in range(B)]) for t in range(T)])
    model = LossyModel(oracle_default, rate, ids)
    ctx = contexts.get("xnnpack", cap)
    wit = plan["witnesses"]
    wit0 = ctx.export_streams(wit)
    _lossy_check(ctx, model, ids, packets, mask, bits)
    assert ctx.decode_lossy_errors() == 0
    model.tally.report(f"probe ids B={B} {rate} Hz")
    assert model.tally.exact_fraction() > 0.97
    assert model.saw_back >= 2 and model.saw_mix and model.saw_cn
    # the encoder side has no id-keyed randomness: the same calls on a small context must give the same bytes and state
    dev = torch.device("cuda", 0)
    hops = 4
    x48 = np.repeat(_speech(golden_dir, B, hops, offset=777), 3, axis=2)         # any 48 kHz input will do
    x48[:, 1::3] //= 256                                                        # every third stream close to silence
    small = lyra_amd.LyraHip(device=0, max_streams=64)
    try:
        res = []
        for c, these in ((ctx, ids), (small, np.arange(B, dtype=np.int32))):
            d_ids = torch.from_numpy(these).to(dev)
            c.set_encoder_sample_rate(rate)          # what a DTX LyraEncoder created at `rate` gives its estimator
            got = []
            for t in range(hops):
                pk = torch.zeros((B, lyra_amd.packet_size(bits)), dtype=torch.uint8, device=dev)
                nb = torch.zeros(B, dtype=torch.int32, device=dev)
                c.encode_ext_dev(d_ids, torch.from_numpy(x48[t]).to(dev), rate, bits, pk, nb, dtx=True)
                c.synchronize()
                got.append((pk.cpu().numpy(), nb.cpu().numpy()))
            res.append((got, _payload(bridge, c.export_streams(these))))
        for t in range(hops):
            assert np.array_equal(res[0][0][t][1], res[1][0][t][1]), f"DTX encode at 48 kHz, hop {t}: packet sizes"
            assert np.array_equal(res[0][0][t][0], res[1][0][t][0]), f"DTX encode at 48 kHz, hop {t}: packets"
        enc = np.zeros(res[0][1].shape[1], bool)
        for r, side in enumerate(bridge.L["region_side"]):
            if side & lyra_amd.codec.STATE_ENCODER:
                o, nbytes = bridge.region(r)
                enc[o - bridge.L["header_bytes"]:o - bridge.L["header_bytes"] + nbytes] = True
        assert np.array_equal(res[0][1][:, enc], res[1][1][:, enc]), "DTX encode at 48 kHz: the encoder side's state"
    finally:
        small.close()
        ctx.set_encoder_sample_rate(16000)           # the context is shared: back to what creation set
    _witnesses_untouched("side kernels", ctx, wit, wit0)


# ---- (e) ------------------------------------------------------------------------------------------------------------------
def test_span_with_lent_lanes_at_the_top(golden_dir, bridge, layout, contexts):
    """A 350-frame span on the first stream of R_D1 with bit 31 set, its 40 lanes lent from cap - 41 .. cap - 2
    (span_lane_init_kernel, span_handover_kernel at high ids): packets, PCM and the span stream's state equal the hop-by-hop
    calls on a twin stream of the same context, and the lanes hold afterwards what they held before."""
    cap, plan = layout
    sid, twin, n, bits = plan["cross"][state_bridge.R_D1], plan["cross"][state_bridge.R_E1], 350, 184
    lanes = np.arange(cap - 41, cap - 1, dtype=np.int32)
    assert len(lanes) == 40 and sid not in lanes and twin not in lanes
    x = _audio(golden_dir, n, 350)
    ctx = contexts.get("xnnpack", cap)
    lanes0 = ctx.export_streams(lanes)
    want_pk = _sequential(ctx, {twin: x}, bits, True)[twin]
    want_pcm = _sequential(ctx, {twin: want_pk}, bits, False)[twin]
    pk = ctx.encode_spans([(sid, 0, n)], x, bits, lanes)
    diff = np.flatnonzero((pk != want_pk).any(axis=1))
    assert len(diff) == 0, f"packets of the span differ at hops {list(diff[:8])} of {n}"
    assert np.array_equal(ctx.export_streams(lanes), lanes0), "lanes after encode_spans"
    out = ctx.decode_spans([(sid, 0, n)], pk, bits, lanes)
    diff = np.flatnonzero((out != want_pcm).any(axis=1))
    assert len(diff) == 0, f"PCM of the span differs at hops {list(diff[:8])} of {n}"
    got = ctx.export_streams([sid, twin])
    assert np.array_equal(_payload(bridge, got[0]), _payload(bridge, got[1])), "the span stream's state is not its twin's"
    bad = [int(lanes[k]) for k, (a, b) in enumerate(zip(ctx.export_streams(lanes), lanes0)) if not np.array_equal(a, b)]
    assert not bad, f"lanes {bad} do not hold what they held before"


# ---- (a) ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_stage_kernels_at_the_probe_ids(golden_dir, bridge, oracles, layout, contexts, mode):
    """The probe ids in one batch, every row with audio of its own, 20 hops at 184 bits (the ring phase passes 18 -> 0):
    packets and PCM equal the oracle's at every hop; after hops 1, 18 and 20 every probe's exported state equals the oracle's
    tensor by tensor, fp32 included, padding zero, phase words right; and the witnesses next to the probes are, after the last
    hop, byte for byte what they were after creation."""
    cap, plan = layout
    ids, wit = plan["order"], plan["witnesses"]
    n, hops = len(ids), 20
    rows = list(range(n))
    pcm = _row_inputs(golden_dir, hops, n)
    ora = OracleSide(oracles[mode], n)
    ctx = contexts.get(mode, cap, fresh=True)         # a context no call has touched: the witnesses' blobs are creation's
    t0 = time.perf_counter()
    wit0 = ctx.export_streams(wit)
    for t in range(hops):
        pk, _, out = _device_hop(ctx, ids, rows, pcm[t], [])
        want_pk = ora.encode(pcm[t], rows)
        _same_rows(f"{mode} hop {t + 1}", "the packet", pk, want_pk)
        _same_rows(f"{mode} hop {t + 1}", "the PCM", out, ora.decode(want_pk))
        if t + 1 in (1, 18, 20):
            _compare_states(bridge, ctx.export_streams(ids), ora.states(), [t + 1] * n, [t + 1] * n,
                            f"{mode}, probe ids {ids}, export after hop {t + 1}")
    _witnesses_untouched(f"{mode}, stage kernels", ctx, wit, wit0)
    print(f"{mode}: {n} probes x {hops} hops with the oracle beside them in {time.perf_counter() - t0:.2f} s")
