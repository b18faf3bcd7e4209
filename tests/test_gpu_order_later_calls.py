"""The later entry points on the streams production runs on, driven by a caller that does not synchronise.

Stream kind: every context here is made with streams="plain" (tests/gpu_plumbing.py make_ctx): hipStreamNonBlocking priority
streams, the kind a 4,096-stream context gets, at 64 to 256 streams.  The first test holds that premise to hipStreamGetFlags.
On the CU-masked streams that small contexts get by default, every upload and read-back through torch's NULL stream is a
barrier across the four library streams, and a missing event, scratch reused a tick early, an output that completes on a
stream lyra_hip_stream_wait does not cover, or a binding without the _dev_call bracket cannot show.

1. The premise: the four stream handles report hipStreamNonBlocking on a plain context and agree on a default one.
2. The control: the instrument sees the defect it is built for.  With torch_order off, a payload uploaded behind the late
   caller's work is not seen by the call (its result is the one of the buffer's EARLIER payload), and a read on a stream the
   library's work was not ordered before returns the output buffer's earlier content; with torch_order on, the same scripts
   give the fresh result.  The late work is sized from a timing of the same call, synchronised, on the twin (gpu_plumbing
   late_delay_ms: 20 times, 2 ms at least, 50 ms at most; measured on an MI355X at B = 37: encode_streams_dev 0.17 ms, so
   3.4 ms of late work, decode_streams_dev 0.25 ms, so 5.0 ms).  That it suffices is asserted, not assumed: the late work
   must still be pending when the library's call (input side) or the read (output side) has finished, on a caller stream
   chosen so that a shared hardware queue does not order the two by itself (LateStream.clear_of).
3. The ordering game (after tests/test_gpu_api_fuzz.py): about 40 operations per seed over random subsets of the ids in random
   order -- encode_streams_dev, decode_streams_dev, decode_lossy_mixed_dev, decode_lossy_rates_dev, decode_samples_streams_dev,
   the three bridge ticks, export + import under other ids, resets, one encode_spans_dev and one decode_spans_lossy_dev -- on
   `x`, from the late stream with torch_order on, two buffer sets in rotation, results read with .cpu() on the caller's
   stream.  `ref` runs the whole script first, one operation at a time with a synchronise after each; then `x` runs it with
   no synchronise of the context or of the device until the closing state check (lyra_hip_reset_streams drains the context by
   its own contract).  Everything written must agree bit for bit, and the exported state of every id at the end.

Checked by hand on an MI355X: with LateStream.hold enqueuing nothing, both control cases fail (at their first assertion, that
the late work is still pending when the call has finished)."""
import time

import numpy as np
import pytest

from bridge_models import np_bridge_plan
from gpu_plumbing import (HIP_STREAM_NON_BLOCKING, _dev, _ids, _pinned, _t, late_delay_ms, late_stream, make_ctx,
                          stream_flags)
from row_cases import ROW, _draw_bits, _same_state
from signals import RATES

pytestmark = pytest.mark.gpu
SIZES = np.array([0, 8, 15, 23], np.int32)


# ---- 1. the premise -------------------------------------------------------------------------------------------------------

def test_plain_contexts_run_on_non_blocking_streams():
    plain, default = make_ctx(64, streams="plain"), make_ctx(64)
    try:
        got = stream_flags(plain)
        if got is None:
            pytest.skip("hipStreamGetFlags cannot be resolved from the HIP runtime this process has loaded")
        masked = stream_flags(default)
        print("hipStreamGetFlags, encode / decode / quantizer / noise: plain", got, "default 64-stream context", masked)
        assert got == [HIP_STREAM_NON_BLOCKING] * 4, got
        # masked streams report the default flags; a runtime that refused CU masks gives the non-blocking fallback
        assert len(set(masked)) == 1 and masked[0] in (0, HIP_STREAM_NON_BLOCKING), masked
    finally:
        plain.close()
        default.close()


# ---- 2. the control -------------------------------------------------------------------------------------------------------

class _Side:
    """One side of the codec for the control: fixed ids / rates / sizes, a payload buffer and the call on it"""

    def __init__(self, side, B, ms, rng):
        import torch
        self.side, self.B = side, B
        self.ids = _ids(B, ms, 77)
        self.rates = np.array([RATES[(b // 3) % 4] for b in range(B)], np.int32)
        self.d_ids, self.d_rates = _t(self.ids), _t(self.rates)
        if side == "encode":
            self.d_aux = _t(np.array([(64, 120, 184)[b % 3] for b in range(B)], np.int32))     # bit counts
            self.payloads = [rng.integers(-12000, 12000, (B, ROW)).astype(np.int16) for _ in range(4)]
        else:
            self.d_aux = _t(SIZES[1 + np.arange(B) % 3])                                       # packet sizes, none empty
            self.payloads = [rng.integers(0, 256, (B, 23), dtype=np.uint8) for _ in range(4)]
        self.d_payload = {}          # per context
        self.out = {}
        self.torch = torch

    def bufs(self, c):
        torch, B = self.torch, self.B
        if c not in self.out:
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=_dev())   # noqa: E731
            self.d_payload[c] = _t(self.payloads[0])
            self.out[c] = ((z((B, 23), torch.uint8), z((B,), torch.int32)) if self.side == "encode" else
                           (z((B * ROW,), torch.int16), z((B, 320), torch.int16), z((B,), torch.int32), z((B,), torch.int32)))
        return self.d_payload[c], self.out[c]

    def call(self, c):
        p, o = self.bufs(c)
        if self.side == "encode":
            c.encode_streams_dev(self.d_ids, p, self.d_rates, self.d_aux, o[0], o[1])
        else:
            c.decode_streams_dev(self.d_ids, p, self.d_aux, self.d_rates, o[0], None, o[1], o[2], o[3])

    def read(self, c):
        return tuple(t.cpu().numpy().copy() for t in self.bufs(c)[1])

    def read_on(self, c, stream):
        """the outputs through pinned memory on `stream`, waiting for that stream alone"""
        torch, outs = self.torch, self.bufs(c)[1]
        hosts = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in outs]
        with torch.cuda.stream(stream):
            for h, t in zip(hosts, outs):
                h.copy_(t, non_blocking=True)
        stream.synchronize()
        return tuple(h.numpy().copy() for h in hosts)

    def run_synchronised(self, c, payload):
        """the call on `payload`, everything synchronised -> (outputs, seconds of call + synchronise)"""
        torch = self.torch
        self.bufs(c)[0].copy_(torch.from_numpy(payload))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.call(c)
        c.synchronize()
        dt = time.perf_counter() - t0
        torch.cuda.synchronize()
        return self.read(c), dt


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("side", ["encode", "decode"])
def test_control_a_late_upload_and_an_unordered_read_are_seen(side):
    import torch
    ms, B = 64, 37
    rng = np.random.default_rng(9100 + (side == "decode"))
    x, ref = make_ctx(ms, cng_seed=7, streams="plain"), make_ctx(ms, cng_seed=7, streams="plain")
    try:
        s = _Side(side, B, ms, rng)
        warm, old, new, other = s.payloads
        for c in (x, ref):                      # two hops: kernels loaded, the state past its reset values
            s.run_synchronised(c, warm)
        _, seconds = s.run_synchronised(ref, warm)
        s.run_synchronised(x, warm)
        delay = late_delay_ms(seconds)
        late = late_stream(delay)
        print(f"{side}: the synchronised call took {seconds * 1e3:.3f} ms, the late caller holds uploads back {delay:.1f} ms "
              f"({late.reps} matmuls of {late.ms_per_matmul:.3f} ms)")
        state = ref.export_streams(s.ids)
        _same_state(x, ref, s.ids, "before the control")

        def probe():
            s.call(x)
            x.synchronize()

        x.torch_order = False
        assert late.clear_of(probe), ("on every torch stream tried the late work was over when the call had finished: the work is "
                                      "too short, or each of them shares a hardware queue (GPU_MAX_HW_QUEUES) with a library "
                                      "stream of this call -- the instrument cannot see a late upload here, whatever the library does")
        x.torch_order = True
        want_stale, _ = s.run_synchronised(ref, old)
        ref.import_streams(s.ids, state)
        want_fresh, _ = s.run_synchronised(ref, new)
        assert not _equal(want_stale, want_fresh) and not np.array_equal(want_stale[0], want_fresh[0])
        p_new = _pinned(new)

        def rewind():
            """x back to `state`, its payload buffer to `old`, its outputs to the result of an unrelated payload"""
            late.stream.synchronize()
            x.import_streams(s.ids, state)
            earlier, _ = s.run_synchronised(x, other)
            x.import_streams(s.ids, state)
            s.bufs(x)[0].copy_(torch.from_numpy(old))
            torch.cuda.synchronize()
            assert not _equal(earlier, want_fresh)
            return earlier

        # (a) the input side, unordered: the payload arrives behind the late work, the call has read the earlier one
        rewind()
        x.torch_order = False
        late.upload(s.bufs(x)[0], p_new)
        s.call(x)
        x.synchronize()
        assert not late.stream.query(), "the late work ended before the library's: it is too short for this control"
        got = s.read(x)
        assert _equal(got, want_stale), "the call did not run on the buffer's earlier payload"
        assert not _equal(got, want_fresh)
        # (b) the input side, ordered: torch_order brackets the call on the caller's stream
        rewind()
        x.torch_order = True
        with torch.cuda.stream(late.stream):
            late.upload(s.bufs(x)[0], p_new)
            s.call(x)
            got = s.read(x)                     # .cpu() on the caller's stream: behind lyra_hip_stream_wait
        assert _equal(got, want_fresh), "torch_order on: the call overtook the caller's upload, or the read the call"
        # (c) the output side, unordered: the library waits for the late work (lyra_hip_wait_for_stream); a read on a second
        # stream of the caller's that nothing ordered behind the library returns the buffer's earlier content.  The read is
        # tried on a few streams, until one is not held back by a hardware queue it shares (LateStream.clear_of): the late
        # work is then still pending when the read has returned, so the library cannot have started.
        for reader in [torch.cuda.Stream(device=_dev()) for _ in range(3)] + [torch.cuda.default_stream(_dev())]:
            earlier = rewind()
            s.bufs(x)[0].copy_(torch.from_numpy(new))
            torch.cuda.synchronize()
            x.torch_order = False
            late.hold()
            x._chk(x.L.lyra_hip_wait_for_stream(x.h, late.stream.cuda_stream))
            s.call(x)
            got = s.read_on(x, reader)
            pending = not late.stream.query()
            x.synchronize()
            if pending:
                break
        else:
            pytest.fail("no stream found whose read passes the waiting library: no control of the output side")
        assert _equal(got, earlier), "the unordered read did not return the buffer's earlier content"
        assert not _equal(got, want_fresh)
        assert _equal(s.read(x), want_fresh)
        # (d) the output side, ordered: the same script with the bracket, on the same stream
        rewind()
        s.bufs(x)[0].copy_(torch.from_numpy(new))
        torch.cuda.synchronize()
        x.torch_order = True
        late.hold()
        x._chk(x.L.lyra_hip_wait_for_stream(x.h, late.stream.cuda_stream))
        with torch.cuda.stream(reader):
            s.call(x)
        got = s.read_on(x, reader)
        assert _equal(got, want_fresh), "torch_order on: the read overtook the call"
        late.stream.synchronize()
        x.synchronize()
        _same_state(x, ref, s.ids, "after the control")
    finally:
        torch.cuda.synchronize()
        x.close()
        ref.close()


# ---- 3. the ordering game -------------------------------------------------------------------------------------------------

MS, POOL, MAXB, E_MAX, N_TABLE, SPAN_F, SPAN_BITS = 256, 224, 130, 144, 16, 124, 120
QUIET = np.arange(POOL, POOL + 24, dtype=np.int32)   # DTX encoders at 16 kHz that hear room noise after three hops of speech: only
                                                     # `enc` operations name them, never a reset, a tick or an import
LANES = np.arange(POOL + 24, MS, dtype=np.int32)     # 8 ids lent to the span calls; nothing else names them
WARM = 6                                             # `enc` operations over all of QUIET in front of the drawn ones: a
                                                     # NoiseEstimator that heard 3 hops of speech calls the third hop of
                                                     # room noise after them noise (oracle/lyra_oracle.NoiseEstimator, on the CPU)
B_SET = (3, 37, 65, 130)
REQUESTS = (1, 128, 441, 1024, 3840)
KINDS = {"enc": 5, "dec_streams": 4, "lossy_mixed": 3, "lossy_rates": 3, "samples": 4, "bridge": 4, "speakers": 4, "shared": 4,
         "expimp": 3, "reset": 3, "spans_enc": 1, "spans_lossy": 1}


def _draw_rooms(rng, B):
    """labels [B]: at B = 130 one room of 65, past a wavefront; rooms of 1 to 9 members; a few rows in no room; at most
    N_TABLE - 1 rooms"""
    rooms = np.full(B, -1, np.int32)
    rows = rng.permutation(B)
    at = label = 0
    if B >= 130:
        rooms[rows[:65]] = 0
        at, label = 65, 1
    while at < B - min(2, B // 3) and label < N_TABLE - 1:
        n = int(rng.integers(1, 10))
        rooms[rows[at:at + n]] = label
        at, label = at + n, label + 1
    return rooms


def _draw_script(seed):
    """The operations of one sequence, drawn on the CPU: a shuffled multiset of KINDS, each kind's B running through a
    permutation of B_SET.  Between resets a decoder serves hop-synchronous calls or DecodeSamples requests, not both, and a
    stream's rate belongs to the stream, on either side (lyra_hip.h): `form`, `enc_rate` and `dec_rate` track what every id
    holds -- an import under another id moves them with the state, the ticks and the span calls here run at 16 kHz -- and a
    reset is put in front of an operation that finds too few ids it may name.  In front of the drawn operations WARM `enc`
    operations take the QUIET encoders through three hops of speech into room noise; every later `enc` operation names some
    of them beside streams with speech, so that its DTX rows give empty and full packets."""
    rng = np.random.Generator(np.random.PCG64(7000 + seed))
    kinds = [k for k, n in KINDS.items() for _ in range(n)]
    kinds = ["enc"] * WARM + [kinds[i] for i in rng.permutation(len(kinds))]
    sizes = {k: [B_SET[i] for i in rng.permutation(4)] for k in KINDS}
    sizes["enc"] += [37] * WARM                      # (popped first: the warm-up has all of QUIET in every operation)
    speakers = {k: [(1, 3, 8, 3)[i] for i in rng.permutation(4)] for k in ("speakers", "shared")}
    form = np.zeros(POOL, np.int8)                   # 0: fresh, 1: hop-synchronous, 2: DecodeSamples
    enc_rate, dec_rate = np.zeros(POOL, np.int32), np.zeros(POOL, np.int32)     # 0: none yet
    heard = np.zeros(MS, np.int32)                   # hops a QUIET encoder has been given
    ops = []

    def forget(ids):
        form[ids], enc_rate[ids], dec_rate[ids] = 0, 0, 0

    def pick(B, ok):
        ok = ok.copy()
        if ok.sum() < B:
            other = rng.permutation(np.flatnonzero(~ok))[:B - int(ok.sum()) + 8].astype(np.int32)
            ops.append(dict(kind="reset", ids=other))
            forget(other)
            ok[other] = True
        cand = np.flatnonzero(ok)
        return cand[rng.permutation(cand.size)][:B].astype(np.int32)

    def rates_of(ids, table):
        """the streams' rates; one is drawn where a stream has none yet"""
        r = table[ids].copy()
        r[r == 0] = rng.choice(RATES, int((r == 0).sum()))
        table[ids] = r
        return r.astype(np.int32)

    def at16(table):
        return (table == 0) | (table == 16000)

    def packets(n):
        return rng.integers(0, 256, (n, 23), dtype=np.uint8), rng.choice(SIZES, n, p=[0.3, 0.2, 0.2, 0.3]).astype(np.int32)

    for kind in kinds:
        B = sizes[kind].pop() if sizes[kind] else int(rng.choice(B_SET))
        op = dict(kind=kind)
        if kind == "reset":
            op["ids"] = rng.permutation(POOL)[:B].astype(np.int32)
            forget(op["ids"])
        elif kind == "enc":
            q = QUIET[rng.permutation(QUIET.size)][:max(1, min(B // 3, QUIET.size)) if B != 37 else QUIET.size]
            loud = pick(B - q.size, np.ones(POOL, bool))
            rows = rng.permutation(B)                # (the quiet rows scattered over the batch)
            ids, rates, dtx = np.zeros(B, np.int32), np.zeros(B, np.int32), rng.integers(0, 2, B).astype(np.int32)
            ids[rows[:q.size]], rates[rows[:q.size]], dtx[rows[:q.size]] = q, 16000, 1
            ids[rows[q.size:]], rates[rows[q.size:]] = loud, rates_of(loud, enc_rate)
            pcm = rng.integers(-12000, 12000, (B, ROW)).astype(np.int16)
            pcm[rows[:q.size][heard[q] >= 3]] //= 1500
            heard[q] += 1
            op.update(ids=ids, pcm=pcm, rates=rates, bits=_draw_bits(rng, B), dtx=dtx)
        elif kind in ("dec_streams", "lossy_rates"):
            ids = pick(B, form != 2)
            form[ids] = 1
            pk, sz = packets(B)
            op.update(ids=ids, pk=pk, sz=sz, rates=rates_of(ids, dec_rate))
        elif kind == "lossy_mixed":              # one rate for the call: 16 kHz
            ids = pick(B, (form != 2) & at16(dec_rate))
            form[ids], dec_rate[ids] = 1, 16000
            pk, sz = packets(B)
            op.update(ids=ids, pk=pk, sz=sz)
        elif kind == "samples":
            ids = pick(B, form != 1)
            form[ids] = 2
            pk, sz = packets(B)
            rates = rates_of(ids, dec_rate)
            ns = np.array([rng.choice([n for n in REQUESTS if n * 50 <= 4 * r]) for r in rates], np.int32)
            rn = np.stack([np.full(MAXB, 16000, np.int32), np.full(MAXB, 320, np.int32)])   # (the whole buffer, one upload)
            rn[0, :B], rn[1, :B] = rates, ns
            op.update(ids=ids, pk=pk, sz=sz, rn=rn)
        elif kind in ("bridge", "speakers", "shared"):   # both legs at 16 kHz
            if kind != "bridge":                 # (the full mix has no speaker count)
                op["N"] = N = speakers[kind].pop()
            rooms = _draw_rooms(rng, B)
            order, start = np_bridge_plan(rooms)
            if kind == "shared":     # encoder ids from the whole context, so partly the participants' own
                E = (start.size - 1) * (1 + N)
                ids = pick(B, (form != 2) & at16(dec_rate))
                e_ids = pick(E, at16(enc_rate))      # (a reset in front of this draw leaves the participants eligible: fresh)
                enc_rate[e_ids] = 16000
                op.update(e_ids=e_ids, e_bits=_draw_bits(rng, max(E, 1))[:E], e_dtx=(np.arange(E) % 2).astype(np.int32))
            else:
                ids = pick(B, (form != 2) & at16(dec_rate) & at16(enc_rate))
                enc_rate[ids] = 16000
            form[ids], dec_rate[ids] = 1, 16000
            pk, sz = packets(B)
            op.update(ids=ids, pk=pk, sz=sz, rooms=rooms, order=order, start=start, muted=(rng.random(B) < 0.15).astype(np.int32),
                      bits=_draw_bits(rng, B), dtx=rng.integers(0, 2, B).astype(np.int32))
        elif kind == "expimp":
            src = rng.permutation(POOL)[:B].astype(np.int32)
            dst = rng.permutation(POOL)[:B].astype(np.int32)
            op.update(ids=src, dst=dst)
            form[dst], enc_rate[dst], dec_rate[dst] = form[src].copy(), enc_rate[src].copy(), dec_rate[src].copy()
        elif kind == "spans_enc":    # two spans of 60 hops at 16 kHz on the 8 lent lanes, a gap in front of each
            ids = pick(2, at16(enc_rate))
            enc_rate[ids] = 16000
            op.update(ids=ids, spans=[(int(ids[0]), 1, 60), (int(ids[1]), 63, 60)],
                      pcm=rng.integers(-12000, 12000, (SPAN_F, 320)).astype(np.int16))
        else:
            ids = pick(2, (form != 2) & at16(dec_rate))
            form[ids], dec_rate[ids] = 1, 16000
            op.update(ids=ids, spans=[(int(ids[0]), 1, 60), (int(ids[1]), 63, 60)],
                      pk=rng.integers(0, 256, (SPAN_F, 15), dtype=np.uint8),
                      pb=(rng.choice([0, 15], SPAN_F, p=[0.3, 0.7])).astype(np.int32))
        ops.append(op)
    return ops


def _check_script(ops):
    """what a sequence has to exercise, as far as the drawn script shows it (before the first device call)"""
    counts = {}
    for op in ops:
        counts[op["kind"]] = counts.get(op["kind"], 0) + 1
    assert set(counts) == set(KINDS) and all(counts[k] >= n for k, n in KINDS.items()), counts
    # (the decoders' input: rows without a packet beside rows with one.  What the DTX encoders put out is asserted on the
    # reference's results, _run_sequence)
    lossy = sum(int((op["sz"] == 0).any() and (op["sz"] > 0).any()) for op in ops if "sz" in op)
    assert lossy > 5, "the decoders never met missing and received packets in one call"
    for kind in ("bridge", "speakers", "shared"):
        big = [np.bincount(op["rooms"][op["rooms"] >= 0]).max() for op in ops if op["kind"] == kind]
        assert max(big) == 65 and min(big) <= 9, (kind, big)
    for kind in ("speakers", "shared"):
        assert {op["N"] for op in ops if op["kind"] == kind} == {1, 3, 8}, kind
    assert sum(np.intersect1d(op["e_ids"], op["ids"]).size for op in ops if op["kind"] == "shared") >= 4, \
        "no encoder id of a shared tick is a participant's own"
    assert len({op["ids"].size for op in ops if op["kind"] == "enc"}) == 4
    assert len(ops) <= 60, len(ops)
    return counts


class _Set:
    """One buffer set: every input with a valid earlier content (ids distinct and in range, sizes 0, legal rates, bit counts
    and request sizes), so that a call that read too early would compute a wrong answer and nothing else; every output."""

    def __init__(self, blob_bytes):
        import torch
        d = _dev()
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=d)            # noqa: E731
        full = lambda n, v: torch.full((n,), v, dtype=torch.int32, device=d)      # noqa: E731
        ar = lambda n: torch.arange(n, dtype=torch.int32, device=d)               # noqa: E731
        self.ids, self.dst, self.e_ids, self.order = ar(MAXB), ar(MAXB), ar(E_MAX), ar(MAXB)
        self.pk, self.sz = z((MAXB, 23), torch.uint8), full(MAXB, 0)
        self.rates, self.bits, self.dtx, self.muted = full(MAXB, 16000), full(MAXB, 64), full(MAXB, 0), full(MAXB, 0)
        self.rn = torch.stack([full(MAXB, 16000), full(MAXB, 320)])
        self.e_bits, self.e_dtx = full(E_MAX, 64), full(E_MAX, 0)
        self.start = full(N_TABLE + 1, 0)
        self.pcm = z((MAXB, ROW), torch.int16)
        self.span_pcm, self.span_pk = z((SPAN_F, 320), torch.int16), z((SPAN_F, 15), torch.uint8)
        # outputs
        self.out_pk, self.out_n = z((MAXB, 23), torch.uint8), z((MAXB,), torch.int32)
        self.pcm16, self.ext, self.mix = z((MAXB, 320), torch.int16), z((MAXB, ROW), torch.int16), z((MAXB, 320), torch.int16)
        self.samples = z((MAXB, 4 * ROW), torch.int16)
        self.isn, self.icn, self.spk, self.slot_of = (z((MAXB,), torch.int32) for _ in range(4))
        self.levels = z((MAXB,), torch.int64)
        self.enc_mix, self.enc_pk, self.enc_n = z((E_MAX, 320), torch.int16), z((E_MAX, 23), torch.uint8), z((E_MAX,), torch.int32)
        self.blobs = z((MAXB, blob_bytes), torch.uint8)
        self.span_out_pk, self.span_16 = z((SPAN_F, 15), torch.uint8), z((SPAN_F, 320), torch.int16)
        self.span_isn, self.span_icn = z((SPAN_F,), torch.int32), z((SPAN_F,), torch.int32)


def _padded_ids(ids, n, avoid=()):
    """`ids` followed by other ids of the context up to n entries, all distinct: the whole buffer is uploaded, so what a later,
    shorter call would find behind its own rows is valid as well"""
    rest = np.setdiff1d(np.arange(MS, dtype=np.int32), np.concatenate([ids, np.asarray(avoid, np.int32)]))
    return np.concatenate([ids, rest])[:n].astype(np.int32)


def _host_inputs(op):
    """name of the set's buffer -> the array that goes into its first rows"""
    kind, h = op["kind"], {}
    for k in ("pk", "sz", "rates", "bits", "dtx", "muted", "order", "start", "e_bits", "e_dtx", "rn"):
        if k in op and kind not in ("spans_lossy",):
            h[k] = op[k]
    if kind not in ("reset", "spans_enc", "spans_lossy"):
        h["ids"] = _padded_ids(op["ids"], MAXB)
    if kind == "expimp":
        h["dst"] = _padded_ids(op["dst"], MAXB)
    if kind == "shared":
        h["e_ids"] = _padded_ids(op["e_ids"], E_MAX)
    if kind == "enc":
        h["pcm"] = op["pcm"]
    if kind == "spans_enc":
        h["span_pcm"] = op["pcm"]
    if kind == "spans_lossy":
        h["span_pk"] = op["pk"]
    return h


def _issue(c, s, op, table):
    """the operation's device call(s) on context c and buffer set s -> [(name, tensor)] of everything it writes"""
    kind = op["kind"]
    B = op["ids"].size
    ids, pk, sz, rates = s.ids[:B], s.pk[:B], s.sz[:B], s.rates[:B]
    if kind == "enc":
        outs = [("packets", s.out_pk[:B]), ("packet sizes", s.out_n[:B])]
        call = lambda: c.encode_streams_dev(ids, s.pcm[:B], rates, s.bits[:B], s.out_pk[:B], s.out_n[:B], s.dtx[:B])   # noqa: E731
    elif kind == "dec_streams":
        outs = [("pcm at the rows' rates", s.ext[:B]), ("pcm16", s.pcm16[:B]), ("is_noise", s.isn[:B]), ("is_comfort_noise", s.icn[:B])]
        call = lambda: c.decode_streams_dev(ids, pk, sz, rates, s.ext[:B], None, s.pcm16[:B], s.isn[:B], s.icn[:B])     # noqa: E731
    elif kind == "lossy_mixed":
        outs = [("pcm16", s.pcm16[:B]), ("is_noise", s.isn[:B]), ("is_comfort_noise", s.icn[:B])]
        call = lambda: c.decode_lossy_mixed_dev(ids, pk, sz, 16000, s.pcm16[:B], None, s.isn[:B], s.icn[:B])            # noqa: E731
    elif kind == "lossy_rates":
        outs = [("pcm at the rows' rates", s.ext[:B]), ("pcm16", s.pcm16[:B]), ("is_noise", s.isn[:B]), ("is_comfort_noise", s.icn[:B])]
        call = lambda: c.decode_lossy_rates_dev(ids, pk, sz, rates, s.pcm16[:B], s.ext[:B], s.isn[:B], s.icn[:B])       # noqa: E731
    elif kind == "samples":
        outs = [("samples", s.samples[:B]), ("is_noise", s.isn[:B]), ("is_comfort_noise", s.icn[:B])]
        call = lambda: c.decode_samples_streams_dev(ids, pk, sz, s.rn[0, :B], s.rn[1, :B], 4, s.samples[:B], None,      # noqa: E731
                                                    s.isn[:B], s.icn[:B])
    elif kind in ("bridge", "speakers", "shared"):
        nm, nr, N = op["order"].size, op["start"].size - 1, op.get("N")
        order, start, muted = s.order[:nm], s.start[:nr + 1], s.muted[:B]
        outs = [("out packets", s.out_pk[:B]), ("out sizes", s.out_n[:B]), ("pcm16", s.pcm16[:B]), ("is_noise", s.isn[:B]),
                ("is_comfort_noise", s.icn[:B])]
        if kind == "bridge":
            outs += [("mix", s.mix[:B])]
            call = lambda: c.bridge_tick_dev(ids, pk, sz, order, start, s.bits[:B], s.out_pk[:B], s.out_n[:B], muted,   # noqa: E731
                                             s.dtx[:B], 0, s.pcm16[:B], s.mix[:B], s.isn[:B], s.icn[:B])
        elif kind == "speakers":
            outs += [("mix", s.mix[:B]), ("levels", s.levels[:B]), ("is_speaker", s.spk[:B])]
            call = lambda: c.speakers_tick_dev(ids, pk, sz, order, start, s.bits[:B], s.out_pk[:B], s.out_n[:B], N,     # noqa: E731
                                               muted, s.dtx[:B], 0, s.pcm16[:B], s.mix[:B], s.isn[:B], s.icn[:B],
                                               s.levels[:B], s.spk[:B])
        else:
            E = nr * (1 + N)
            outs += [("levels", s.levels[:B]), ("is_speaker", s.spk[:B]), ("slot_of", s.slot_of[:B]), ("enc_mix", s.enc_mix[:E]),
                     ("enc packets", s.enc_pk[:E]), ("enc sizes", s.enc_n[:E])]
            call = lambda: c.shared_tick_dev(ids, pk, sz, order, start, s.out_pk[:B], s.out_n[:B], N, table, s.e_ids[:E],   # noqa: E731
                                             s.e_bits[:E], None, s.e_dtx[:E], muted, 0, s.pcm16[:B], s.isn[:B], s.icn[:B],
                                             s.levels[:B], s.spk[:B], s.enc_mix[:E], s.enc_pk[:E], s.enc_n[:E], s.slot_of[:B])
    elif kind == "expimp":
        outs = [("blobs", s.blobs[:B])]

        def call():
            c.export_streams_dev(ids, s.blobs[:B])
            c.import_streams_dev(s.dst[:B], s.blobs[:B])
    elif kind == "spans_enc":
        outs = [("span packets", s.span_out_pk)]
        call = lambda: c.encode_spans_dev(op["spans"], s.span_pcm, SPAN_BITS, s.span_out_pk, LANES)                     # noqa: E731
    else:
        outs = [("span pcm16", s.span_16), ("span is_noise", s.span_isn), ("span is_comfort_noise", s.span_icn)]
        call = lambda: c.decode_spans_lossy_dev(op["spans"], s.span_pk, op["pb"], SPAN_BITS, s.span_16, LANES, 16000, None,   # noqa: E731
                                                s.span_isn, s.span_icn)
    for _, t in outs:
        t.zero_()                    # (on the caller's stream: the call is ordered behind it)
    call()
    return outs


@pytest.mark.parametrize("seed,sub_batches", [(0, 1), (1, 1), (2, 1), (3, 2)])
def test_unsynchronised_sequences_of_the_later_calls_equal_the_synchronised_reference(seed, sub_batches):
    _run_sequence(seed, sub_batches)


def _run_sequence(seed, sub_batches, every=5):
    """Two passes.  First `ref` alone runs the whole script, one operation at a time with a synchronise after each; every output
    and the slot table after every operation are kept on the host, and what the sequence has to exercise on the device's
    outputs is asserted.  Then `x` runs it from the late stream: no lyra_hip_synchronize and no device synchronise until the
    closing state check, pinned upload buffers made beforehand.  Results are read with .cpu() on the caller's stream after every
    `every`-th operation (the last two each time) and at the end.  What still waits on the host, by the library's own
    contract: lyra_hip_reset_streams drains the context, and decode_spans_lossy_dev blocks once for its control words."""
    import torch
    ops = _draw_script(seed)
    counts = _check_script(ops)
    ref = make_ctx(MS, cng_seed=7, streams="plain")
    x = make_ctx(MS, cng_seed=7, streams="plain", sub_batches=sub_batches)
    try:
        assert x.torch_order
        blob = x.stream_blob_bytes()
        # ---- the reference pass ----
        rset = _Set(blob)
        table_r = torch.full((N_TABLE, 8), -1, dtype=torch.int32, device=_dev())
        keep, tables, hosts = {}, {}, {}
        moved = shared_ticks = 0
        dtx_flips, empties = {}, {}
        for t, op in enumerate(ops):
            if op["kind"] == "reset":
                ref.reset(op["ids"])
                keep[t] = []
            else:
                hosts[t] = {name: np.ascontiguousarray(a).reshape(-1) for name, a in _host_inputs(op).items()}
                for name, a in hosts[t].items():
                    getattr(rset, name).view(-1)[:a.size].copy_(torch.from_numpy(a))
                before = table_r.cpu().numpy()
                outs = _issue(ref, rset, op, table_r)
                ref.synchronize()
                torch.cuda.synchronize()
                keep[t] = [(name, v.cpu().numpy().copy()) for name, v in outs]
                if op["kind"] == "shared":
                    shared_ticks += 1
                    moved += int(shared_ticks > 1 and not np.array_equal(before, table_r.cpu().numpy()))
                if op["kind"] in ("enc", "bridge", "speakers", "shared"):     # the encoders' own decisions: sizes of 0 under DTX
                    n = dict(keep[t])["enc sizes" if op["kind"] == "shared" else "packet sizes" if op["kind"] == "enc" else "out sizes"]
                    dtx_flips[op["kind"]] = dtx_flips.get(op["kind"], 0) + int((n == 0).any() and (n > 0).any())
                    empties[op["kind"]] = empties.get(op["kind"], 0) + int((n == 0).sum())
            tables[t] = table_r.cpu().numpy().copy()
        print(f"seed {seed}: {len(ops)} operations {counts}; slot table moved in {moved} of {shared_ticks} shared ticks; operations "
              f"whose encoders gave empty and full packets {dtx_flips}, empty packets {empties}")
        assert moved >= 1, "the sequence never moved the slot table"
        assert dtx_flips.get("enc", 0) > 5, "the DTX encoders of encode_streams_dev never mixed empty and full packets"
        assert ref.bridge_errors() == 0 and ref.import_errors() == 0 and ref.rates_errors() == 0 \
            and ref.encode_mixed_errors() == 0 and ref.decode_lossy_errors() == 0
        # ---- the pass under test ----
        sets = [_Set(blob), _Set(blob)]
        table_x = torch.full((N_TABLE, 8), -1, dtype=torch.int32, device=_dev())
        pinned = {t: {name: _pinned(a) for name, a in h.items()} for t, h in hosts.items()}
        late = late_stream(4.0)
        torch.cuda.synchronize()                     # the last one until the closing checks
        pending = {}
        for t, op in enumerate(ops):
            if op["kind"] == "reset":
                x.reset(op["ids"])
                pending[t] = []
            else:
                s = sets[t & 1]
                with torch.cuda.stream(late.stream):
                    for k, (name, p) in enumerate(pinned[t].items()):
                        late.upload(getattr(s, name).view(-1)[:p.numel()], p, late=k == 0)
                    pending[t] = _issue(x, s, op, table_x)
            if t % every == every - 1 or t == len(ops) - 1:
                with torch.cuda.stream(late.stream):
                    for tt in (t - 1, t):
                        for (name, want), (_, got) in zip(keep[tt], pending[tt]):
                            g = got.cpu().numpy()             # on the caller's stream alone: behind lyra_hip_stream_wait
                            bad = np.argwhere((g != want).reshape(g.shape[0], -1))
                            assert bad.size == 0, (f"op {tt} ({ops[tt]['kind']}, seed {seed}): {name} differs at (row, column)",
                                                   bad[:8].tolist(), "of", len(bad))
                    assert np.array_equal(table_x.cpu().numpy(), tables[t]), f"op {t} ({op['kind']}, seed {seed}): the slot table"
        print(f"seed {seed}: late work {late.total_ms:.0f} ms")
        late.stream.synchronize()
        assert x.bridge_errors() == 0 and x.import_errors() == 0 and x.rates_errors() == 0 and x.encode_mixed_errors() == 0 \
            and x.decode_lossy_errors() == 0
        assert x.decode_samples_errors() == ref.decode_samples_errors()
        _same_state(x, ref, np.arange(MS, dtype=np.int32), "after the last operation")
    finally:
        torch.cuda.synchronize()
        x.close()
        ref.close()
