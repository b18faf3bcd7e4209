"""The host-buffer calls on PINNED caller memory, every buffer overwritten the moment the call returns.

include/lyra_hip.h ("Pipelined host-buffer calls") promises that the caller's buffers may be reused as soon as begin() / end()
returns, and a blocking host call promises it by its nature.  From pageable memory the runtime copies before hipMemcpyAsync
returns, so a call that did not wait for its upload cannot be told from one that did; from pinned memory (hipHostMalloc,
hipHostRegister, torch's pin_memory()) the copy is asynchronous, and "returned before the copy finished" reads the buffer's
LATER content.  On an idle GPU such a copy starts at once and normally wins the race against the host; here it cannot:

The instrument (gpu_plumbing.Held): the late caller of tests/test_gpu_order_later_calls.py enqueues a few milliseconds of
bounded torch work, lyra_hip_wait_for_stream puts the four library streams behind it, the hold is asserted to be live, the call
under test is made with every caller-owned input in pinned memory, and on return every input is overwritten (gpu_plumbing.scrub:
0x3333 samples, FILL bytes, 0x33333333 in the small int32 arrays; stream ids become OTHER ids of the context, not out-of-range
ones -- the kernels index the state by id unchecked, and a defect must show as a wrong answer, not as a wild write).  Outputs go
to pinned memory prefilled with FILL and are compared with nothing between the return and the comparison.  The late work is
sized by late_delay_ms from a synchronised timing of the same calls on the twin.  What is expected comes from a second context
of the same mode that is never held and is given pageable copies (the pair's `_dev` call plus explicit copies, or the blocking
host call); everything is compared bit for bit, and the exported state of every id of the context at the end.

The control (once per module, in the fixture every case uses, and reported by the first test): with the same hold a torch
stream is ordered behind the late stream, dst.copy_(pinned, non_blocking=True) runs on it, the pinned tensor is overwritten on
the host, the late work must still be pending then, and after a synchronise dst must hold the overwritten pattern: on this
machine a copy nobody waited for does read the buffer's later content.  Without that every case below would pass vacuously.

Cases: B = 37 on max_streams = 64 (ragged 8- and 16-row tiles, scattered ids).  Per pair one hop that is not held (first use: slots
are allocated, kernels loaded -- no hold of a few milliseconds outlasts that), then four hops in which every begin() and every
end() is a held call: one begin then end (no call in flight), three two deep, a final drain.

Out of scope: the twin-fetch pair (lyra_hip_twin_fetch_begin / _end) has no Python mirror, stages its inputs through the
context's own h_twin_args, and is driven only by the C++ classes, which tests/test_gpu_pipelined.py holds to the blocking
session.  Host-side races between threads are not what this instrument sees either.

Checked by hand on an MI355X: the control holds (5.1 ms of late work pending after the overwrite, the copy delivered the
overwritten pattern; the process's FIRST copy from pinned memory takes some 12 ms on the host, hence the control's warm-up
copy and the unheld first hop).  Against the library before lyra_hip_encode_begin waited for its upload in every branch, the
four encode_begin cases with sub_batches = 1 (16 kHz and 48 kHz with DTX, default and plain streams) failed at the first held
hop -- begin then end, no call in flight -- with the packets of all 37 rows wrong: begin() had returned with the late work
pending and the upload read the overwritten samples.  The two sub_batches = 2 cases passed there (that branch synchronised
already), as did decode_begin.  With the wait in place all pass, and no other call of the table was found to return early with
an upload outstanding: the blocking calls return with the late work over, the begin() calls of the bridge, decode_streams and
decode_samples_streams pairs return with it pending because they copy their small inputs into pinned slots on the host."""
import contextlib
import time

import numpy as np
import pytest

from gpu_plumbing import FILL, Held, _dev, _ids, _pinned, _t, late_delay_ms, late_stream, make_ctx, scrub
from row_cases import _same_state
from signals import RATES, _pcm_rows, synth

pytestmark = pytest.mark.gpu
MS, B, HOPS = 64, 37, 5      # hop 0 is not held: slots are allocated and kernels loaded there, no hold would outlast that
ALL_IDS = np.arange(MS, dtype=np.int32)
IDS = _ids(B, MS, 77)


# ---- the instrument ---------------------------------------------------------------------------------------------------------

def _control(late):
    """-> (the late work was pending after the host's overwrite, dst holds the overwritten pattern, ms of late work)"""
    import torch
    late.resize(5.0)
    src = _pinned(np.full((B, 320), 0x1111, np.int16))
    dst = torch.zeros((B, 320), dtype=torch.int16, device=_dev())
    side = torch.cuda.Stream(device=_dev())
    with torch.cuda.stream(side):            # (a process's first copy of this kind takes some 12 ms on the host)
        dst.copy_(src, non_blocking=True)
    torch.cuda.synchronize()
    late.hold()
    side.wait_stream(late.stream)
    with torch.cuda.stream(side):
        dst.copy_(src, non_blocking=True)
    scrub(src)
    pending = not late.stream.query()
    side.synchronize()
    late.stream.synchronize()
    return pending, bool((dst.cpu().numpy() == 0x3333).all()), late.reps * late.ms_per_matmul


class _Contexts:
    """The module's contexts by (sub_batches, streams), made on first use and reset for every case; one that a failing case
    leaves with calls in flight is closed and made anew."""

    def __init__(self):
        self.made = {}

    @contextlib.contextmanager
    def pair(self, sub_batches=None, streams=None, rate=16000):
        """(the context under test, its twin: default streams, unsplit), both reset, same DTX rate, same comfort-noise seed"""
        keys = [("x", sub_batches, streams), ("twin", None, None)]
        for k in keys:
            if k not in self.made:
                self.made[k] = make_ctx(MS, cng_seed=7, streams=k[2], sub_batches=k[1])
        x, twin = (self.made[k] for k in keys)
        try:
            for c in (x, twin):
                c.reset()
                c.set_encoder_sample_rate(rate)
                c.set_cng_seed(7)
            yield x, twin
        except BaseException:
            for k in keys:
                self.made.pop(k).close()
            raise

    def close(self):
        for c in self.made.values():
            c.close()
        self.made = {}


@pytest.fixture(scope="module")
def rig():
    """(the late caller, the contexts) of the module, behind the control: no case runs on an instrument that sees nothing"""
    import torch
    late = late_stream(5.0)
    pending, overwritten, ms = _control(late)
    print(f"control: {ms:.1f} ms of late work; pending after the host's overwrite: {pending}; the copy read the overwritten "
          f"pattern: {overwritten}")
    assert pending, "the late work was over before the host had overwritten the buffer: the hold is too short"
    assert overwritten, ("a copy from pinned memory that nobody waited for did not read the buffer's later content: on this "
                         "machine the instrument cannot see a begin() that returns early")
    contexts = _Contexts()
    yield late, contexts
    torch.cuda.synchronize()
    contexts.close()


@pytest.fixture
def late(rig):
    """the late caller with a fresh budget (LateStream.BUDGET_MS per test case), drained afterwards"""
    rig[0].total_ms = 0.0
    yield rig[0]
    rig[0].stream.synchronize()


def _timed(twin, fn):
    """fn() and a synchronise on the twin -> (fn's result, seconds)"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = fn()
    twin.synchronize()
    torch.cuda.synchronize()
    return got, time.perf_counter() - t0


def _two_deep(h, T, begin, end):
    """hop 0: begin then end, not held (first use); hop 1: begin then end (no call in flight); hops 2 .. T - 1 two deep; the
    last end() drains -> [end(t)]"""
    h.live = False
    begin(0)
    got = [end(0)]
    h.live = True
    begin(1)
    got.append(end(1))
    begin(2)
    for t in range(2, T):
        if t + 1 < T:
            begin(t + 1)
        got.append(end(t))
    assert h.calls == 2 * (T - 1)
    return got


def _filled_pinned(shape, dtype):
    """a pinned tensor, every byte FILL"""
    import torch
    t = torch.empty(shape, dtype=dtype, pin_memory=True)
    t.view(torch.uint8).fill_(FILL)
    return t


def _take(*outs):
    """the pinned outputs as they are on return (the read IS the comparison's: nothing is synchronised in front of it), and
    FILL put back"""
    import torch
    got = tuple(o.numpy().copy() for o in outs)
    for o in outs:
        o.view(torch.uint8).fill_(FILL)
    return got


def _compare(where, got, want, names):
    for t, (g, w) in enumerate(zip(got, want)):
        for name, x, y in zip(names, g, w):
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape, (where, t, name, x.shape, y.shape)
            rows = np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1))
            assert rows.size == 0, f"{where}, hop {t}: {name} differs in {rows.size} of {len(x)} rows, first {rows[:12].tolist()}"


def _finish(where, h, x, twin):
    print(f"{where}: {h.calls} held calls, {h.returned_early} returned with the late work pending, {h.late.total_ms:.0f} ms "
          f"of late work")
    h.late.stream.synchronize()
    _same_state(x, twin, ALL_IDS, where)


def test_control_and_buffers_passed_in_place(rig, late):
    """The control ran in the fixture (asserted there; its figures are printed with -s).  Here: what the cases hand to the
    Python mirror is read in place -- the address the mirror gives the ABI is the pinned tensor's."""
    from lyra_amd import codec
    for a, dtype, shape in ((synth(B, 1, 1)[0], np.int16, (-1, 320)), (np.zeros((B, 23), np.uint8), np.uint8, (-1, 23)),
                            (IDS, np.int32, (B,)), (np.zeros((B, 64), np.float32), np.float32, (-1, 64))):
        p = _pinned(a)
        assert p.is_pinned() and codec._np(p.numpy(), dtype, shape).ctypes.data == p.data_ptr()
    pending, overwritten, ms = _control(late)
    assert pending and overwritten, (pending, overwritten, ms)


# ---- lyra_hip_encode_begin / _end -------------------------------------------------------------------------------------------

def _encode_script(golden_dir, rate, dtx):
    """[WARM + HOPS][B][rate / 50]; with dtx rows 0, 5, 10, ... turn to near-silence after three hops of speech, so that the
    encoder-side estimator calls them noise inside the held hops"""
    warm = 6 if dtx else 0
    if rate == 16000:
        pcm = synth(B, warm + HOPS, 31)
    else:
        pcm = np.ascontiguousarray(_pcm_rows(golden_dir, B, warm + HOPS, [rate] * B, 0, 31, 0)[:, :, :rate // 50])
    if dtx:
        pcm[3:, ::5] //= 2000
    return pcm, warm


@pytest.mark.parametrize("sub_batches,streams", [(1, None), (2, None), (1, "plain")], ids=["sub1", "sub2", "sub1-plain"])
@pytest.mark.parametrize("rate,dtx,bits", [(16000, False, 184), (48000, True, 120)], ids=["16k", "48k-dtx"])
def test_encode_begin_end_on_pinned_buffers(rig, late, golden_dir, rate, dtx, bits, sub_batches, streams):
    import torch
    where = f"encode_begin {rate} Hz dtx={dtx} sub_batches={sub_batches} {streams or 'default'}"
    pcm, warm = _encode_script(golden_dir, rate, dtx)
    nbytes = (bits + 7) // 8
    with rig[1].pair(sub_batches, streams, rate) as (x, twin):
        d_ids, d_pk, d_len = _t(IDS), torch.zeros((B, nbytes), dtype=torch.uint8, device=_dev()), \
            torch.zeros((B,), dtype=torch.int32, device=_dev())

        def hop(c, t):
            """the hop through the `_dev` call that begin() is made of, on a pageable copy"""
            d_pk.zero_()
            c.encode_ext_dev(d_ids, _t(pcm[t].copy()), rate, bits, d_pk, d_len if dtx else None, dtx)
            c.synchronize()
            return d_pk.cpu().numpy(), d_len.cpu().numpy() if dtx else np.full(B, nbytes, np.int32)

        for t in range(warm):
            hop(x, t), hop(twin, t)
        want, seconds = [], 0.0
        for t in range(warm, warm + HOPS):
            w, s = _timed(twin, lambda: hop(twin, t))
            want.append(w)
            seconds = max(seconds, s)
        if dtx:
            empty = sum(int((w[1] == 0).sum()) for w in want)
            print(f"{where}: {empty} empty packets in {HOPS} hops")
            assert empty > 0 and all((w[1] > 0).any() for w in want), "the DTX rows gave no empty packet beside full ones"
        late.resize(late_delay_ms(seconds))
        L, h = x.L, Held(x, late)
        p_ids, p_pcm = _pinned(IDS), _pinned(pcm[0])
        o_pk, o_len = _filled_pinned((B + 1, nbytes), torch.uint8), _filled_pinned((B + 1,), torch.int32)   # (a guard row each)

        def begin(t):
            p_ids.copy_(torch.from_numpy(IDS))
            p_pcm.copy_(torch.from_numpy(pcm[warm + t]))
            h.call(lambda: x._chk(L.lyra_hip_encode_begin(x.h, p_ids.data_ptr(), B, p_pcm.data_ptr(), rate, bits, int(dtx))),
                   p_pcm, ids=[p_ids])

        def end(t):
            h.call(lambda: x._chk(L.lyra_hip_encode_end(x.h, o_pk.data_ptr(), o_len.data_ptr())))
            pk, n = _take(o_pk, o_len)
            assert (pk[B] == FILL).all() and n.view(np.uint8)[4 * B:].tolist() == [FILL] * 4, "end() wrote past its B rows"
            return pk[:B], n[:B]

        got = _two_deep(h, HOPS, begin, end)
        _compare(where, got, want, ("packets", "packet_bytes"))
        _finish(where, h, x, twin)


# ---- lyra_hip_decode_begin / _end -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sub_batches", [1, 2])
def test_decode_begin_end_on_pinned_buffers(rig, late, sub_batches):
    import torch
    where, bits, nbytes = f"decode_begin sub_batches={sub_batches}", 120, 15
    packets = np.random.default_rng(41).integers(0, 256, (HOPS, B, nbytes), dtype=np.uint8)
    with rig[1].pair(sub_batches) as (x, twin):
        want, seconds = [], 0.0
        for t in range(HOPS):
            w, s = _timed(twin, lambda: (twin.decode(packets[t].copy(), bits, IDS.copy()),))
            want.append(w)
            seconds = max(seconds, s)
        late.resize(late_delay_ms(seconds))
        L, h = x.L, Held(x, late)
        p_ids, p_pk = _pinned(IDS), _pinned(packets[0])
        o_pcm = _filled_pinned((B + 1, 320), torch.int16)

        def begin(t):
            p_ids.copy_(torch.from_numpy(IDS))
            p_pk.copy_(torch.from_numpy(packets[t]))
            h.call(lambda: x._chk(L.lyra_hip_decode_begin(x.h, p_ids.data_ptr(), B, p_pk.data_ptr(), bits)), p_pk, ids=[p_ids])

        def end(t):
            h.call(lambda: x._chk(L.lyra_hip_decode_end(x.h, o_pcm.data_ptr())))
            pcm, = _take(o_pcm)
            assert (pcm.view(np.uint8)[B] == FILL).all(), "end() wrote past its B rows"
            return (pcm[:B],)

        got = _two_deep(h, HOPS, begin, end)
        _compare(where, got, want, ("pcm",))
        _finish(where, h, x, twin)


# ---- lyra_hip_encode_streams_begin / _end, lyra_hip_decode_streams_begin / _end ------------------------------------------

ROW_RATES = np.array([RATES[(b // 3) % 4] for b in range(B)], np.int32)     # rows at all four rates
SIZES = np.array([0, 8, 15, 23], np.int32)


def _packed(rows, counts):
    """rows [B][width] -> row b's first counts[b] samples, back to back"""
    return np.concatenate([rows[b, :n] for b, n in enumerate(counts)])


def _p_all(**arrays):
    """name -> pinned tensor; the ABI reads them in place (data_ptr())"""
    return {k: _pinned(v) for k, v in arrays.items()}


def _refill(pinned, **arrays):
    import torch
    for k, v in arrays.items():
        pinned[k].copy_(torch.from_numpy(np.ascontiguousarray(v)))


def _but_ids(pinned):
    return [p for k, p in pinned.items() if not k.startswith("ids")]


def test_encode_streams_begin_end_on_pinned_buffers(rig, late, golden_dir):
    import torch
    where = "encode_streams_begin"
    rng = np.random.default_rng(61)
    bits = rng.choice([64, 120, 184, 4, 100], B).astype(np.int32)
    dtx = (np.arange(B) % 2).astype(np.int32)
    pcm = _pcm_rows(golden_dir, B, HOPS, ROW_RATES, 3, 4, 0)
    counts = ROW_RATES // 50
    with rig[1].pair() as (x, twin):
        d_pk, d_pb = torch.zeros((B, 23), dtype=torch.uint8, device=_dev()), torch.zeros((B,), dtype=torch.int32, device=_dev())

        def hop(t):
            d_pk.zero_()         # (end() hands over zeros behind each packet and for empty ones)
            twin.encode_streams_dev(_t(IDS), _t(pcm[t]), _t(ROW_RATES), _t(bits), d_pk, d_pb, _t(dtx))
            twin.synchronize()
            pk, pb = d_pk.cpu().numpy(), d_pb.cpu().numpy()
            for b in range(B):
                pk[b, pb[b]:] = 0
            return pk, pb

        want, seconds = [], 0.0
        for t in range(HOPS):
            w, s = _timed(twin, lambda: hop(t))
            want.append(w)
            seconds = max(seconds, s)
        late.resize(late_delay_ms(seconds))
        L, h = x.L, Held(x, late)
        p = _p_all(ids=IDS, pcm=_packed(pcm[0], counts), rates=ROW_RATES, bits=bits, dtx=dtx)
        o_pk, o_pb = _filled_pinned((B + 1, 23), torch.uint8), _filled_pinned((B + 1,), torch.int32)

        def begin(t):
            _refill(p, ids=IDS, pcm=_packed(pcm[t], counts), rates=ROW_RATES, bits=bits, dtx=dtx)
            h.call(lambda: x._chk(L.lyra_hip_encode_streams_begin(x.h, p["ids"].data_ptr(), B, p["pcm"].data_ptr(),
                                                                  p["rates"].data_ptr(), p["bits"].data_ptr(), p["dtx"].data_ptr())),
                   *_but_ids(p), ids=[p["ids"]])

        def end(t):
            h.call(lambda: x._chk(L.lyra_hip_encode_streams_end(x.h, o_pk.data_ptr(), o_pb.data_ptr())))
            pk, pb = _take(o_pk, o_pb)
            assert (pk[B] == FILL).all() and (pb.view(np.uint8)[4 * B:] == FILL).all(), "end() wrote past its B rows"
            return pk[:B], pb[:B]

        got = _two_deep(h, HOPS, begin, end)
        _compare(where, got, want, ("packets", "packet_bytes"))
        print(f"{where}: {sum(int((w[1] == 0).sum()) for w in want)} empty packets in {HOPS} hops")
        assert x.rates_errors() == 0 and x.encode_mixed_errors() == 0
        _finish(where, h, x, twin)


def test_decode_streams_begin_end_on_pinned_buffers(rig, late):
    import torch
    where = "decode_streams_begin"
    rng = np.random.default_rng(62)
    pk = rng.integers(0, 256, (HOPS, B, 23), dtype=np.uint8)
    sz = rng.choice(SIZES, (HOPS, B)).astype(np.int32)
    counts, total = ROW_RATES // 50, int(ROW_RATES.sum()) // 50
    with rig[1].pair() as (x, twin):
        def hop(t):
            d_pcm = torch.zeros((B, 960), dtype=torch.int16, device=_dev())
            dn, dc = (torch.zeros((B,), dtype=torch.int32, device=_dev()) for _ in range(2))
            twin.decode_streams_dev(_t(IDS), _t(pk[t]), _t(sz[t]), _t(ROW_RATES), d_pcm, None, None, dn, dc)
            twin.synchronize()
            return _packed(d_pcm.cpu().numpy(), counts), dn.cpu().numpy(), dc.cpu().numpy()

        want, seconds = [], 0.0
        for t in range(HOPS):
            w, s = _timed(twin, lambda: hop(t))
            want.append(w)
            seconds = max(seconds, s)
        late.resize(late_delay_ms(seconds))
        L, h = x.L, Held(x, late)
        p = _p_all(ids=IDS, pk=pk[0], sz=sz[0], rates=ROW_RATES)
        o_pcm, o_n, o_c = _filled_pinned((total + 8,), torch.int16), _filled_pinned((B + 1,), torch.int32), \
            _filled_pinned((B + 1,), torch.int32)

        def begin(t):
            _refill(p, ids=IDS, pk=pk[t], sz=sz[t], rates=ROW_RATES)
            h.call(lambda: x._chk(L.lyra_hip_decode_streams_begin(x.h, p["ids"].data_ptr(), B, p["pk"].data_ptr(),
                                                                  p["sz"].data_ptr(), p["rates"].data_ptr())),
                   *_but_ids(p), ids=[p["ids"]])

        def end(t):
            h.call(lambda: x._chk(L.lyra_hip_decode_streams_end(x.h, o_pcm.data_ptr(), o_n.data_ptr(), o_c.data_ptr())))
            pcm, n, c = _take(o_pcm, o_n, o_c)
            assert (pcm.view(np.uint8)[2 * total:] == FILL).all() and (n.view(np.uint8)[4 * B:] == FILL).all() \
                and (c.view(np.uint8)[4 * B:] == FILL).all(), "end() wrote past its rows"
            return pcm[:total], n[:B], c[:B]

        got = _two_deep(h, HOPS, begin, end)
        _compare(where, got, want, ("pcm", "is_noise", "is_comfort_noise"))
        assert x.rates_errors() == 0 and x.decode_lossy_errors() == 0
        _finish(where, h, x, twin)


# ---- the three kinds of bridge tick ---------------------------------------------------------------------------------------

ROOMS = np.concatenate([np.zeros(5, np.int32), 1 + np.arange(32, dtype=np.int32) // 4])    # one room of 5, eight rooms of 4
N_SPEAKERS = 3


def _tick_script(kind):
    from bridge_tick_cases import host_script
    script = host_script(B, HOPS, 71, lambda t, rng, rooms: ROOMS, per_listener=kind != "shared")
    if kind == "shared":
        labels = np.unique(ROOMS)
        cell = labels[:, None] * (1 + N_SPEAKERS) + np.arange(1 + N_SPEAKERS)[None, :]
        for s in script:    # the encoder settings of a room go with its label (after tests/test_gpu_shared_bridge.py)
            s["labels"] = labels.astype(np.int32)
            s["enc"] = (cell.astype(np.int32) % MS, np.array([64, 120, 184], np.int32)[cell % 3], (cell % 2).astype(np.int32))
    return script


@pytest.mark.parametrize("kind", ["bridge", "speakers", "shared"])
def test_bridge_ticks_begin_end_on_pinned_buffers(rig, late, kind):
    import torch
    from bridge_models import np_bridge_plan
    where = f"{kind}_begin"
    script = _tick_script(kind)
    order, start = np_bridge_plan(ROOMS)
    E = (start.size - 1) * (1 + N_SPEAKERS)
    with rig[1].pair() as (x, twin):
        if kind == "shared":
            x.shared_reset_rooms(script[0]["labels"])    # (the context is the module's: the rows of an earlier case)
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=_dev())   # noqa: E731
        table = torch.full((MS, 8), -1, dtype=torch.int32, device=_dev())

        def tick(s):
            """the `_dev` call of the kind on the twin -> what end() hands over, in its order"""
            out, out_n, isn, icn, spk, slot_of = z((B, 23), torch.uint8), *(z((B,), torch.int32) for _ in range(5))
            levels = z((B,), torch.int64)
            head = (_t(IDS), _t(s["pk"]), _t(s["sz"]), _t(order), _t(start))
            if kind == "bridge":
                twin.bridge_tick_dev(*head, _t(s["bits"]), out, out_n, _t(s["muted"]), _t(s["dtx"]), 0, None, None, isn, icn)
                outs = (out, out_n, isn, icn)
            elif kind == "speakers":
                twin.speakers_tick_dev(*head, _t(s["bits"]), out, out_n, N_SPEAKERS, _t(s["muted"]), _t(s["dtx"]), 0, None, None,
                                       isn, icn, levels, spk)
                outs = (out, out_n, isn, icn, levels, spk)
            else:
                e_ids, e_bits, e_dtx = (_t(np.ascontiguousarray(v).reshape(-1)) for v in s["enc"])
                twin.shared_tick_dev(*head, out, out_n, N_SPEAKERS, table, e_ids, e_bits, _t(s["labels"]), e_dtx, _t(s["muted"]), 0,
                                     None, isn, icn, levels, spk, None, None, None, slot_of)
                outs = (out, out_n, isn, icn, levels, spk, slot_of)
            twin.synchronize()
            got = [o.cpu().numpy() for o in outs]
            for b in range(B):
                got[0][b, got[1][b]:] = 0
            return tuple(got)

        want, seconds = [], 0.0
        for s in script:
            w, sec = _timed(twin, lambda: tick(s))
            want.append(w)
            seconds = max(seconds, sec)
        late.resize(late_delay_ms(seconds))
        h = Held(x, late)
        p = _p_all(ids=IDS, pk=script[0]["pk"], sz=script[0]["sz"], rooms=ROOMS)
        if kind != "shared":
            p.update(_p_all(bits=script[0]["bits"]))

        def begin(t):
            s = script[t]
            _refill(p, ids=IDS, pk=s["pk"], sz=s["sz"], rooms=ROOMS, **({} if kind == "shared" else {"bits": s["bits"]}))
            v = {k: t_.numpy() for k, t_ in p.items()}
            if kind == "bridge":
                fn = lambda: x.bridge_begin(v["pk"], v["sz"], v["rooms"], v["bits"], s["muted"], s["dtx"], 0, v["ids"])   # noqa: E731
            elif kind == "speakers":
                fn = lambda: x.speakers_begin(v["pk"], v["sz"], v["rooms"], v["bits"], N_SPEAKERS, s["muted"], s["dtx"], 0, v["ids"])   # noqa: E731
            else:
                fn = lambda: x.shared_begin(v["pk"], v["sz"], v["rooms"], N_SPEAKERS, s["labels"], *s["enc"], s["muted"], 0, v["ids"])   # noqa: E731
            h.call(fn, *_but_ids(p), ids=[p["ids"]])

        def end(t):
            return h.call({"bridge": x.bridge_end, "speakers": x.speakers_end, "shared": x.shared_end}[kind])

        got = _two_deep(h, HOPS, begin, end)
        names = ("out packets", "out sizes", "is_noise", "is_comfort_noise", "levels", "is_speaker", "slot_of")
        _compare(where, got, want, names[:len(want[0])])
        assert x.bridge_errors() == 0 and x.decode_lossy_errors() == 0 and x.encode_mixed_errors() == 0
        assert E == 9 * (1 + N_SPEAKERS)
        _finish(where, h, x, twin)


# ---- lyra_hip_decode_samples_any_begin / _end, lyra_hip_decode_samples_streams_begin / _end -------------------------------

REQUESTS = (160, 441, 1024)


@pytest.mark.parametrize("rate", [8000, 32000, 48000])
def test_decode_samples_any_begin_end_on_pinned_buffers(rig, late, rate):
    import torch
    where = f"decode_samples_any_begin {rate} Hz"
    rng = np.random.default_rng(81 + rate)
    ok = [n for n in REQUESTS if n * 50 <= 4 * rate]       # a request is at most four hops
    ns = [ok[(t + rate // 8000) % len(ok)] for t in range(HOPS)]
    pk = rng.integers(0, 256, (HOPS, B, 23), dtype=np.uint8)
    sz = rng.choice(SIZES, (HOPS, B)).astype(np.int32)
    with rig[1].pair() as (x, twin):
        def hop(t):
            d_pcm = torch.zeros((B, ns[t]), dtype=torch.int16, device=_dev())
            twin.decode_samples_any_dev(_t(IDS), _t(pk[t]), _t(sz[t]), ns[t], rate, d_pcm)
            twin.synchronize()
            return (d_pcm.cpu().numpy(),)

        want, seconds = [], 0.0
        for t in range(HOPS):
            w, s = _timed(twin, lambda: hop(t))
            want.append(w)
            seconds = max(seconds, s)
        late.resize(late_delay_ms(seconds))
        L, h = x.L, Held(x, late)
        p = _p_all(ids=IDS, pk=pk[0], sz=sz[0])
        o_pcm = _filled_pinned((B * max(ns) + 8,), torch.int16)

        def begin(t):
            _refill(p, ids=IDS, pk=pk[t], sz=sz[t])
            h.call(lambda: x._chk(L.lyra_hip_decode_samples_any_begin(x.h, p["ids"].data_ptr(), B, p["pk"].data_ptr(),
                                                                      p["sz"].data_ptr(), ns[t], rate)),
                   *_but_ids(p), ids=[p["ids"]])

        def end(t):
            h.call(lambda: x._chk(L.lyra_hip_decode_samples_any_end(x.h, o_pcm.data_ptr())))
            pcm, = _take(o_pcm)
            assert (pcm.view(np.uint8)[2 * B * ns[t]:] == FILL).all(), "end() wrote past its rows"
            return (pcm[:B * ns[t]].reshape(B, ns[t]),)

        got = _two_deep(h, HOPS, begin, end)
        _compare(where, got, want, ("pcm",))
        assert x.decode_samples_errors() == twin.decode_samples_errors()
        _finish(where, h, x, twin)


def test_decode_samples_streams_begin_end_on_pinned_buffers(rig, late):
    import torch
    where = "decode_samples_streams_begin"
    rng = np.random.default_rng(91)
    rates = np.array([(8000, 32000, 48000)[(b // 3) % 3] for b in range(B)], np.int32)
    ns = np.array([[[n for n in REQUESTS if n * 50 <= 4 * r][(b + t) % (2 if r == 8000 else 3)] for b, r in enumerate(rates)]
                   for t in range(HOPS)], np.int32)
    pk = rng.integers(0, 256, (HOPS, B, 23), dtype=np.uint8)
    sz = rng.choice(SIZES, (HOPS, B)).astype(np.int32)
    with rig[1].pair() as (x, twin):
        def hop(t):
            d_pcm = torch.zeros((B, 4 * 960), dtype=torch.int16, device=_dev())
            dn, dc = (torch.zeros((B,), dtype=torch.int32, device=_dev()) for _ in range(2))
            twin.decode_samples_streams_dev(_t(IDS), _t(pk[t]), _t(sz[t]), _t(rates), _t(ns[t]), 4, d_pcm, None, dn, dc)
            twin.synchronize()
            return _packed(d_pcm.cpu().numpy(), ns[t]), dn.cpu().numpy(), dc.cpu().numpy()

        want, seconds = [], 0.0
        for t in range(HOPS):
            w, s = _timed(twin, lambda: hop(t))
            want.append(w)
            seconds = max(seconds, s)
        late.resize(late_delay_ms(seconds))
        L, h = x.L, Held(x, late)
        p = _p_all(ids=IDS, pk=pk[0], sz=sz[0], rates=rates, ns=ns[0])
        cap = int(ns.sum(axis=1).max())
        o_pcm, o_n, o_c = _filled_pinned((cap + 8,), torch.int16), _filled_pinned((B + 1,), torch.int32), \
            _filled_pinned((B + 1,), torch.int32)

        def begin(t):
            _refill(p, ids=IDS, pk=pk[t], sz=sz[t], rates=rates, ns=ns[t])
            h.call(lambda: x._chk(L.lyra_hip_decode_samples_streams_begin(x.h, p["ids"].data_ptr(), B, p["pk"].data_ptr(),
                                                                          p["sz"].data_ptr(), p["rates"].data_ptr(),
                                                                          p["ns"].data_ptr())),
                   *_but_ids(p), ids=[p["ids"]])

        def end(t):
            total = int(ns[t].sum())
            h.call(lambda: x._chk(L.lyra_hip_decode_samples_streams_end(x.h, o_pcm.data_ptr(), o_n.data_ptr(), o_c.data_ptr())))
            pcm, n, c = _take(o_pcm, o_n, o_c)
            assert (pcm.view(np.uint8)[2 * total:] == FILL).all() and (n.view(np.uint8)[4 * B:] == FILL).all() \
                and (c.view(np.uint8)[4 * B:] == FILL).all(), "end() wrote past its rows"
            return pcm[:total], n[:B], c[:B]

        got = _two_deep(h, HOPS, begin, end)
        _compare(where, got, want, ("pcm", "is_noise", "is_comfort_noise"))
        assert x.rates_errors() == 0 and x.decode_samples_errors() == twin.decode_samples_errors()
        _finish(where, h, x, twin)


# ---- the blocking host calls ----------------------------------------------------------------------------------------------

def _blocking_cases(n):
    """name -> (inputs by name, ("ids...": stream ids), call(c, inputs) -> outputs) on n rows"""
    rng = np.random.default_rng(53)
    ids = _ids(n, MS, 77)
    pcm = synth(n, 1, 53)[0]
    pcm48 = rng.integers(-20000, 20000, (n, 960)).astype(np.int16)
    pk = rng.integers(0, 256, (n, 23), dtype=np.uint8)
    feat = rng.standard_normal((n, 64)).astype(np.float32)
    mel = rng.standard_normal((n, 160)).astype(np.float32)
    lanes = np.setdiff1d(ALL_IDS, ids)[:4].astype(np.int32)
    spans, F = [(int(ids[0]), 0, 30)], 30
    span_pcm = synth(F, 1, 54)[0]
    span_pb = rng.choice([0, 15], F, p=[0.3, 0.7]).astype(np.int32)
    return {
        "encode": (dict(pcm=pcm, ids=ids), lambda c, a: (c.encode(a["pcm"], 184, a["ids"]),)),
        "decode": (dict(pk=pk, ids=ids), lambda c, a: (c.decode(a["pk"], 184, a["ids"]),)),
        "encode_dtx": (dict(pcm=pcm // 3000, ids=ids), lambda c, a: c.encode_dtx(a["pcm"], 120, a["ids"])),
        "extract": (dict(pcm=pcm, ids=ids), lambda c, a: (c.extract(a["pcm"], a["ids"]),)),
        "generate": (dict(feat=feat, ids=ids), lambda c, a: (c.generate(a["feat"], a["ids"]),)),
        "logmel": (dict(pcm=pcm, ids=ids), lambda c, a: (c.logmel(a["pcm"], a["ids"]),)),
        "resample_48_16": (dict(pcm=pcm48, ids=ids), lambda c, a: (c.resample(a["pcm"], 48000, 16000, a["ids"]),)),
        "resample_16_48": (dict(pcm=pcm, ids=ids), lambda c, a: (c.resample(a["pcm"], 16000, 48000, a["ids"], side="decoder"),)),
        "noise_receive": (dict(pcm=pcm // 3000, ids=ids), lambda c, a: (c.noise_receive(a["pcm"], a["ids"]),)),
        "comfort_noise": (dict(mel=mel, ids=ids), lambda c, a: (c.comfort_noise(a["mel"], a["ids"]),)),
        "import_streams": (dict(blobs=None, ids=ids[::-1].copy()), lambda c, a: (c.import_streams(a["ids"], a["blobs"]), ())[1]),
        "export_streams": (dict(ids=ids), lambda c, a: (c.export_streams(a["ids"]),)),
        "encode_spans": (dict(pcm=span_pcm), lambda c, a: (c.encode_spans(spans, a["pcm"], 120, lanes),)),
        "decode_spans_lossy": (dict(pk=rng.integers(0, 256, (F, 15), dtype=np.uint8), pb=span_pb),
                               lambda c, a: tuple(o for o in c.decode_spans_lossy(spans, a["pk"], a["pb"], 120, lanes) if o is not None)),
        "encode_spans_packed": (dict(pcm=np.repeat(span_pcm, 2, axis=1).reshape(-1), bits=np.full(F, 120, np.int32)),
                                lambda c, a: c.encode_spans_packed(spans, a["pcm"], [32000], a["bits"], lanes)),
    }


def _held_blocking_call(rig, late, name, n):
    """one held call of the table on n rows, pinned inputs overwritten on return, against the twin's on pageable copies"""
    inputs, call = _blocking_cases(n)[name]
    where = f"{name}, B = {n}"
    warm = _blocking_cases(n)
    with rig[1].pair() as (x, twin):
        for c in (x, twin):      # both sides of every stream past their reset values
            for k in ("encode", "decode", "noise_receive"):
                warm[k][1](c, warm[k][0])
        if name == "import_streams":
            inputs["blobs"] = twin.export_streams(inputs["ids"][::-1].copy())
        for c in (x, twin):      # the call itself once, not held: what it allocates and loads on first use
            call(c, {k: v.copy() for k, v in inputs.items()})
        want, seconds = _timed(twin, lambda: call(twin, {k: v.copy() for k, v in inputs.items()}))
        late.resize(late_delay_ms(seconds))
        h = Held(x, late)
        p = _p_all(**inputs)
        views = {k: t.numpy() for k, t in p.items()}
        got = h.call(lambda: call(x, views), *_but_ids(p), ids=[t for k, t in p.items() if k.startswith("ids")])
        assert len(got) == len(want)
        _compare(where, [got], [want], [f"output {k}" for k in range(len(want))])
        _finish(where, h, x, twin)


BLOCKING = ("encode", "decode", "encode_dtx", "extract", "generate", "logmel", "resample_48_16", "resample_16_48", "noise_receive",
            "comfort_noise", "import_streams", "export_streams", "encode_spans", "decode_spans_lossy", "encode_spans_packed")


@pytest.mark.parametrize("name", BLOCKING)
def test_blocking_host_calls_on_pinned_buffers(rig, late, name):
    _held_blocking_call(rig, late, name, B)


# lyra_hip_ctx::ZC_MAX (api.hip) is 16: a blocking call of at most 16 rows that goes through HostIO (extract, generate and the
# two quantizer calls) copies into and out of the pinned, device-mapped arena on the host and enqueues no copy at all; from 17
# rows on it uploads with hipMemcpyAsync from the caller's memory.  encode and decode always take the second way.
@pytest.mark.parametrize("n", [16, 17])
@pytest.mark.parametrize("name", ["encode", "decode", "extract", "generate"])
def test_small_call_arena_threshold_on_pinned_buffers(rig, late, name, n):
    _held_blocking_call(rig, late, name, n)
