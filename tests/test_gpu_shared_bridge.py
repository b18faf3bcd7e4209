"""The loudest-N bridge with shared encoders on the device (include/lyra_hip_shared_bridge.h): the kernels against the model
(two successive updates, permuted keys into a larger table, sentinels, a bad index, a bad key), the scripted conference with
its slot events, the tick against the calls it composes, free slots carrying the room's packet, the two-deep host form against
the `_dev` call with its refusals, bridge_demo --shared-encoders, and the argument checks.  Helpers:
tests/shared_bridge_models.py, tests/bridge_tick_cases.py.

Shapes.  The slot kernel serves one room per wavefront and the mix kernel one encoder row, four per workgroup, the fan-out 256
bytes per workgroup: the kernel cases of the loudest-N test (B = 330, rooms of 1 .. 257, and rooms of 63 / 64 / 65 / 129) give
8 and 4 rooms, E = 16 .. 72 encoder rows; B = 37 and B = 5 for the tick.

Stream kind: the contexts here (64 to 512 streams) run on the CU-masked streams the library picks up to 1,024 streams, which
are blocking streams with respect to the NULL stream; the cases with streams="plain" run on hipStreamNonBlocking streams, the
kind of a 4,096-stream context (tests/gpu_plumbing.py make_ctx)."""
import numpy as np
import pytest

from bridge_models import np_bridge_plan
from bridge_tick_cases import (Bufs, TickKind, begin, begin_end_ticks, compose_case, demo_conference, host_script,
                               rooms_redrawn_every_fourth_tick, run_demo)
from gpu_plumbing import _dev, _ids, _t, make_ctx as _ctx, stream_cases
from row_cases import _draw_bits, _same_state
from shared_bridge_models import EVENTS, SLOTS, np_fanout, np_shared_mix, run_slot_script, slot_script
from speaker_models import SKIP_CN, np_levels, speakers_kernel_case, threshold_case

EINVAL = -1
MIX_FILL, LEVEL_FILL, FLAG_FILL, TABLE_FILL = 0x3333, 0x5555555555555555, 0x77777777, 0x66666666


# ---- 1. the kernels against the model -------------------------------------------------------------------------------------

class _MixBufs:
    """Every output of shared_mix_dev with sentinels behind it; the table with sentinel rows where no room has its key"""

    def __init__(self, B, E, n_table, keys):
        import torch
        f = lambda n, v, dt: torch.full((n,), v, dtype=dt, device=_dev())   # noqa: E731
        self.B, self.E = B, E
        self.mix = torch.full((E + 2, 320), MIX_FILL, dtype=torch.int16, device=_dev())
        self.levels = f(B + 3, LEVEL_FILL, torch.int64)
        self.flags, self.slot_of = f(B + 3, FLAG_FILL, torch.int32), f(B + 3, FLAG_FILL, torch.int32)
        table = np.full((n_table + 1, SLOTS), TABLE_FILL, np.int32)
        table[keys[(keys >= 0) & (keys < n_table)]] = -1
        self.table = _t(table)

    def run(self, a, x, ids, order, start, N, keys, muted, is_cn):
        B, E = self.B, self.E
        a.shared_mix_dev(_t(x), _t(ids), _t(order), _t(start), self.table[:-1], self.mix[:E], N, _t(keys), _t(muted),
                         None if is_cn is None else _t(is_cn), self.levels[:B], self.flags[:B], self.slot_of[:B])
        a.synchronize()
        mix, levels, flags, slot_of, table = (t.cpu().numpy() for t in (self.mix, self.levels, self.flags, self.slot_of, self.table))
        assert (mix[E:] == MIX_FILL).all(), "rows behind the encoder mixes were written"
        assert (levels[B:] == LEVEL_FILL).all() and (flags[B:] == FLAG_FILL).all() and (slot_of[B:] == FLAG_FILL).all(), \
            "words behind the levels / flags / slot_of were written"
        assert (table[-1] == TABLE_FILL).all(), "the row behind the table was written"
        return mix[:E], levels[:B], flags[:B], slot_of[:B], table[:-1].copy()


def _check_mix(got, want, what):
    for name, g, w in zip(("enc_mix", "levels", "is_speaker", "slot_of", "table"), got, want):
        assert np.array_equal(g, w), (what, name, "differs in rows", np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[:16])


def _two_updates(a, x, rooms, ids, order, start, N, muted, is_cn, what, keeps=True):
    """-> (bufs, second x, the model's result of the second update): the update from an empty table, then one from the table
    it left with the loudness ranks turned over (row b takes the audio of row B - 1 - b); keeps: some speaker must stay one"""
    B, n_rooms = x.shape[0], start.size - 1
    n_table = n_rooms + 5
    keys = np.random.default_rng(n_rooms).permutation(n_table)[:n_rooms].astype(np.int32)
    bufs = _MixBufs(B, n_rooms * (1 + N), n_table, keys)
    table0 = bufs.table.cpu().numpy()[:-1]
    want = np_shared_mix(x, ids, order, start, N, table0, keys, muted, is_cn)[:5]
    _check_mix(bufs.run(a, x, ids, order, start, N, keys, muted, is_cn), want, what + ", first update")
    x2 = np.ascontiguousarray(x[::-1])
    want2 = np_shared_mix(x2, ids, order, start, N, want[4], keys, muted, is_cn)[:5]
    kept = (want2[4][keys] == want[4][keys]) & (want[4][keys] >= 0)
    assert not np.array_equal(want2[4], want[4]) and (kept.any() or not keeps), "the second update must keep some slots and move others"
    _check_mix(bufs.run(a, x2, ids, order, start, N, keys, muted, is_cn), want2, what + ", second update")
    assert (want2[4][np.setdiff1d(np.arange(n_table), keys)] == TABLE_FILL).all()
    return bufs, keys, x2, want2


@pytest.fixture(scope="module")
def kernel_case():
    return speakers_kernel_case()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 3, 8])
def test_kernels_equal_the_model_and_survive_a_bad_index_and_a_bad_key(kernel_case, N):
    x, rooms, muted, is_cn, order, start = kernel_case
    B = x.shape[0]
    ids = _ids(B, 512, 40 + N)
    a = _ctx(512)
    try:
        bufs, keys, x2, want2 = _two_updates(a, x, rooms, ids, order, start, N, muted, is_cn, f"N = {N}")
        assert a.bridge_errors() == 0
        n_table = keys.size + 5
        table2 = want2[4]

        def fresh():
            bufs.table[:-1].copy_(_t(table2))

        # the three bad entries of the loudest-N test: counted once each, the rooms with a good index unchanged
        broken = order.copy()
        hit = [int(start[3]), int(start[6]) + 100, int(start[7]) + 5]
        broken[hit] = [-1, B, 2 ** 30]
        fresh()
        got = bufs.run(a, x2, ids, broken, start, N, keys, muted, is_cn)
        assert a.bridge_errors(clear=True) == 3 and a.bridge_errors() == 0
        keep = np.ones(order.size, bool)
        keep[hit] = False
        less_start = np.array([keep[:s].sum() for s in start], np.int32)
        _check_mix(got, np_shared_mix(x2, ids, order[keep], less_start, N, table2, keys, muted, is_cn)[:5], f"N = {N}, bad entries")
        good = np.setdiff1d(np.arange(keys.size), [3, 6, 7])
        want3 = np_shared_mix(x2, ids, order, start, N, table2, keys, muted, is_cn)
        assert np.array_equal(got[4][keys[good]], want3[4][keys[good]]), "rooms with a good index changed their slots"
        # room boundaries outside [0, n_members] are clamped: nothing faults, nothing behind the buffers is written
        wild = start.copy()
        wild[1], wild[-1] = -5, 2 ** 30
        fresh()
        got = bufs.run(a, x2, ids, order, wild, N, keys, muted, is_cn)
        assert np.array_equal(got[1], want3[1]) and a.bridge_errors() == 0
        # one bad key (and a negative one in a second run): counted once, the room's encoder rows hear zeros and its members hold no
        # slot, its table row and every other room unchanged
        for bad_room, bad_key in ((6, n_table), (2, -3)):
            bad = keys.copy()
            bad[bad_room] = bad_key
            fresh()
            got = bufs.run(a, x2, ids, order, start, N, bad, muted, is_cn)
            assert a.bridge_errors(clear=True) == 1
            want = np_shared_mix(x2, ids, order, start, N, table2, bad, muted, is_cn)[:5]
            _check_mix(got, want, f"N = {N}, bad key")
            assert np.array_equal(got[4][keys[bad_room]], table2[keys[bad_room]])
            rows = slice(bad_room * (1 + N), (bad_room + 1) * (1 + N))
            assert not got[0][rows].any() and (got[3][rooms == sorted(set(rooms[rooms >= 0]))[bad_room]] == -1).all()
    finally:
        a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 3, 8])
def test_kernels_at_the_room_sizes_around_64(N):
    x, rooms, muted, order, start = threshold_case()
    assert np.diff(start).tolist() == [63, 64, 65, 129]
    a = _ctx(512)
    try:
        _two_updates(a, x, rooms, _ids(x.shape[0], 512, 50 + N), order, start, N, muted, None, f"N = {N}", keeps=N == 8)
        assert a.bridge_errors() == 0
    finally:
        a.close()


@pytest.mark.gpu
def test_the_scripted_conference_keeps_its_slots_on_the_device():
    import torch
    ticks, ids, keys, n_table = slot_script()
    want, seen = run_slot_script(ticks, ids, keys, n_table, fill=TABLE_FILL)
    assert len(ticks) >= 40 and all(seen[e] >= 1 for e in EVENTS), seen     # (on the CPU, before anything goes to the device)
    a = _ctx(64)
    try:
        table = np.full((n_table, SLOTS), TABLE_FILL, np.int32)
        table[keys] = -1
        table = _t(table)
        B = ids.size
        for t, w in enumerate(want):
            N, tick = w["N"], w["tick"]
            if tick["poke"]:
                q, j, src = tick["poke"]
                table[q, j] = table[q, src]
            assert np.array_equal(table.cpu().numpy(), w["before"]), f"tick {t}: the table before the tick"
            mix = torch.zeros((2 * (1 + N), 320), dtype=torch.int16, device=_dev())
            levels = torch.zeros(B, dtype=torch.int64, device=_dev())
            flags, slot_of = (torch.zeros(B, dtype=torch.int32, device=_dev()) for _ in range(2))
            a.shared_mix_dev(_t(tick["x"]), _t(ids), _t(w["order"]), _t(w["start"]), table, mix, N, _t(keys), None, None, levels,
                             flags, slot_of)
            a.synchronize()
            got = tuple(v.cpu().numpy() for v in (mix, levels, flags, slot_of, table))
            _check_mix(got, (w["enc_mix"], w["levels"], w["is_speaker"], w["slot_of"], w["after"]), f"tick {t}")
        assert a.bridge_errors() == 0
    finally:
        a.close()


# ---- 2. the tick equals its composition -----------------------------------------------------------------------------------

NAMES = ("out sizes", "out packets", "pcm16", "is_noise", "is_comfort_noise", "levels", "is_speaker", "slot_of", "enc_mix",
         "enc packets", "enc sizes")


def _TickBufs(B, e_max):
    """Every output of one tick with B rows and room for E_max encoder rows"""
    return Bufs(B, NAMES, e_max)


def _labels(rooms):
    return np.array(sorted(set(int(v) for v in rooms if v >= 0)), np.int32)


def _shared_tick(a, bufs, table, ids, pk, sz, rooms, muted, flags, N, enc, keys=None):
    """enc: (ids, bits, dtx) [n_rooms][1 + N] each; keys None: the room labels"""
    order, start = np_bridge_plan(rooms)
    E = (start.size - 1) * (1 + N)
    keys = _labels(rooms) if keys is None else keys
    bufs.enc_pk.zero_()
    e_ids, e_bits, e_dtx = (_t(np.ascontiguousarray(v).reshape(-1)) for v in enc)
    a.shared_tick_dev(_t(ids), _t(pk), _t(sz), _t(order), _t(start), bufs.out, bufs.out_n, N, table, e_ids, e_bits, _t(keys),
                      e_dtx, _t(muted), flags, bufs.pcm16, bufs.isn, bufs.icn, bufs.levels, bufs.spk, bufs.enc_mix[:E],
                      bufs.enc_pk[:E], bufs.enc_n[:E], bufs.slot_of)
    a.synchronize()
    return bufs.read(E)


def _composed_tick(u, bufs, table, ids, pk, sz, rooms, muted, flags, N, enc, keys=None):
    """On the twin: the lossy decode at 16 kHz, a synchronise, the numpy model (which updates `table`, a numpy array, in place),
    the encode on E rows, a numpy fan-out."""
    import torch
    B = ids.size
    order, start = np_bridge_plan(rooms)
    E = (start.size - 1) * (1 + N)
    keys = _labels(rooms) if keys is None else keys
    u.decode_lossy_mixed_dev(_t(ids), _t(pk), _t(sz), 16000, bufs.pcm16, None, bufs.isn, bufs.icn)
    u.synchronize()
    x, icn = bufs.pcm16.cpu().numpy(), bufs.icn.cpu().numpy()
    enc_mix, levels, spk, slot_of, new, _ = np_shared_mix(x, ids, order, start, N, table, keys, muted, icn if flags & SKIP_CN else None)
    table[:] = new
    bufs.enc_pk.zero_()
    if E:
        bufs.enc_mix[:E].copy_(torch.from_numpy(enc_mix))
        e_ids, e_bits, e_dtx = (_t(np.ascontiguousarray(v).reshape(-1)) for v in enc)
        u.encode_streams_dev(e_ids, bufs.enc_mix[:E], _t(np.full(E, 16000, np.int32)), e_bits, bufs.enc_pk[:E], bufs.enc_n[:E],
                             e_dtx, _t(np.arange(E, dtype=np.int32) * 320), 320 * E)
        u.synchronize()
    out, out_n = np_fanout(bufs.enc_pk.cpu().numpy(), bufs.enc_n.cpu().numpy(), B, order, start, slot_of, N, keys, table.shape[0])
    for t, v in ((bufs.out, out), (bufs.out_n, out_n), (bufs.levels, levels), (bufs.spk, spk), (bufs.slot_of, slot_of)):
        t.copy_(torch.from_numpy(v))
    return bufs.read(E)


def _enc_settings(rng, rooms, N, ids, ms, bits=None, dtx=None):
    """Encoder ids / bits / DTX [n_rooms][1 + N]: the ids drawn from the whole context, so partly equal to participants' ids"""
    n_rooms = _labels(rooms).size
    E = n_rooms * (1 + N)
    pool = np.concatenate([ids[:E // 2 + 1], np.setdiff1d(np.arange(ms, dtype=np.int32), ids)])[:max(E, 1)]
    e_ids = pool[rng.permutation(pool.size)][:E].astype(np.int32)
    e_bits = _draw_bits(rng, max(E, 1))[:E] if bits is None else np.full(E, bits, np.int32)
    e_dtx = (np.arange(E) % 2).astype(np.int32) if dtx is None else np.full(E, dtx, np.int32)
    return tuple(v.reshape(n_rooms, 1 + N) for v in (e_ids, e_bits, e_dtx))


class _SharedEncoders(TickKind):
    names = NAMES
    ms, seed, id_offset = 128, 200, 5

    def prepare(self, c, rng):
        if c.flags & SKIP_CN:
            c.muted[2:4] = 1
        c.enc = [_enc_settings(rng, r, c.N, c.ids, c.ms) for r in c.rooms]
        assert np.intersect1d(c.enc[0][0], c.ids).size >= 1, "some encoder ids must coincide with participants' ids"
        c.state_ids = np.union1d(c.ids, np.concatenate([e[0].reshape(-1) for e in c.enc])).astype(np.int32)
        n_table = 12                # (the labels, which are the keys here, reach 9)
        c.table_u = np.full((n_table, SLOTS), -1, np.int32)
        c.table_a = _t(c.table_u)

    def bufs(self, c):
        return _TickBufs(c.B, max(e[0].size for e in c.enc))

    def draw(self, c, rng):
        """(bit counts and DTX flags belong to the encoder rows: nothing is drawn per tick)"""

    def tick(self, c, a, bufs, pk, sz, rooms):
        c.before = c.table_u.copy()
        return _shared_tick(a, bufs, c.table_a, c.ids, pk, sz, rooms, c.muted, c.flags, c.N, c.enc[c.t >= 20])

    def composed(self, c, u, bufs, pk, sz, rooms):
        return _composed_tick(u, bufs, c.table_u, c.ids, pk, sz, rooms, c.muted, c.flags, c.N, c.enc[c.t >= 20])

    def observe(self, c, t, rooms, got, want):
        assert np.array_equal(c.table_a.cpu().numpy(), c.table_u), f"tick {t}: the slot table"
        c.count["moved"] += int(t > 0 and not np.array_equal(c.before, c.table_u))
        c.count["shared"] += int((np.unique(want[1][want[0] > 0], axis=0).shape[0]) < int((want[0] > 0).sum()))

    def verdict(self, c):
        assert c.count["moved"] >= 2 and c.count["shared"] >= c.T // 4, "the table never changed, or no packet was ever shared"


def _compose_case(B, mode="xnnpack", N=2, **kw):
    compose_case(_SharedEncoders(), B, mode, N=N, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("B,mode,streams", stream_cases([(37, "xnnpack"), (5, "xnnpack"), (37, "builtin_mixed")],
                                                        plain=(37, "xnnpack")))
def test_tick_equals_its_composition(B, mode, streams):
    _compose_case(B, mode, streams=streams)


@pytest.mark.gpu
def test_tick_equals_its_composition_in_serial_order():
    _compose_case(37, serial=True)


@pytest.mark.gpu
def test_tick_equals_its_composition_on_a_split_context():
    _compose_case(37, sub_batches=2)


@pytest.mark.gpu
def test_tick_equals_its_composition_without_comfort_noise_rows():
    _compose_case(37, flags=SKIP_CN)


# ---- 3. free slots carry the room's packet --------------------------------------------------------------------------------

@pytest.mark.gpu
def test_free_slots_carry_the_rooms_packet_bit_for_bit():
    """One room of 8, N = 3, every encoder row at 184 bits without DTX, on a fresh context.  Rows 0 and 1 are the only sources
    until row 1 is muted for good at tick `gone`: slot 2 is free from the start, slot 1 from `gone` on.  The encoder of a free
    slot hears what the room's common row hears; after as many hops as the encoder remembers -- the warm-up of the span code
     -- it is in the same state and emits the same packets."""
    import lyra_amd
    W = lyra_amd.codec.span_warmup_frames("encoder")
    B, ms, N, gone = 8, 32, 3, 4
    T = gone + W + 3
    rng = np.random.default_rng(77)
    ids = _ids(B, ms, 3)
    rooms = np.zeros(B, np.int32)
    enc = (np.array([[ms - 1, ms - 2, ms - 3, ms - 4]], np.int32), np.full((1, 4), 184, np.int32), np.zeros((1, 4), np.int32))
    a = _ctx(ms)
    try:
        bufs = _TickBufs(B, 4)
        table = _t(np.full((1, SLOTS), -1, np.int32))
        differed, vac = 0, None          # vac: the encoder row of the slot that row 1 holds, then leaves
        for t in range(T):
            muted = np.ones(B, np.int32)
            muted[:1 if t >= gone else 2] = 0
            pk = rng.integers(0, 256, (B, 23), dtype=np.uint8)
            got = _shared_tick(a, bufs, table, ids, pk, np.full(B, 23, np.int32), rooms, muted, 0, N, enc)
            slot_of, enc_mix, enc_pk, enc_n = got[7], got[8], got[9], got[10]
            assert (enc_n == 23).all() and got[5][:2].min() > 0, f"tick {t}: a decoded hop of silence, or an empty packet"
            if t == 0:
                vac = 1 + int(slot_of[1])
                assert sorted(slot_of[:2].tolist()) == [0, 1]
            assert slot_of[0] == 2 - vac and slot_of[1] == (vac - 1 if t < gone else -1) and (slot_of[2:] == -1).all(), f"tick {t}"
            assert np.array_equal(enc_pk[3], enc_pk[0]), f"tick {t}: slot 2, free from the start, does not carry the room's packet"
            assert np.array_equal(enc_mix[3], enc_mix[0])
            if t < gone:
                differed += int(not np.array_equal(enc_pk[vac], enc_pk[0]))
            else:
                assert np.array_equal(enc_mix[vac], enc_mix[0]), f"tick {t}: the vacated slot does not hear the room"
            if t >= gone + W:
                assert np.array_equal(enc_pk[vac], enc_pk[0]), \
                    f"tick {t}: the slot vacated at tick {gone} still differs from the room's packet after {W} hops"
        assert differed == gone, "the slot's packets must differ from the room's while it is taken"
    finally:
        a.close()


# ---- 4. library scratch ---------------------------------------------------------------------------------------------------

def _host_ticks(B, T, seed, N):
    """T ticks of host arrays for shared_begin: rooms of 6 at first, redrawn every fourth tick (five rooms of about 7 and rows
    in no room), nobody in any room at tick 9; the encoder settings of a room go with its label."""
    ticks = host_script(B, T, seed, rooms_redrawn_every_fourth_tick(B), per_listener=False)
    for t, s in enumerate(ticks):
        if t == 9:
            s["rooms"] = np.full(B, -1, np.int32)
        s["labels"] = _labels(s["rooms"])
        cell = s["labels"][:, None] * (1 + N) + np.arange(1 + N)[None, :]
        s["enc"] = (cell.astype(np.int32), np.array([64, 120, 184], np.int32)[cell % 3], (cell % 2).astype(np.int32))
    return ticks


def _begin(c, s, N, ids, flags=0):
    begin(c, s, ids, flags, N)


@pytest.mark.gpu
def test_tick_with_library_scratch_for_the_optional_outputs():
    import torch
    B, ms, T, N = 37, 64, 12, 2
    ids = _ids(B, ms, 1)
    script = _host_ticks(B, T, 5, N)
    a, u = _ctx(ms), _ctx(ms)
    try:
        bufs = _TickBufs(B, ms)
        table_a, table_u = (_t(np.full((ms, SLOTS), -1, np.int32)) for _ in range(2))
        out, out_n = torch.zeros((B, 23), dtype=torch.uint8, device=_dev()), torch.zeros(B, dtype=torch.int32, device=_dev())
        for t, s in enumerate(script):
            want = _shared_tick(u, bufs, table_u, ids, s["pk"], s["sz"], s["rooms"], s["muted"], SKIP_CN, N, s["enc"])
            order, start = np_bridge_plan(s["rooms"])
            e_ids, e_bits, e_dtx = (_t(np.ascontiguousarray(v).reshape(-1)) for v in s["enc"])
            a.shared_tick_dev(_t(ids), _t(s["pk"]), _t(s["sz"]), _t(order), _t(start), out, out_n, N, table_a, e_ids, e_bits,
                              _t(s["labels"]), e_dtx, _t(s["muted"]), SKIP_CN)
            a.synchronize()
            assert np.array_equal(out_n.cpu().numpy(), want[0]) and np.array_equal(out.cpu().numpy(), want[1]), f"tick {t}"
            assert torch.equal(table_a, table_u), f"tick {t}: the slot table"
        _same_state(a, u, np.arange(ms, dtype=np.int32), "after the last tick")
    finally:
        a.close()
        u.close()


# ---- 5. shared_begin / shared_end equal the `_dev` call -------------------------------------------------------------------

def _want_ticks(u, ids, script, N, flags, ms, reset_at=None):
    """The `_dev` call on the twin with a table of its own, keyed by label -> the outputs of every tick"""
    bufs, table = _TickBufs(ids.size, ms), _t(np.full((ms, SLOTS), -1, np.int32))
    want = []
    for t, s in enumerate(script):
        if reset_at and t == reset_at[0]:
            table[_t(reset_at[1]).long()] = -1
        want.append(_shared_tick(u, bufs, table, ids, s["pk"], s["sz"], s["rooms"], s["muted"], flags, N, s["enc"]))
    return want


def _same_tick(got, w, t):
    out, out_n, isn, icn, levels, spk, slot_of = got
    assert np.array_equal(out_n, w[0]) and np.array_equal(out, w[1]), f"tick {t}: packets"
    assert np.array_equal(isn, w[3]) and np.array_equal(icn, w[4]), f"tick {t}: flags"
    assert np.array_equal(levels, w[5]) and np.array_equal(spk, w[6]) and np.array_equal(slot_of, w[7]), f"tick {t}: levels, flags, slots"
    assert np.array_equal(levels, np_levels(w[2]))


@pytest.mark.gpu
@pytest.mark.parametrize("depth,streams", stream_cases([1, 2], plain=2))
def test_begin_end_equal_the_dev_call(depth, streams):
    B, ms, T, N = 37, 64, 16, 3
    ids = _ids(B, ms, 11)
    script = _host_ticks(B, T, 21, N)
    a, u = _ctx(ms, streams=streams), _ctx(ms, streams=streams)
    try:
        want = _want_ticks(u, ids, script, N, SKIP_CN, ms)
        got = begin_end_ticks(a, script, a.shared_end, depth, ids, SKIP_CN, N)
        for t in range(T):
            _same_tick(got[t], want[t], t)
        assert sum(int((g[6] >= 0).sum()) for g in got) > T and not got[9][1].any() and not got[9][0].any()
        _same_state(a, u, np.arange(ms, dtype=np.int32), "after the last tick")
    finally:
        a.close()
        u.close()


@pytest.mark.gpu
def test_reset_rooms_frees_the_rows_of_the_labels_given():
    B, ms, T, N = 37, 64, 8, 3
    ids = _ids(B, ms, 13)
    script = _host_ticks(B, T, 23, N)
    gone = np.array([1, 3, 40], np.int32)           # two rooms of the script, and a label that has never been used
    a, u, v = _ctx(ms), _ctx(ms), _ctx(ms)
    try:
        want = _want_ticks(u, ids, script, N, 0, ms, reset_at=(3, gone))
        plain = _want_ticks(v, ids, script[:4], N, 0, ms)
        assert not np.array_equal(plain[3][7], want[3][7]), "the reset must change who holds which slot at tick 3"
        with pytest.raises(Exception, match="outside"):
            a.shared_reset_rooms([0, ms])
        a.shared_reset_rooms(gone)                  # before the first tick: there is no table yet
        for t, s in enumerate(script):
            _begin(a, s, N, ids)
            if t == 2:
                a.shared_reset_rooms(gone)          # tick 2 is in flight: drained first, and still to be ended
            _same_tick(a.shared_end(), want[t], t)
        _same_state(a, u, np.arange(ms, dtype=np.int32), "after the last tick")
    finally:
        for c in (a, u, v):
            c.close()


@pytest.mark.gpu
def test_begin_refusals_enqueue_nothing_and_the_three_kinds_of_tick_share_one_queue():
    import lyra_amd
    Err = lyra_amd.codec.LyraHipError
    B, ms, N = 37, 64, 3
    ids = _ids(B, ms, 12)
    s = _host_ticks(B, 4, 22, N)
    every = np.arange(ms, dtype=np.int32)
    a, u = _ctx(ms), _ctx(ms)
    L = a.L
    try:
        for c in (a, u):
            _begin(c, s[0], N, ids)
            c.shared_end()
        before = a.export_streams(every)

        def refused(match, N=N, ids=ids, **change):
            t = dict(s[1], **change)
            with pytest.raises(Err, match=match):
                a.shared_begin(t["pk"], t["sz"], t["rooms"], N, t["labels"], *t["enc"], t["muted"], 0, ids)

        e_ids, e_bits, e_dtx = s[1]["enc"]
        labels = s[1]["labels"]
        for bad in (0, 9, -1):
            refused("max_speakers", N=bad)
        refused("room_labels", labels=labels[::-1].copy())                         # not ascending
        refused("room_labels", labels=np.where(labels == labels[2], ms + 1, labels).astype(np.int32))   # not below max_streams
        wrong = labels.copy()
        wrong[-1] += 1
        refused("room_labels", labels=wrong)                                        # a label that no row has
        refused("shape|room_labels|size", labels=labels[:-1].copy(), enc=tuple(v[:-1] for v in s[1]["enc"]))   # a room left out
        twice = e_ids.copy()
        twice[1, 2] = twice[0, 0]
        refused("twice", enc=(twice, e_bits, e_dtx))
        far = e_ids.copy()
        far[0, 1] = ms
        refused("outside", enc=(far, e_bits, e_dtx))
        odd = e_bits.copy()
        odd[2, 0] = 66
        refused("divisible", enc=(e_ids, odd, e_dtx))
        size = s[1]["sz"].copy()
        size[5] = 9
        refused("packet of 9 bytes", sz=size)
        refused("twice", ids=np.where(np.arange(B) == 4, ids[3], ids).astype(np.int32))
        alone = np.arange(B, dtype=np.int32)                                        # 37 rooms x 4 encoder rows > 64 streams
        cell = alone[:, None] * 4 + np.arange(4)[None, :]
        with pytest.raises(Err, match="exceed max_streams"):
            a.shared_begin(s[1]["pk"], s[1]["sz"], alone, N, alone, cell % ms, np.full((B, 4), 64), None, None, 0, ids)
        with pytest.raises(Err):
            a.shared_end()                                   # nothing in flight
        assert np.array_equal(a.export_streams(every), before), "a refused begin() changed stream state"
        # one queue of two for all three kinds; a third tick of any kind is refused
        full = lambda c, t: c.bridge_begin(t["pk"], t["sz"], t["rooms"], np.full(B, 120, np.int32), t["muted"], None, 0, ids)   # noqa: E731
        loud = lambda c, t: c.speakers_begin(t["pk"], t["sz"], t["rooms"], np.full(B, 120, np.int32), N, t["muted"], None, 0, ids)   # noqa: E731
        _begin(a, s[1], N, ids)
        loud(a, s[2])
        for third in (lambda: _begin(a, s[3], N, ids), lambda: loud(a, s[3]), lambda: full(a, s[3])):
            with pytest.raises(Err, match="two ticks"):
                third()
        rates = np.full(B, 16000, np.int32)
        with pytest.raises(Err):
            a.decode_streams_begin(s[1]["pk"], s[1]["sz"], rates, ids)
        with pytest.raises(Err):
            a.encode_streams_begin(np.zeros(B * 320, np.int16), rates, np.full(B, 64, np.int32), None, ids)
        with pytest.raises(Err):
            a.export_streams(ids)
        # an end() of another kind on the oldest tick is refused and consumes nothing, in every direction
        with pytest.raises(Err, match="shared_begin"):
            a.speakers_end()
        with pytest.raises(Err, match="shared_begin"):
            a.bridge_end()
        got1 = a.shared_end()
        with pytest.raises(Err, match="oldest tick"):
            a.shared_end()
        got2 = a.speakers_end()
        full(a, s[3])
        with pytest.raises(Err, match="oldest tick"):
            a.shared_end()
        got3 = a.bridge_end()
        for c_begin, c_end, t, got in ((lambda t: _begin(u, t, N, ids), u.shared_end, s[1], got1), (lambda t: loud(u, t), u.speakers_end, s[2], got2),
                                       (lambda t: full(u, t), u.bridge_end, s[3], got3)):
            c_begin(t)
            for g, w in zip(got, c_end()):
                assert np.array_equal(g, w)
        _same_state(a, u, every, "after the refusals")
        # the other direction: a hop of either streams pipeline in flight refuses a tick
        a.decode_streams_begin(s[1]["pk"], s[1]["sz"], rates, ids)
        with pytest.raises(Err, match="another pipelined"):
            _begin(a, s[1], N, ids)
        a.decode_streams_end()
        a.encode_streams_begin(np.zeros(B * 320, np.int16), rates, np.full(B, 64, np.int32), None, ids)
        with pytest.raises(Err, match="another pipelined"):
            _begin(a, s[1], N, ids)
        a.encode_streams_end()
        assert L.lyra_hip_shared_end(a.h, None, None, None, None, None, None, None) == EINVAL
    finally:
        a.close()
        u.close()


# ---- 6. argument checks of the `_dev` calls -------------------------------------------------------------------------------

@pytest.mark.gpu
def test_dev_argument_checks_refuse_and_leave_the_context_alone():
    import torch
    from lyra_amd.codec import C, SharedTick
    B, ms, N = 12, 32, 2
    ids = _ids(B, ms, 2)
    rng = np.random.default_rng(9)
    rooms = (np.arange(B) // 4).astype(np.int32)
    order, start = np_bridge_plan(rooms)
    n_rooms, E = 3, 9
    enc = (np.arange(ms - E, ms, dtype=np.int32).reshape(3, 3), np.full((3, 3), 120, np.int32), np.ones((3, 3), np.int32))
    a, u = _ctx(ms), _ctx(ms)
    L = a.L
    try:
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=_dev())   # noqa: E731
        keep = dict(ids=_t(ids), pk=_t(rng.integers(0, 256, (B, 23), dtype=np.uint8)), sz=_t(np.full(B, 23, np.int32)),
                    order=_t(order), start=_t(start), out=z((B, 23), torch.uint8), out_n=z(B, torch.int32),
                    x=z((B + 1, 320), torch.int16), mix=z((E + 1, 320), torch.int16), slots=_t(np.full((4, SLOTS), -1, np.int32)),
                    e_ids=_t(enc[0].reshape(-1)), e_bits=_t(enc[1].reshape(-1)))
        p = {k: v.data_ptr() for k, v in keep.items()}
        torch.cuda.synchronize()   # (the calls below go to the library directly, without the binding's stream ordering)

        def tick(**change):
            f = dict(d_stream_ids=p["ids"], B=B, d_packets=p["pk"], d_packet_bytes=p["sz"], d_order=p["order"],
                     d_room_start=p["start"], n_rooms=n_rooms, n_members=order.size, d_muted=None, flags=0, d_out_packets=p["out"],
                     d_out_packet_bytes=p["out_n"], d_pcm16=p["x"], d_is_noise=None, d_is_comfort_noise=None, max_speakers=N,
                     d_levels=None, d_is_speaker=None, d_room_keys=None, d_slots=p["slots"], n_table_rooms=4,
                     d_enc_stream_ids=p["e_ids"], d_enc_num_bits=p["e_bits"], d_enc_dtx=None, d_enc_mix=p["mix"],
                     d_enc_packets=None, d_enc_packet_bytes=None, d_slot_of=None)
            f.update(change)
            t = SharedTick(**f)
            return L.lyra_hip_shared_tick_dev(a.h, C.addressof(t))

        for change in (dict(d_stream_ids=None), dict(d_packets=None), dict(d_packet_bytes=None), dict(d_out_packets=None),
                       dict(d_out_packet_bytes=None), dict(d_order=None), dict(d_room_start=None), dict(d_slots=None),
                       dict(d_enc_stream_ids=None), dict(d_enc_num_bits=None), dict(n_table_rooms=0), dict(B=0), dict(B=ms + 1),
                       dict(n_rooms=-1), dict(n_rooms=B + 1), dict(n_members=-1), dict(n_members=B + 1), dict(flags=4),
                       dict(d_pcm16=p["x"] + 2), dict(d_enc_mix=p["mix"] + 8), dict(d_enc_mix=p["x"]), dict(max_speakers=0),
                       dict(max_speakers=9), dict(max_speakers=-1), dict(n_rooms=B, max_speakers=8)):   # (12 x 9 rows > 32 streams)
            assert tick(**change) == EINVAL, change
        assert L.lyra_hip_shared_tick_dev(a.h, None) == EINVAL

        def mix(x=p["x"], i=p["ids"], n=B, o=p["order"], s=p["start"], nr=n_rooms, nm=order.size, k=N, slots=p["slots"], nt=4,
                out=p["mix"]):
            return L.lyra_hip_shared_mix_dev(a.h, x, i, n, o, s, nr, nm, None, None, k, None, slots, nt, out, None, None, None)

        for kw in (dict(x=None), dict(i=None), dict(out=None), dict(slots=None), dict(o=None), dict(s=None), dict(n=0),
                   dict(n=ms + 1), dict(nr=-1), dict(nr=B + 1), dict(nm=B + 1), dict(x=p["x"] + 2), dict(out=p["mix"] + 4),
                   dict(out=p["x"]), dict(k=0), dict(k=9), dict(k=-1), dict(nt=0)):
            assert mix(**kw) == EINVAL, kw
        keep["mix"].fill_(7)
        torch.cuda.synchronize()
        assert mix() == 0 and mix(nr=0, nm=0, o=None, s=None) == 0      # an empty index is a valid one: no encoder row at all
        a.synchronize()
        got = keep["mix"].cpu().numpy()
        assert not got[:E].any() and (got[E] == 7).all() and (keep["slots"].cpu().numpy() == -1).all()
        # a valid tick now matches a twin that never saw a bad call
        ba, bu = _TickBufs(B, E), _TickBufs(B, E)
        ta, tu = (_t(np.full((4, SLOTS), -1, np.int32)) for _ in range(2))
        pk = rng.integers(0, 256, (B, 23), dtype=np.uint8)
        for t in range(3):
            args = (ids, pk, np.full(B, 15, np.int32), rooms, np.zeros(B, np.int32), 0, N, enc)
            got, want = _shared_tick(a, ba, ta, *args), _shared_tick(u, bu, tu, *args)
            for name, g, w in zip(NAMES, got, want):
                assert np.array_equal(g, w), (t, name)
        _same_state(a, u, np.arange(ms, dtype=np.int32), "after the refused calls")
    finally:
        a.close()
        u.close()


# ---- 7. the class, through bridge_demo --shared-encoders ------------------------------------------------------------------

def _demo(tmp_path, mode, streams, script, packets, lengths, N):
    return run_demo(tmp_path, mode, streams, script, packets, lengths, True, (f"--max-speakers={N}", "--shared-encoders"),
                    (("--speakers-out", "spk.i32"), ("--slots-out", "slots.i32")))


@pytest.mark.gpu
def test_bridge_demo_with_shared_encoders_equals_begin_end_from_python(tmp_path):
    T, n, N = 30, 13, 2
    streams, script, packets, lengths = demo_conference(41, T, n, 6, 2)     # (the first member's bitrate is the room's)
    blocking = _demo(tmp_path, 0, streams, script, packets, lengths, N)
    pipelined = _demo(tmp_path, 1, streams, script, packets, lengths, N)
    for b, p in zip(blocking, pipelined):
        assert np.array_equal(b, p)
    max_rooms = int(script[:, :, 0].max()) + 1
    a = _ctx(n + max_rooms * (1 + N))
    try:
        held = shared = 0
        for t in range(T):
            rooms = script[t, :, 0]
            labels = _labels(rooms)
            first = [int(np.flatnonzero(rooms == lab)[0]) for lab in labels]
            enc_ids = n + labels[:, None] * (1 + N) + np.arange(1 + N)[None, :]
            bits = np.repeat(script[t, first, 2] // 50, 1 + N)
            dtx = np.repeat([streams[s][1] for s in first], 1 + N)
            a.shared_begin(packets[t], lengths[t], rooms, N, labels, enc_ids, bits, dtx, script[t, :, 1], SKIP_CN,
                           np.arange(n, dtype=np.int32))
            out, out_n, _, _, _, spk, slot_of = a.shared_end()
            assert np.array_equal(out_n, blocking[1][t]) and np.array_equal(out, blocking[0][t]), f"tick {t}"
            assert np.array_equal(spk, blocking[2][t]) and np.array_equal(slot_of, blocking[3][t]), f"tick {t}: speakers and slots"
            held += int((slot_of >= 0).sum())
            shared += int(np.unique(out[out_n > 0], axis=0).shape[0] < (out_n > 0).sum())
        assert held > T and shared > T // 2, "nobody ever held a slot, or no packet was ever shared"
    finally:
        a.close()
