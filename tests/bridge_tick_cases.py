"""What the GPU tests of the three kinds of conference-bridge tick share (test_gpu_bridge.py: the full mix, test_gpu_speakers.py:
the loudest-N selection, test_gpu_shared_bridge.py: the shared encoders): the holder of a tick's output buffers, the loop that
holds a tick to the calls it composes, the generator of host arrays for begin(), begin() itself, the two-deep begin() / end()
loop, and the runner of bridge_demo with its scripted conference.  What differs per kind -- which tick call, which numpy model,
which further outputs, and the counters that show a case exercised what it is about -- is a TickKind.  No tests here; torch and
lyra_amd are imported inside the functions."""
import collections
import os
import subprocess
import types

import numpy as np

from bridge_models import SKIP_CN
from gpu_plumbing import _dev, _ids, _t, make_ctx as _ctx
from receiver_models import _full_batch_mask
from row_cases import _draw_bits, _same_state

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
SIZES = np.array([8, 15, 23], np.int32)
# the outputs of a tick by the name the assertions give them: attribute, row width (None: a vector), dtype; "enc ..." have E rows
OUTPUTS = {"out sizes": ("out_n", None, "int32"), "out packets": ("out", 23, "uint8"), "pcm16": ("pcm16", 320, "int16"),
           "mix": ("mix", 320, "int16"), "is_noise": ("isn", None, "int32"), "is_comfort_noise": ("icn", None, "int32"),
           "levels": ("levels", None, "int64"), "is_speaker": ("spk", None, "int32"), "slot_of": ("slot_of", None, "int32"),
           "enc_mix": ("enc_mix", 320, "int16"), "enc packets": ("enc_pk", 23, "uint8"), "enc sizes": ("enc_n", None, "int32")}


class Bufs:
    """The outputs `names` of one tick with B rows, and room for e_max encoder rows, as zeroed device tensors"""

    def __init__(self, B, names, e_max=0):
        import torch
        self.names = names
        for name in names:
            attr, width, dt = OUTPUTS[name]
            rows = e_max if name.startswith("enc") else B
            setattr(self, attr, torch.zeros((rows,) if width is None else (rows, width), dtype=getattr(torch, dt), device=_dev()))

    def read(self, E=None):
        """-> the outputs in the order of `names`, the encoder rows' cut to E"""
        got = []
        for name in self.names:
            t = getattr(self, OUTPUTS[name][0])
            got.append((t[:E] if name.startswith("enc") else t).cpu().numpy().copy())
        return tuple(got)


class TickKind:
    """One kind of tick for compose_case.  `c` is the case: B, ms, T, N, flags, ids, rooms (before and from tick 20 on), muted,
    dtx, count (a Counter for observe / verdict), state_ids (whose stream state the twins must share at the end), and t, the
    tick that is running."""
    names = ()
    ms, seed, id_offset = 64, 100, 3

    def prepare(self, c, rng):
        """after ids, mask, rooms and mutes are drawn: the kind's own inputs"""

    def bufs(self, c):
        return Bufs(c.B, self.names)

    def draw(self, c, rng):
        """the kind's own draws of one tick, behind packets and sizes"""
        c.bits = _draw_bits(rng, c.B)

    def tick(self, c, a, bufs, pk, sz, rooms):
        raise NotImplementedError

    def composed(self, c, u, bufs, pk, sz, rooms):
        raise NotImplementedError

    def observe(self, c, t, rooms, got, want):
        """after tick t compared equal: count what the case is about"""

    def verdict(self, c):
        """after the last tick: the case exercised what it is about"""


def compose_case(kind, B, mode="xnnpack", serial=False, flags=0, T=40, N=None, **kw):
    """T ticks on one context against the calls they compose on its twin, every output of every tick and the stream state at
    the end, bit for bit"""
    ms = kind.ms
    rng = np.random.default_rng(kind.seed + B)
    ids = _ids(B, ms, B + kind.id_offset)
    mask = _full_batch_mask(T, B, rng)
    rooms = [(np.arange(B) // 4).astype(np.int32), rng.integers(-1, 4, B).astype(np.int32)]   # membership changes at tick 20
    if flags & SKIP_CN:
        mask[:, :4] = 1
        mask[6:20, 1] = 0           # row 1 of room 0 (rows 0..3) is lost for 14 ticks: comfort noise from the fifth on
    muted = (rng.random(B) < 0.15).astype(np.int32)
    muted[:4] = 0
    c = types.SimpleNamespace(B=B, ms=ms, T=T, N=N, flags=flags, ids=ids, rooms=rooms, muted=muted, state_ids=ids,
                              dtx=(np.arange(B) % 2).astype(np.int32), count=collections.Counter())
    kind.prepare(c, rng)
    a, u = _ctx(ms, mode, **kw), _ctx(ms, mode, **kw)
    try:
        if serial:
            a.set_serial(True)
            u.set_serial(True)
        ba, bu = [kind.bufs(c), kind.bufs(c)], [kind.bufs(c), kind.bufs(c)]
        for t in range(T):
            pk = rng.integers(0, 256, (B, 23), dtype=np.uint8)
            sz = (rng.choice(SIZES, B) * mask[t]).astype(np.int32)
            kind.draw(c, rng)
            r = rooms[t >= 20]
            c.t = t
            got = kind.tick(c, a, ba[t & 1], pk, sz, r)
            want = kind.composed(c, u, bu[t & 1], pk, sz, r)
            for name, g, w in zip(kind.names, got, want):
                assert np.array_equal(g, w), (f"tick {t}: {name} differs in rows",
                                              np.flatnonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[:16])
            kind.observe(c, t, r, got, want)
        assert a.decode_lossy_errors() == 0 and a.encode_mixed_errors() == 0 and a.bridge_errors() == 0
        kind.verdict(c)
        _same_state(a, u, c.state_ids, "after the last tick")
    finally:
        a.close()
        u.close()


def rooms_of_six_then_random(B, T):
    """rooms of 6 in the first half, then drawn anew at every tick"""
    return lambda t, rng, rooms: rng.integers(-1, 5, B).astype(np.int32) if t >= T // 2 else (np.arange(B) // 6).astype(np.int32)


def rooms_redrawn_every_fourth_tick(B):
    """rooms of 6, then five rooms of about 7 with rows in no room, so that N = 3 always leaves talkers out"""
    def rooms_at(t, rng, rooms):
        if t == 0:
            return (np.arange(B) // 6).astype(np.int32)
        return rng.integers(-1, 5, B).astype(np.int32) if t % 4 == 0 else rooms
    return rooms_at


def host_script(B, T, seed, rooms_at, per_listener=True):
    """T ticks of host arrays for begin(): rooms_at(t, rng, the rooms of the tick before) -> the rooms of tick t; per_listener:
    with bit counts and DTX flags per row"""
    rng = np.random.default_rng(seed)
    mask = _full_batch_mask(T, B, rng)
    ticks, rooms = [], None
    for t in range(T):
        rooms = rooms_at(t, rng, rooms)
        s = {"pk": rng.integers(0, 256, (B, 23), dtype=np.uint8), "sz": (rng.choice(SIZES, B) * mask[t]).astype(np.int32),
             "rooms": rooms, "muted": (rng.random(B) < 0.1).astype(np.int32)}
        if per_listener:
            s.update(bits=_draw_bits(rng, B), dtx=(np.arange(B) % 2).astype(np.int32))
        ticks.append(s)
    return ticks


def begin(c, s, ids, flags=0, N=None):
    """begin() of tick `s` of a host script: with encoder settings the shared-encoder tick, with N the loudest-N tick, else the
    full mix"""
    if "enc" in s:
        c.shared_begin(s["pk"], s["sz"], s["rooms"], N, s["labels"], *s["enc"], s["muted"], flags, ids)
    elif N is not None:
        c.speakers_begin(s["pk"], s["sz"], s["rooms"], s["bits"], N, s["muted"], s["dtx"], flags, ids)
    else:
        c.bridge_begin(s["pk"], s["sz"], s["rooms"], s["bits"], s["muted"], s["dtx"], flags, ids)


def begin_end_ticks(a, script, end, depth, ids, flags=0, N=None):
    """every tick of the script through begin() with `depth` ticks in flight -> what end() returned, tick by tick"""
    got = []
    for t, s in enumerate(script):
        begin(a, s, ids, flags, N)
        if t + 1 >= depth:
            got.append(end())
    while len(got) < len(script):
        got.append(end())
    return got


def demo_conference(seed, T, n, room_size, n_labels):
    """A scripted conference for bridge_demo -> (streams [(bitrate, dtx)], script [T][n][room, muted, bitrate], packets, lengths)"""
    rng = np.random.default_rng(seed)
    rates = (3200, 6000, 9200)
    streams = [(rates[s % 3], s % 2) for s in range(n)]
    script = np.zeros((T, n, 3), np.int32)
    script[:, :, 0] = (np.arange(n) // room_size)[None, :]
    script[T // 2:, :, 0] = rng.integers(-1, n_labels, n)[None, :]     # everybody moves at half time ...
    script[:, :, 1] = rng.random((T, n)) < 0.1                         # ... mutes come and go ...
    script[:, :, 2] = np.array(rates)[rng.integers(0, 3, (T, n))]      # ... and bitrates change from tick to tick
    mask = _full_batch_mask(T, n, rng)
    packets = rng.integers(0, 256, (T, n, 23), dtype=np.uint8)
    lengths = (rng.choice(SIZES, (T, n)) * mask).astype(np.int32)
    return streams, script, packets, lengths


def run_demo(tmp_path, mode, streams, script, packets, lengths, skip_cn, options=(), outs=()):
    """bridge_demo on the conference, blocking (mode 0) or pipelined (1); outs: (option, file name) of further int32 [T][n]
    outputs -> (out packets, out sizes, *outs)"""
    import lyra_amd
    demo = os.path.join(ROOT, "lyra_amd", "bridge_demo")
    assert os.path.exists(demo), "lyra_amd/bridge_demo not built (__graft_entry__.build())"
    (tmp_path / "streams.txt").write_text("".join(f"{b} {d}\n" for b, d in streams))
    for name, v in (("script.i32", script), ("pk.bin", packets), ("len.i32", lengths)):
        v.tofile(tmp_path / name)
    out, out_n = tmp_path / f"out{mode}.bin", tmp_path / f"out{mode}.i32"
    files = [tmp_path / f"{mode}{name}" for _, name in outs]
    r = subprocess.run([demo, lyra_amd.default_model_dir(), str(tmp_path / "streams.txt"), str(tmp_path / "script.i32"),
                        str(tmp_path / "pk.bin"), str(tmp_path / "len.i32"), str(out), str(out_n), str(mode), str(int(skip_cn)),
                        *options, *(f"{opt}={f}" for (opt, _), f in zip(outs, files))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (mode, r.returncode, r.stderr[-3000:])
    T, n = lengths.shape
    return (np.fromfile(out, np.uint8).reshape(T, n, 23), np.fromfile(out_n, np.int32).reshape(T, n),
            *(np.fromfile(f, np.int32).reshape(T, n) for f in files))
