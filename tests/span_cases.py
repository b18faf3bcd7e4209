"""The GPU tests of the time-parallel span calls: buffers with filler rows, the hop-by-hop twins, the checks of rows, packets
and exported state, schedules placed on a call's plan.  No tests here; torch and lyra_amd are imported inside the functions."""
import numpy as np

from gpu_plumbing import FILL, _dev, _filled
from signals import EXT_ROW, _long_trace, _speech_hops

MAX_STREAMS = 96                               # the span tests' contexts
ROW = 23                                       # LYRA_HIP_MAX_PACKET_BYTES
EXT = EXT_ROW                                  # LYRA_HIP_MAX_EXT_HOP
FILL16 = 21845                                 # two FILL bytes
GEN, CNG, RX, CN = 1, 2, 4, 8                  # lossy_info (lyra_amd/csrc/lossy_plan.h)
BITS = np.array([4, 8, 12, 64, 100, 120, 180, 184], np.int32)   # 100 bits: 25 stages, the last byte carries a zero low nibble
SIZES = np.array([8, 15, 23], np.int32)


# ---- buffers ----------------------------------------------------------------------------------------------------------------
def _layout(rows_by_id, gaps, tail=2):
    """frame-major buffer, gaps[k] filler rows in front of span k (0: the span touches the one before; an int: that many in
    front of every span) and `tail` behind the last: spans, buffer"""
    first = next(iter(rows_by_id.values()))
    def filler(g):
        return np.full((g, first.shape[1] * first.dtype.itemsize), FILL, np.uint8).view(first.dtype)
    if isinstance(gaps, int):
        gaps = [gaps] * len(rows_by_id)
    spans, parts, at = [], [], 0
    for (i, v), gap in zip(rows_by_id.items(), gaps):
        parts += [filler(gap), v]
        spans.append((i, at + gap, len(v)))
        at += gap + len(v)
    return spans, np.ascontiguousarray(np.concatenate(parts + [filler(tail)]))


def _by_frame(spans, by_id, F, dtype=np.int32):
    """{id: [n]} -> [F], FILL bytes outside the spans"""
    out = np.full(F * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype).copy()
    for (i, first, n) in spans:
        out[first:first + n] = by_id[i]
    return out


def _rows_of(pk184, pb):
    """what the receiver holds: the first pb bytes of each packet, FILL behind them and in the rows of lost packets"""
    rows = np.full((len(pb), ROW), FILL, np.uint8)
    for h, n in enumerate(pb):
        rows[h, :n] = pk184[h, :n]
    return rows


def _padded(x, fill):
    """[n][hop] -> [n][960], `fill` behind the samples"""
    out = np.full((len(x), EXT), fill, np.int16)
    out[:, :x.shape[1]] = x
    return out


def _packets(enc, golden_dir, n, num_bits, seed):
    """n packets of golden speech (the encoder side of `enc`, stream 0, time-parallel on lanes 1..40)"""
    if n == 0:
        return np.zeros((0, (num_bits + 7) // 8), np.uint8)
    enc.reset([0])
    return enc.encode_spans([(0, 0, n)], _speech_hops(golden_dir, n, seed), num_bits, np.arange(1, 41, dtype=np.int32))


def _dirty_lane(contexts, lane, golden_dir):
    """estimator, comfort-noise and resampler slots of a lane that are not the reset state; its decoder stages stay reset"""
    x = _speech_hops(golden_dir, 3, 900)
    for c in contexts:
        for h in x:
            c.noise_receive(h[None], [lane], side="decoder")
        c.comfort_noise(stream_ids=[lane])
        c.resample(x[:1], 16000, 48000, [lane], side="decoder")


def _in_pos_offsets(ctx, scratch_id):
    """Byte offsets of RS_IN_POS of the encoder's and the decoder's resampler slot in a blob, found on the device: resampling
    zeros into a fresh stream's slot leaves its history as it was and moves the phase word alone."""
    offs = []
    for side, n_in, to in (("encoder", 3, (48000, 16000)), ("decoder", 2, (16000, 8000))):
        before = ctx.export_streams([scratch_id])[0]
        ctx.resample(np.zeros((1, n_in), np.int16), to[0], to[1], [scratch_id], side=side)
        after = ctx.export_streams([scratch_id])[0]
        at = np.flatnonzero(before != after)
        assert at.size == 1 and after[at[0]] == n_in and before[at[0]] == 0, \
            f"{side} resampler of stream {scratch_id}: resampling {n_in} zeros changed blob bytes {at.tolist()}, not the phase word alone"
        offs.append(int(at[0]))
    return offs


# ---- the checks -------------------------------------------------------------------------------------------------------------
def _check_rows(where, got, spans, want_by_id, written=None, skipped=FILL):
    """rows of the spans equal the twin's (written[id]: only those rows; every byte of the others is `skipped`, by default
    still the filler); every row outside the spans still holds the filler"""
    covered = np.zeros(len(got), bool)
    for (i, first, n) in spans:
        covered[first:first + n] = True
        if not n:
            continue
        rows, want = got[first:first + n].reshape(n, -1), np.asarray(want_by_id[i]).reshape(n, -1)
        on = np.ones(n, bool) if written is None else np.asarray(written[i], bool)
        diff = np.flatnonzero(on)[(rows[on] != want[on]).any(axis=1)]
        assert len(diff) == 0, f"{where}: stream {i} differs at written hops {diff[:8].tolist()} ({len(diff)} of {n})"
        assert (rows[~on].view(np.uint8) == skipped).all(), f"{where}: stream {i}: rows of noise hops do not hold {skipped}"
    assert (got[~covered].view(np.uint8) == FILL).all(), f"{where}: rows outside every span were written"


def _check_packets(where, got_pk, got_nb, spans, want_pk, want_nb):
    F = len(got_pk)
    _check_rows(where + " packet_bytes", got_nb.reshape(F, 1), spans, want_nb)
    _check_rows(where + " packet rows", got_pk, spans, want_pk)   # (the twin's rows: FILL behind every packet, FILL in noise rows)
    nb = _by_frame(spans, want_nb, F)
    for (i, first, n) in spans:
        for f in range(first, first + n):
            assert (got_pk[f, nb[f]:] == FILL).all(), f"{where}: stream {i}: bytes behind the packet of frame {f} were written"


def _check_ext(where, got, spans, want_by_id, rate_of):
    """[F][960]: the rows of span s equal the twin's up to rate / 50 samples; everything else still holds the filler"""
    untouched = np.ones(got.shape, bool)
    for (i, first, n) in spans:
        hop = rate_of[i] // 50
        untouched[first:first + n, :hop] = False
        diff = np.flatnonzero((got[first:first + n, :hop] != want_by_id[i]).any(axis=1)) if n else np.zeros(0, int)
        assert len(diff) == 0, f"{where}: stream {i} ({rate_of[i]} Hz) differs at hops {diff[:8].tolist()} ({len(diff)} of {n})"
    assert (got[untouched] == FILL16).all(), f"{where}: samples behind a row's rate / 50, or rows outside every span, were written"


def _check_state(where, ctx, twin, span_ids, lanes):
    """span streams: the blob of the stream that ran hop by hop on the twin.  Lanes: the blob of the same id on the twin, where
    no codec stage ever ran on it (a blob's header names its source id, so the SAME id is the one to compare with; what a test
    dirtied in a lane's other slots, it dirtied on both contexts)."""
    got, want = ctx.export_streams(span_ids), twin.export_streams(span_ids)
    bad = [int(span_ids[k]) for k in range(len(span_ids)) if not np.array_equal(got[k], want[k])]
    assert not bad, f"{where}: the blobs of span streams {bad} differ from the twin's"
    if not len(lanes):
        return
    got, want = ctx.export_streams(lanes), twin.export_streams(lanes)
    bad = [int(lanes[k]) for k in range(len(lanes)) if not np.array_equal(got[k], want[k])]
    assert not bad, f"{where}: lanes {bad} differ from the twin's untouched lanes: stages not in the reset state, or another slot touched"


# ---- the twins: hop by hop on a second context ------------------------------------------------------------------------------
def _stacked(rows_by_id, width, dtype):
    return {i: np.stack(v) if v else np.zeros((0, width), dtype) for i, v in rows_by_id.items()}


def _hops_of(rows_by_id):
    """per hop the ids that still have a row, in the dict's order"""
    for h in range(max((len(v) for v in rows_by_id.values()), default=0)):
        yield h, [i for i, v in rows_by_id.items() if h < len(v)]


def _sequential(ctx, rows_by_id, num_bits, encode):
    """hop by hop on `ctx`, one blocking call per hop over the streams that still have rows: {id: [n][.]} -> {id: [n][.]}"""
    out = {i: [] for i in rows_by_id}
    for h, ids in _hops_of(rows_by_id):
        batch = np.stack([rows_by_id[i][h] for i in ids])
        res = ctx.encode(batch, num_bits, ids) if encode else ctx.decode(batch, num_bits, ids)
        for k, i in enumerate(ids):
            out[i].append(res[k])
    return _stacked(out, (num_bits + 7) // 8 if encode else 320, np.uint8 if encode else np.int16)


def _twin_encode_ext(twin, ext_by_id, rate, num_bits, dtx=False):
    """resample + encode hop by hop: {id: [n][rate / 50]} -> packets {id: [n][bytes]}, 16 kHz hops {id: [n][320]}; dtx:
    through encode_dtx, with the sizes {id: [n]} between the two"""
    pk, nb, p16 = ({i: [] for i in ext_by_id} for _ in range(3))
    for h, ids in _hops_of(ext_by_id):
        x = np.stack([ext_by_id[i][h] for i in ids])
        x16 = twin.resample(x, rate, 16000, ids, side="encoder") if rate != 16000 else x
        res, size = twin.encode_dtx(x16, num_bits, ids) if dtx else (twin.encode(x16, num_bits, ids), [num_bits // 8] * len(ids))
        for k, i in enumerate(ids):
            pk[i].append(res[k]); nb[i].append(size[k]); p16[i].append(x16[k])
    out = (_stacked(pk, (num_bits + 7) // 8, np.uint8), {i: np.array(v, np.int32) for i, v in nb.items()}, _stacked(p16, 320, np.int16))
    return out if dtx else (out[0], out[2])


def _twin_encode_rows(twin, ext_by_id, bits_by_id, rates, dtx=False, aux=None):
    """hop by hop with a bit count per row: {id: [n][rate / 50]}, {id: [n] bit counts} -> rows {id: [n][23], FILL behind each
    packet}, sizes {id: [n]}.  rates: one rate (encode_mixed_dev) or {id: rate} (encode_rates_dev on rows padded to 960 samples);
    aux (a context that runs nothing else): its resample(side="encoder") gives the 16 kHz hops {id: [n][320]} as a third result"""
    import torch
    dev = _dev()
    per_row = isinstance(rates, dict)
    rate_of = rates if per_row else {i: rates for i in ext_by_id}
    pk, nb, p16 = ({i: [] for i in ext_by_id} for _ in range(3))
    for h, ids in _hops_of(ext_by_id):
        B = len(ids)
        d_ids = torch.tensor(ids, dtype=torch.int32, device=dev)
        d_bits = torch.tensor([int(bits_by_id[i][h]) for i in ids], dtype=torch.int32, device=dev)
        d_pk, d_nb = _filled(dev, B, ROW, np.uint8), _filled(dev, B, 1, np.int32).view(-1)
        if per_row:
            d_x = torch.from_numpy(np.concatenate([_padded(ext_by_id[i][h][None], 0) for i in ids])).to(dev)
            d_rates = torch.tensor([rate_of[i] for i in ids], dtype=torch.int32, device=dev)
            twin.encode_rates_dev(d_ids, d_x, d_rates, d_bits, d_pk, d_nb, dtx=dtx)
        else:
            d_x = torch.from_numpy(np.stack([ext_by_id[i][h] for i in ids])).to(dev)
            twin.encode_mixed_dev(d_ids, d_x, rates, d_bits, d_pk, d_nb, dtx=dtx)
        twin.synchronize()
        rows, sizes = d_pk.cpu().numpy(), d_nb.cpu().numpy()
        for k, i in enumerate(ids):
            pk[i].append(rows[k]); nb[i].append(sizes[k])
            x = ext_by_id[i][h]
            if aux is not None:
                p16[i].append(x if rate_of[i] == 16000 else aux.resample(x[None], rate_of[i], 16000, [i], side="encoder")[0])
    assert twin.encode_mixed_errors() == 0 and twin.rates_errors() == 0, \
        f"the twin's encode calls flagged {twin.encode_mixed_errors()} bit counts and {twin.rates_errors()} rates"
    out = (_stacked(pk, ROW, np.uint8), {i: np.array(v, np.int32) for i, v in nb.items()})
    return out + (_stacked(p16, 320, np.int16),) if per_row else out


def _twin_decode_ext(twin, pk_by_id, rate, num_bits):
    """decode + resample hop by hop: packets -> external-rate PCM {id: [n][rate / 50]}, 16 kHz PCM {id: [n][320]}"""
    ext, p16 = {i: [] for i in pk_by_id}, {i: [] for i in pk_by_id}
    for h, ids in _hops_of(pk_by_id):
        x16 = twin.decode(np.stack([pk_by_id[i][h] for i in ids]), num_bits, ids)
        res = twin.resample(x16, 16000, rate, ids, side="decoder")
        for k, i in enumerate(ids):
            ext[i].append(res[k]); p16[i].append(x16[k])
    return _stacked(ext, rate // 50, np.int16), _stacked(p16, 320, np.int16)


def _twin_decode_plain(twin, pk_by_id, num_bits, rate_of):
    """hop by hop through decode + resample(side="decoder") at each stream's rate: {id: pcm16 [n][320]}, {id: pcm_ext
    [n][rate / 50]}"""
    p16, ext = ({i: [] for i in pk_by_id} for _ in range(2))
    for h, ids in _hops_of(pk_by_id):
        x16 = twin.decode(np.stack([pk_by_id[i][h] for i in ids]), num_bits, ids)
        for k, i in enumerate(ids):
            p16[i].append(x16[k])
            ext[i].append(x16[k] if rate_of[i] == 16000 else twin.resample(x16[k][None], 16000, rate_of[i], [i], side="decoder")[0])
    return _stacked(p16, 320, np.int16), {i: np.stack(v) if v else np.zeros((0, rate_of[i] // 50), np.int16) for i, v in ext.items()}


def _lossy_ticks(twin, pk_by_id, pb_by_id, hop_of, ext_width, call, watch=None):
    """The loop of the three lossy twins: per hop the rows of the streams that still have one, packet_bytes from pb_by_id, outputs
    on zeroed buffers (flags on -7), `call(ids, d_ids, d_pk, d_pb, d_16, d_ext, d_n, d_cn)` for the tick itself.  d_ext is
    [B][ext_width], or None for ext_width 0 (then the 16 kHz hop stands for it); a row of it is kept up to hop_of(id) samples.
    -> [{id: pcm16 [n][320]}, {id: pcm_ext [n][hop]}, {id: is_noise [n]}, {id: is_cn [n]}] and, for stream `watch`, the
    decoder-side noise estimate after every tick [n][160]"""
    import torch
    dev = _dev()
    out = [{i: [] for i in pk_by_id} for _ in range(4)]
    est = []
    for h, ids in _hops_of(pk_by_id):
        B = len(ids)
        d_ids = torch.tensor(ids, dtype=torch.int32, device=dev)
        d_pk = torch.from_numpy(np.stack([pk_by_id[i][h] for i in ids])).to(dev)
        d_pb = torch.tensor([int(pb_by_id[i][h]) for i in ids], dtype=torch.int32, device=dev)
        d_16 = torch.zeros((B, 320), dtype=torch.int16, device=dev)
        d_ext = torch.zeros((B, ext_width), dtype=torch.int16, device=dev) if ext_width else None
        d_n, d_cn = (torch.full((B,), -7, dtype=torch.int32, device=dev) for _ in range(2))
        call(ids, d_ids, d_pk, d_pb, d_16, d_ext, d_n, d_cn)
        twin.synchronize()
        res = (d_16.cpu().numpy(), d_ext.cpu().numpy() if d_ext is not None else d_16.cpu().numpy(), d_n.cpu().numpy(),
               d_cn.cpu().numpy())
        for k, i in enumerate(ids):
            for j, (o, r) in enumerate(zip(out, res)):
                o[i].append(r[k][:hop_of(i)] if j == 1 else r[k])
        if watch in ids:
            est.append(twin.noise_estimate([watch])[0].copy())
    assert twin.decode_lossy_errors() == 0, f"the twin's lossy decode calls flagged {twin.decode_lossy_errors()} rows"
    dt = (np.int16, np.int16, np.int32, np.int32)
    shape = lambda i: ((0, 320), (0, hop_of(i)), (0,), (0,))
    return [{i: np.stack(v) if v else np.zeros(shape(i)[k], dt[k]) for i, v in o.items()} for k, o in enumerate(out)], \
        np.array(est, np.float32)


def _twin_decode_lossy(twin, pk_by_id, rx_by_id, rate, num_bits, watch=None):
    """hop by hop through decode_lossy_dev: {id: pcm16 [n][320]}, {id: pcm_ext [n][rate / 50]}, {id: is_noise [n]}, {id: is_cn
    [n]} and, for stream `watch`, the decoder-side noise estimate after every tick [n][160]"""
    nbytes = (num_bits + 7) // 8
    def call(ids, d_ids, d_pk, d_pb, d_16, d_ext, d_n, d_cn):
        twin.decode_lossy_dev(d_ids, d_pk, d_pb, num_bits, rate, d_16, d_ext, d_n, d_cn)
    out, est = _lossy_ticks(twin, pk_by_id, {i: np.where(rx_by_id[i], nbytes, 0) for i in pk_by_id}, lambda i: rate // 50,
                            rate // 50 if rate != 16000 else 0, call, watch)
    return (*out, est)


def _twin_decode_mixed(twin, pk_by_id, pb_by_id, rate):
    """hop by hop through decode_lossy_mixed_dev: {id: pcm16 [n][320]}, {id: pcm_ext [n][rate / 50]}, {id: is_noise [n]},
    {id: is_cn [n]}"""
    def call(ids, d_ids, d_pk, d_pb, d_16, d_ext, d_n, d_cn):
        twin.decode_lossy_mixed_dev(d_ids, d_pk, d_pb, rate, d_16, d_ext, d_n, d_cn)
    return _lossy_ticks(twin, pk_by_id, pb_by_id, lambda i: rate // 50, rate // 50 if rate != 16000 else 0, call)[0]


def _twin_decode_rates(twin, pk_by_id, pb_by_id, rate_of):
    """hop by hop through decode_lossy_rates_dev: {id: pcm16 [n][320]}, {id: pcm_ext [n][rate / 50]}, {id: is_noise [n]},
    {id: is_cn [n]}"""
    import torch
    def call(ids, d_ids, d_pk, d_pb, d_16, d_ext, d_n, d_cn):
        d_rates = torch.tensor([rate_of[i] for i in ids], dtype=torch.int32, device=_dev())
        twin.decode_lossy_rates_dev(d_ids, d_pk, d_pb, d_rates, d_16, d_ext, d_n, d_cn)
    out = _lossy_ticks(twin, pk_by_id, pb_by_id, lambda i: rate_of[i] // 50, EXT, call)[0]
    assert twin.rates_errors() == 0, f"the twin's decode_lossy_rates_dev calls flagged {twin.rates_errors()} rates"
    return out


# ---- schedules placed on a call's plan --------------------------------------------------------------------------------------
def _other(value, choices):
    """the choice behind `value`, cyclically: a different one"""
    return choices[(int(np.flatnonzero(choices == value)[0]) + 1) % len(choices)]


def _encode_plan(spans, active_by_id, lanes, max_streams=MAX_STREAMS):
    """the encoder's plan on the frames that reach it (active_by_id: {id: [n] bool}, all True without DTX) and the map of its
    frame index to buffer frames"""
    import lyra_amd.codec as codec
    compact, frame_map, region = [], {}, 0
    for (i, first, n) in spans:
        at = np.flatnonzero(active_by_id[i])
        compact.append((i, region, len(at)))
        frame_map.update({region + c: first + int(f) for c, f in enumerate(at)})
        region += n
    chunks, n_steps = codec.spans_plan("encoder", compact, lanes, max_streams)
    return chunks, n_steps, frame_map, compact


def _draw_sizes(rng, rx):
    return np.where(rx, rng.choice(SIZES, len(rx)), 0).astype(np.int32)


def _size_changes(plan, g0, n_gen):
    """compacted indices g0 <= g < g0 + n_gen of the span's ticks fed from a packet whose size differs from the last such
    tick's in front of them"""
    gb, last, out = plan["gen_bytes"], 0, set()
    for g in range(g0, g0 + n_gen):
        if gb[g]:
            if last and gb[g] != last:
                out.add(g)
            last = int(gb[g])
    return out


def _assert_size_changes(where, plan, k_long, first, W):
    """on the long span: a size change on a lane chunk's first tick, one inside a warm-up, and one on the first received tick
    behind a comfort-noise stretch"""
    counts = plan["counts"]
    g0, n_gen = int(counts["n_gen"][:k_long].sum()), int(counts["n_gen"][k_long])
    changes = _size_changes(plan, g0, n_gen)
    lane_chunks = [c for c in plan["chunks"] if c["span"] == k_long and c["n_warmup"] > 0]
    assert any(int(c["first_frame"]) in changes for c in lane_chunks), (where, "no size change on a chunk's first tick")
    assert any(g in changes for c in lane_chunks for g in range(int(c["first_frame"]) - W, int(c["first_frame"]))), \
        (where, "no size change inside a warm-up")
    info = plan["info"][:350]   # (the long span is the call's first)
    frame_of = plan["gen_frames"] - first
    behind_cng = {h for h in range(1, 350) if info[h] & RX and info[h - 1] & CNG and not info[h - 1] & RX}
    assert any(int(frame_of[g]) in behind_cng for g in changes), (where, "no size change behind a comfort-noise stretch")


def _decode_schedule(where, rng, spans, rx, lanes, F, W, max_streams=MAX_STREAMS):
    """rx[7]: the long loss trace, placed on the call's plan; then a size per received frame {id: [n]}, drawn from SIZES and
    adjusted on the plan: a switch on the first packet behind a comfort-noise stretch and on a lane chunk's first tick"""
    import lyra_amd.codec as codec
    first = spans[0][1]
    def plan_of(rx7):   # (the plan depends on the receive pattern alone)
        pb = _by_frame(spans, {i: np.where(rx7 if i == 7 else rx[i], ROW, 0) for (i, _, _) in spans}, F)
        return codec.spans_lossy_plan(spans, pb, ROW, [0] * len(spans), lanes, max_streams), first
    rx[7] = _long_trace(plan_of)
    pb = {i: _draw_sizes(rng, rx[i]) for (i, _, _) in spans}
    plan, _ = plan_of(rx[7])
    frame_of = plan["gen_frames"] - first
    info = plan["info"][:350]
    def switch_at(h):
        before = pb[7][:h][pb[7][:h] > 0]
        pb[7][h] = _other(before[-1], SIZES)
    chunk_first = [int(frame_of[int(c["first_frame"])]) for c in plan["chunks"] if c["span"] == 0 and c["n_warmup"] > 0]
    switch_at(next(h for h in range(1, 350) if rx[7][h] and info[h - 1] & CNG and not rx[7][h - 1]))
    switch_at(next(h for h in chunk_first if rx[7][h]))
    mixed_plan = codec.spans_lossy_plan_mixed(spans, _by_frame(spans, pb, F), [0] * len(spans), lanes, max_streams)
    _assert_size_changes(where, mixed_plan, 0, first, W)
    return pb
