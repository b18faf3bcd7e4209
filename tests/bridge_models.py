"""The conference bridge as the tests hold the device to it (include/lyra_hip_bridge.h): a numpy restatement of the membership
plan and of the mix-minus formula, the synthetic rows and index of the kernel test, and BridgeModel -- B reference decoders, the
mix, B reference encoders.  No tests here; torch, lyra_amd and the oracle are imported inside the functions."""
import numpy as np

from receiver_models import ROW, SEED, Tally, cn_flags

MAX_ROOM = 32767   # LYRA_HIP_BRIDGE_MAX_ROOM
SKIP_CN = 1        # LYRA_HIP_BRIDGE_SKIP_COMFORT_NOISE
HOP16 = 320


def np_bridge_plan(rooms):
    """rooms [B] labels (< 0: in no room) -> (order [n_members], room_start [n_rooms + 1]), or None where the planner refuses:
    rooms in ascending label order, rows ascending inside a room."""
    rooms = np.asarray(rooms, np.int64).reshape(-1)
    rows = np.flatnonzero(rooms >= 0)
    order = rows[np.argsort(rooms[rows], kind="stable")]
    labels, counts = np.unique(rooms[rows], return_counts=True)
    if counts.size and counts.max() > MAX_ROOM:
        return None
    return order.astype(np.int32), np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def np_bridge_mix(pcm16, order, room_start, muted=None, is_cn=None):
    """The formula, row by row: y_b = clamp(S_r - (source_b ? x_b : 0)) over the rooms of a VALID index (every entry in
    [0, B), no row twice); rows no room names hear zeros.  muted / is_cn [B] or None: rows that are no source."""
    x = np.asarray(pcm16, np.int16).astype(np.int64)
    B = x.shape[0]
    source = np.ones(B, bool)
    if muted is not None:
        source &= np.asarray(muted) == 0
    if is_cn is not None:
        source &= np.asarray(is_cn) == 0
    y = np.zeros_like(x)
    for r in range(len(room_start) - 1):
        members = np.asarray(order[room_start[r]:room_start[r + 1]], np.int64)
        total = x[members[source[members]]].sum(axis=0)
        for b in members:
            y[b] = total - (x[b] if source[b] else 0)
    return np.clip(y, -32768, 32767).astype(np.int16)


def bridge_kernel_case(seed=7):
    """The shape of the kernel test, B = 330 (the rooms alone take 313 rows): (pcm16 [B][320], rooms [B], muted [B], is_cn [B]).
    Rows of +-32767, -32768, ramps and random samples; rooms of 1, 2, 3, 8, 9, 16, 17 and 257 members, one of them (the 17)
    scattered over the batch; muted rows, one comfort-noise row, a room whose every member is muted; the rest in no room."""
    rng = np.random.default_rng(seed)
    B = 330
    x = rng.integers(-32768, 32768, size=(B, HOP16)).astype(np.int16)
    x[0::7] = 32767
    x[1::7] = -32768
    x[2::7] = -32767
    x[3::7] = (np.arange(HOP16) * 200 - 32000).astype(np.int16)
    sizes = {0: 1, 1: 2, 2: 3, 3: 8, 4: 9, 5: 16, 6: 257}
    rooms = np.full(B, -1, np.int32)
    free = rng.permutation(B)
    scattered, free = free[:17], free[17:]
    rooms[scattered] = 40                      # a label that is no index: non-contiguous labels, rows all over the batch
    free = np.sort(free)
    at = 0
    for label, n in sizes.items():
        rooms[free[at:at + n]] = label
        at += n
    assert at < free.size                      # some rows stay in no room
    muted = (rng.random(B) < 0.1).astype(np.int32)
    muted[rooms == 2] = 1                      # a room whose every member is muted
    muted[rooms == 0] = 0
    is_cn = np.zeros(B, np.int32)
    is_cn[np.flatnonzero((rooms == 3) & (muted == 0))[0]] = 1
    # saturation on both sides is certain: the 257-room holds rows of +32767 and rows of -32768 ...
    big = np.flatnonzero(rooms == 6)
    x[big[:100]] = 32767                       # ... and here its sum is far above the range at every sample,
    muted[big[:100]] = 0
    nine = np.flatnonzero(rooms == 4)
    x[nine] = -32768                           # and the 9-room's far below
    muted[nine] = 0
    return x, rooms, muted, is_cn


class BridgeModel:
    """B RefLyraDecoder(16000, cng_seed = SEED ^ id), the mix, B RefLyraEncoder(16000, bits[b], dtx[b]) from
    oracle/lyra_codec_model.py.  tick() runs the model's own bridge and returns (hops [B][320], reach [B][320] bool: where
    comfort noise went in, mix [B][320], packets [B][23], sizes [B], is_cn [B]); encode_of() runs the model's encoders over a mix
    that was made elsewhere (the device's own), the pattern LossyModel uses behind the resampler."""

    def __init__(self, oracle, ids, rooms, muted, bits, dtx, flags=0):
        from oracle import lyra_codec_model as M
        self.ids = [int(i) for i in ids]
        self.decs = [M.RefLyraDecoder(oracle, 16000, cng_seed=SEED ^ i) for i in self.ids]
        self.encs = [M.RefLyraEncoder(oracle, 16000, int(b), bool(d)) for b, d in zip(bits, dtx)]
        self.own_encs = [M.RefLyraEncoder(oracle, 16000, int(b), bool(d)) for b, d in zip(bits, dtx)]
        self.rooms, self.muted, self.flags = np.asarray(rooms, np.int32), np.asarray(muted, np.int32), flags
        self.tally = Tally()

    @staticmethod
    def _encode(encs, mix):
        rows = np.zeros((len(encs), ROW), np.uint8)
        sizes = np.zeros(len(encs), np.int32)
        for b, enc in enumerate(encs):
            p = enc.Encode(mix[b])
            rows[b, :p.size], sizes[b] = p, p.size
        return rows, sizes

    def tick(self, packets, sizes):
        B = len(self.decs)
        hops, reach, is_cn = np.zeros((B, HOP16), np.int16), np.zeros((B, HOP16), bool), np.zeros(B, np.int32)
        for b, dec in enumerate(self.decs):
            if sizes[b]:
                dec.SetEncodedPacket(packets[b, :sizes[b]])
            dec.DecodeSamples(HOP16)
            hops[b], reach[b], is_cn[b] = dec.last_internal, cn_flags(dec), int(dec.is_comfort_noise())
        order, start = np_bridge_plan(self.rooms)
        mix = np_bridge_mix(hops, order, start, self.muted, is_cn if self.flags & SKIP_CN else None)
        rows, out_sizes = self._encode(self.own_encs, mix)
        return hops, reach, mix, rows, out_sizes, is_cn

    def encode_of(self, mix):
        return self._encode(self.encs, mix)
