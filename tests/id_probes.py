"""Which stream ids to test so that the whole documented id range of a context is covered, from the regions' slot sizes alone.

The six stage kernels address a stream's state as a 32-bit byte offset `id * slot bytes` into their region (lyra_dev.h goff,
resblocks.h TileCtx::soff), so a context holds at most cap = floor(2^32 / widest slot) streams (api.hip create_impl).  The
offsets worth a test of their own are the first one with bit 31 set in every region that reaches it (and the last one
without), the last two slots under the cap, the edges earlier tests stopped at, and a few ids drawn in between.

A plain helper module for tests/test_id_probes_cpu.py and tests/test_gpu_id_range.py; pure functions of their arguments:
nothing of the layout is a literal here."""
import numpy as np

N_STAGE_REGIONS = 6          # R_E0 .. R_D2 of state_layout.h: the regions the stage kernels address with 32-bit offsets
OLD_EDGE = 32768             # the largest context an earlier test creates (test_config5_32768_streams_one_gpu)
TILE = 8                     # streams per workgroup of the widest stage tiles


def cap_of(all_region_bytes):
    """streams per context: every region's last slot must end at or before 2^32 (create_impl)"""
    return (1 << 32) // max(int(b) for b in all_region_bytes)


def crossings(stage_region_bytes, cap):
    """region index -> k_r = ceil(2^31 / bytes_r), the first id whose offset into the region has bit 31 set, for the stage
    regions where that id lies under the cap"""
    out = {}
    for r, b in enumerate(stage_region_bytes):
        k = -(-(1 << 31) // int(b))
        if k <= cap - 1:
            out[r] = k
    return out


def witnesses_of(probes, cap):
    """the neighbours p - 1 and p + 1 of every probe that lie in 0..cap-1 and are no probes themselves, ascending"""
    ps = set(int(p) for p in probes)
    return sorted({q for p in ps for q in (p - 1, p + 1) if 0 <= q < cap and q not in ps})


def _call_order(probes, cap, rng):
    """the probes dealt over tiles of TILE consecutive rows so that every tile holds ids of the lower and of the upper half of
    the arena, in seeded random order inside each tile"""
    low = [p for p in probes if p < cap // 2]
    high = [p for p in probes if p >= cap // 2]
    n_tiles = -(-len(probes) // TILE)
    assert len(low) >= n_tiles and len(high) >= n_tiles, "too few ids at one end to mix every tile"
    low = [low[i] for i in rng.permutation(len(low))]
    high = [high[i] for i in rng.permutation(len(high))]
    sizes = [min(TILE, len(probes) - TILE * t) for t in range(n_tiles)]
    tiles = [[low.pop(), high.pop()] for _ in range(n_tiles)]
    rest = low + high
    rest = [rest[i] for i in rng.permutation(len(rest))]
    for t in range(n_tiles):
        while len(tiles[t]) < sizes[t]:
            tiles[t].append(rest.pop())
    assert not rest, f"{len(rest)} probe ids fit in no tile"
    return [tiles[t][i] for t in range(n_tiles) for i in rng.permutation(len(tiles[t]))]


def probe_plan(stage_region_bytes, cap, seed=289262):
    """-> dict: `cross` {region: k_r}; `probes` ascending; `order` the probes in call order (every TILE rows mix both ends of
    the arena; the count is no multiple of TILE, so the last tile is ragged); `witnesses` ids next to the probes that no codec
    call may ever be given."""
    stage_region_bytes = [int(b) for b in stage_region_bytes]
    assert len(stage_region_bytes) == N_STAGE_REGIONS and cap > 2 * OLD_EDGE, (len(stage_region_bytes), "stage regions; cap", cap)
    rng = np.random.default_rng(seed)
    cross = crossings(stage_region_bytes, cap)
    ids = {0, 1, OLD_EDGE - 1, OLD_EDGE, cap - 2, cap - 1}
    for k in cross.values():
        ids |= {k - 1, k}

    def draw(lo, hi, n):                       # n new ids of lo..hi-1
        while n:
            v = int(rng.integers(lo, hi))
            if v not in ids:
                ids.add(v)
                n -= 1

    draw(cap // 2, cap, 8)                     # the upper half
    draw(OLD_EDGE + 1, cap // 2, 3)            # past the old edge, below it: offsets between 2^29 and 2^31
    while len(ids) % TILE < 2:                 # a ragged last tile, of at least two rows so that it can mix as well
        draw(OLD_EDGE + 1, cap // 2, 1)
    probes = sorted(ids)
    return {"cross": cross, "probes": probes, "order": _call_order(probes, cap, rng), "witnesses": witnesses_of(probes, cap)}
