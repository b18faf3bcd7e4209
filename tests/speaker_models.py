"""The loudest-N mix of the conference bridge as the tests hold the device to it (include/lyra_hip_speakers.h): a restatement of
the levels, the selection and the mix in numpy / Python ints, and the synthetic rows and index of the kernel test.  No tests
here."""
import numpy as np

from bridge_models import HOP16, bridge_kernel_case, np_bridge_mix, np_bridge_plan

SPEAKERS_MAX = 8   # LYRA_HIP_SPEAKERS_MAX
SKIP_CN = 1        # LYRA_HIP_SPEAKERS_SKIP_COMFORT_NOISE


def np_levels(pcm16):
    """level_b = sum_k x_b[k]^2, exact, int64 [B]"""
    x = np.asarray(pcm16, np.int16).astype(np.int64)
    return (x * x).sum(axis=1)


def _source(B, muted, is_cn):
    source = np.ones(B, bool)
    if muted is not None:
        source &= np.asarray(muted) == 0
    if is_cn is not None:
        source &= np.asarray(is_cn) == 0
    return source


def np_select(levels, order, room_start, source, max_speakers):
    """-> (speakers: one list of row numbers per room, loudest first; is_speaker int32 [B]) over a VALID index.  A candidate is
    a member that is a source with level > 0; the max_speakers candidates with the largest level speak, the earlier position
    in `order` winning among equal levels.  Python ints throughout."""
    assert 1 <= max_speakers <= SPEAKERS_MAX
    is_speaker = np.zeros(len(levels), np.int32)
    speakers = []
    for r in range(len(room_start) - 1):
        members = [int(b) for b in order[room_start[r]:room_start[r + 1]]]
        cands = [(-int(levels[b]), pos, b) for pos, b in enumerate(members) if source[b] and int(levels[b]) > 0]
        chosen = [b for _, _, b in sorted(cands)[:max_speakers]]
        speakers.append(chosen)
        is_speaker[chosen] = 1
    return speakers, is_speaker


def np_speakers_mix(pcm16, order, room_start, max_speakers, muted=None, is_cn=None):
    """-> (mix int16 [B][320], levels int64 [B], is_speaker int32 [B]): y_b = clamp(S_r - (speaker_b ? x_b : 0)) with S_r the
    sum of the speakers of b's room; rows no room names hear zeros."""
    x = np.asarray(pcm16, np.int16).astype(np.int64)
    levels = np_levels(pcm16)
    speakers, is_speaker = np_select(levels, order, room_start, _source(x.shape[0], muted, is_cn), max_speakers)
    y = np.zeros_like(x)
    for r, chosen in enumerate(speakers):
        total = x[chosen].sum(axis=0) if chosen else np.zeros(HOP16, np.int64)
        for b in order[room_start[r]:room_start[r + 1]]:
            y[b] = total - (x[b] if is_speaker[b] else 0)
    return np.clip(y, -32768, 32767).astype(np.int16), levels, is_speaker


def tie_decided(levels, order, room_start, source, max_speakers):
    """rooms in which the last speaker and the first candidate left out have the same level: the position rule decided"""
    rooms = []
    for r in range(len(room_start) - 1):
        members = [int(b) for b in order[room_start[r]:room_start[r + 1]]]
        lv = sorted((int(levels[b]) for b in members if source[b] and int(levels[b]) > 0), reverse=True)
        if len(lv) > max_speakers and lv[max_speakers - 1] == lv[max_speakers]:
            rooms.append(r)
    return rooms


def speakers_kernel_case(seed=7):
    """bridge_kernel_case() (B = 330; rooms of 1, 2, 3, 8, 9, 16, 17 scattered, and 257) with the rows at which the selection
    can go wrong -> (pcm16, rooms, muted, is_cn, order, room_start); `order` is the planner's with the positions inside the
    16-room, the 257-room and the scattered room permuted.
      16-room   five identical rows of +32767 among quieter rows: equal levels, the position rule decides for N < 5, and three
                of them saturate the mix upwards; one all-zero row;
      257-room  five identical rows of 10000 among quieter rows, in the part of the kernel that parks keys in memory; all-zero rows;
      9-room    every row -32768 (the base case): level 320 * 2^30 > 2^32, and the mix saturates downwards;
      2-room    an all-zero row and one source: fewer candidates than N = 3;   3-room  every member muted (the base case);
      8-room    a comfort-noise row (the base case): fewer candidates than N = 8."""
    x, rooms, muted, is_cn = bridge_kernel_case(seed)
    rng = np.random.default_rng(seed + 1)
    order, start = np_bridge_plan(rooms)
    order = order.copy()
    labels = sorted(set(int(v) for v in rooms if v >= 0))
    seg = {lab: (int(start[i]), int(start[i + 1])) for i, lab in enumerate(labels)}
    for lab, same, value in ((5, 5, 32767), (6, 5, 10000)):
        m = np.flatnonzero(rooms == lab)
        x[m] = x[m] // 8                                    # everybody else in the room is quieter ...
        loud = rng.choice(m, same, replace=False)
        x[loud] = value                                     # ... than the identical rows
        muted[loud] = 0
        rest = np.setdiff1d(m, loud)
        x[rest[:1 if lab == 5 else 4]] = 0                  # all-zero rows: level 0, never speakers
        muted[rest[:1 if lab == 5 else 4]] = 0
    two = np.flatnonzero(rooms == 1)
    x[two[0]] = 0
    muted[two] = 0
    if not x[two[1]].any():
        x[two[1]] = 1234
    for lab in (5, 6, 40):                                  # positions decide ties: hand these rooms over permuted
        lo, hi = seg[lab]
        order[lo:hi] = order[lo:hi][rng.permutation(hi - lo)]
    # ---- what the case must show, in numpy, before anything goes to a device ----
    levels = np_levels(x)
    assert levels.max() == 320 * 2 ** 30 and (levels[rooms == 4] == 320 * 2 ** 30).all()
    source = _source(x.shape[0], muted, is_cn)
    ri = {lab: i for i, lab in enumerate(labels)}
    assert set(tie_decided(levels, order, start, source, 3)) >= {ri[5], ri[6]}, "N = 3: no tie decides in the 16- and 257-room"
    n_cand = {lab: int((source & (levels > 0) & (rooms == lab)).sum()) for lab in labels}
    assert n_cand[2] == 0 and n_cand[1] == 1 and n_cand[3] < 8 and n_cand[0] == 1
    mix3, _, spk3 = np_speakers_mix(x, order, start, 3, muted, is_cn)
    assert (mix3.astype(np.int64) == 32767).any() and (mix3 == -32768).any(), "the selected mix must saturate on both sides"
    s3 = x[np.flatnonzero(spk3 & (rooms == 5))].astype(np.int64).sum(axis=0)
    assert (s3 > 32767).all() and spk3[rooms == 4].sum() == 3, "saturation above (16-room) and below (9-room) is by clamping"
    full = np_bridge_mix(x, order, start, muted, is_cn)
    differ = (mix3 != full).any(axis=1)
    for lab in labels:
        if n_cand[lab] <= 3:
            assert not differ[rooms == lab].any(), lab      # at most N candidates: the full mix, bit for bit
    assert differ[rooms == 6].any() and differ[rooms == 40].any() and differ[rooms == 3].any()
    assert not spk3[levels == 0].any() and not spk3[rooms < 0].any()
    return x, rooms, muted, is_cn, order, start


def threshold_case(seed=11):
    """Rooms of 63, 64, 65 and 129 members (B = 330 again, 9 rows in no room): the sizes around the 64 members that the select
    kernel keeps in registers, with few distinct levels so that ties are everywhere -> (pcm16, rooms, muted, order, start)."""
    rng = np.random.default_rng(seed)
    B = 330
    rooms = np.full(B, -1, np.int32)
    rows = rng.permutation(B)
    at = 0
    for lab, n in enumerate((63, 64, 65, 129)):
        rooms[rows[at:at + n]] = lab
        at += n
    amp = rng.choice([0, 100, 200, 300], B)                  # four levels only
    x = (amp[:, None] * rng.choice([-1, 1], (B, HOP16))).astype(np.int16)
    muted = (rng.random(B) < 0.2).astype(np.int32)
    order, start = np_bridge_plan(rooms)
    order = order.copy()
    for i in range(4):
        order[start[i]:start[i + 1]] = order[start[i]:start[i + 1]][rng.permutation(start[i + 1] - start[i])]
    return x, rooms, muted, order, start
