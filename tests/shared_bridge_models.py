"""The loudest-N bridge with shared encoders as the tests hold the device to it (include/lyra_hip_shared_bridge.h): np_select
of speaker_models plus the slot rule, the encoder mixes and the fan-out, in numpy / Python ints; the scripted conference whose
slot events the tests count; and the planner-side label check.  No tests here."""
import numpy as np

from bridge_models import HOP16, np_bridge_plan
from speaker_models import _source, np_levels, np_select

SLOTS = 8   # LYRA_HIP_SHARED_SLOTS


def np_slot_update(old, speaker_ids, N):
    """One room's row of the slot table -> its new row (list of 8).  speaker_ids: this tick's speakers in selection order."""
    old, ids = [int(v) for v in old], [int(v) for v in speaker_ids]
    new = [-1] * SLOTS
    for j in range(N):                                   # 1. kept: a speaker's id that no lower slot holds
        if old[j] >= 0 and old[j] in ids and old[j] not in old[:j]:
            new[j] = old[j]
    waiting = [s for s in ids if s >= 0 and s not in new]
    for j in range(N):                                   # 2. the rest, in selection order, into the free slots, ascending
        if new[j] < 0 and waiting:
            new[j] = waiting.pop(0)
    return new                                           # 3. slots >= N are -1


def np_shared_mix(pcm16, ids, order, room_start, N, table, keys=None, muted=None, is_cn=None):
    """-> (enc_mix int16 [E][320], levels int64 [B], is_speaker int32 [B], slot_of int32 [B], table', speakers) over a valid
    index; E = n_rooms * (1 + N).  `table` int32 [n_table][8] is not changed, table' is the updated copy.  A room whose key is
    outside the table keeps its speakers (levels and flags are the selection's) but hears zeros and holds no slots."""
    x = np.asarray(pcm16, np.int16).astype(np.int64)
    B, n_rooms = x.shape[0], len(room_start) - 1
    levels = np_levels(pcm16)
    speakers, is_speaker = np_select(levels, order, room_start, _source(B, muted, is_cn), N)
    table = np.array(table, np.int32, copy=True)
    slot_of = np.full(B, -1, np.int32)
    y = np.zeros((n_rooms * (1 + N), HOP16), np.int64)
    for r, chosen in enumerate(speakers):
        q = r if keys is None else int(keys[r])
        if not 0 <= q < table.shape[0]:
            continue
        row = np_slot_update(table[q], [int(ids[b]) for b in chosen], N)
        table[q] = row
        total = x[chosen].sum(axis=0) if chosen else np.zeros(HOP16, np.int64)
        y[r * (1 + N)] = total
        by_id = {int(ids[b]): b for b in chosen}
        for j in range(N):
            y[r * (1 + N) + 1 + j] = total - (x[by_id[row[j]]] if row[j] >= 0 else 0)
            if row[j] >= 0:
                slot_of[by_id[row[j]]] = j
    return np.clip(y, -32768, 32767).astype(np.int16), levels, is_speaker, slot_of, table, speakers


def np_fanout(enc_packets, enc_bytes, B, order, room_start, slot_of, N, keys=None, n_table=None):
    """-> (out_packets uint8 [B][23], out_bytes int32 [B]): a member of room r receives all 23 bytes and the size of encoder
    row r * (1 + N) + 1 + slot_of if it holds a slot, of row r * (1 + N) otherwise; a row in no room, or in a room whose key is
    outside the table, 23 zero bytes and size 0."""
    out, out_n = np.zeros((B, 23), np.uint8), np.zeros(B, np.int32)
    for r in range(len(room_start) - 1):
        if keys is not None and not 0 <= int(keys[r]) < n_table:
            continue
        for b in order[room_start[r]:room_start[r + 1]]:
            e = r * (1 + N) + (1 + int(slot_of[b]) if slot_of[b] >= 0 else 0)
            out[b], out_n[b] = enc_packets[e], enc_bytes[e]
    return out, out_n


def check_labels(rooms, labels, limit):
    """What lyra_hip_shared_begin holds room_labels to: strictly ascending, below `limit`, exactly the labels >= 0 in rooms"""
    present = sorted(set(int(v) for v in rooms if v >= 0))
    return [int(v) for v in labels] == present and all(0 <= v < limit for v in present)


# ---- the scripted conference ----------------------------------------------------------------------------------------------

EVENTS = ("order changed, slots kept", "newcomer took the freed slot", "two newcomers, the louder one lower",
          "fewer speakers than N", "N shrank, slots >= N cleared", "the id of a participant in another room freed",
          "an id twice in a row, the lower slot won")


def slot_script(seed=3):
    """45 ticks of 12 rows (stream ids 20, 31, 42, ...): room 0 = rows 0..5, room 1 = rows 6..9, rows 10 and 11 in no room; from
    tick 35 row 4 sits in room 1.  Table of 7 rows, room 0 at key 5 and room 1 at key 2.  Room 0 is written by hand, five ticks
    a phase (amplitudes; the level is 320 * amp^2), room 1 is random.  -> list of dicts: x int16 [12][320], rooms, N, and
    `poke`: (key, slot, from_slot) to copy inside the table BEFORE the tick, or None."""
    rng = np.random.default_rng(seed)
    quiet = [20, 30, 25, 15, 35, 10]
    phases = [  # (N, amplitudes of rows 0..5)
        (3, [900, 800, 700, None, None, None]),    # slots: row 0 -> 0, row 1 -> 1, row 2 -> 2
        (3, [900, 800, 950, None, None, None]),    # the same three, another order
        (3, [900, 5, 950, None, 850, None]),       # row 1 leaves, row 4 arrives: slot 1
        (3, [5, 5, 6, 990, 850, 600]),             # rows 0 and 2 leave, rows 3 (louder) and 5 arrive: slots 0 and 2
        (3, [0, 0, 0, 990, 850, 0]),               # two candidates only: slot 2 stays free
        (3, [0, 0, 0, 990, 850, 600]),             # row 5 is back: slot 2
        (2, [0, 0, 0, 990, 850, 600]),             # N = 2: slot 2 is cleared
        (3, [700, 0, 0, 990, 850, 600]),           # row 4 is in room 1 now: its id leaves room 0's row
        (3, [700, 0, 0, 990, 850, 600]),           # ... and the table is poked: slot 0's id copied into another slot
    ]
    ticks = []
    for p, (N, amps) in enumerate(phases):
        for i in range(5):
            t = 5 * p + i
            rooms = np.array([0] * 6 + [1] * 4 + [-1] * 2, np.int32)
            if t >= 35:
                rooms[4] = 1
            amp = np.zeros(12, np.int64)
            amp[:6] = [quiet[b] if a is None else a + ((t + b) % 3 if a > 100 else 0) for b, a in enumerate(amps)]
            amp[6:] = rng.integers(0, 2000, 6)
            x = (amp[:, None] * rng.choice([-1, 1], (12, HOP16))).astype(np.int16)
            ticks.append({"x": x, "rooms": rooms, "N": N, "poke": (5, None, 0) if t == 40 else None})
    return ticks, np.arange(12, dtype=np.int32) * 11 + 20, np.array([5, 2], np.int32), 7


def run_slot_script(ticks, ids, keys, n_table, fill=-1):
    """The model over the script -> (per tick: dict with the table before and after, speakers as ids, N, slot_of, enc_mix,
    levels, is_speaker; and the events counted).  A poke with slot None picks a slot that holds another speaker who stays."""
    table = np.full((n_table, SLOTS), fill, np.int32)
    table[keys] = -1
    seen = dict.fromkeys(EVENTS, 0)
    out, prev = [], None
    for t, tick in enumerate(ticks):
        order, start = np_bridge_plan(tick["rooms"])
        N = tick["N"]
        if tick["poke"]:
            q, j, src = tick["poke"]
            if j is None:
                j = 2 if src != 2 else 1
            table[q, j] = table[q, src]
            tick = dict(tick, poke=(q, j, src))
        before = table.copy()
        enc_mix, levels, is_speaker, slot_of, table, speakers = np_shared_mix(tick["x"], ids, order, start, N, table, keys)
        spk_ids = [[int(ids[b]) for b in chosen] for chosen in speakers]
        rec = dict(tick=tick, order=order, start=start, N=N, before=before, after=table.copy(), speakers=spk_ids,
                   slot_of=slot_of, enc_mix=enc_mix, levels=levels, is_speaker=is_speaker)
        _count_events(seen, prev, rec, ids, keys)
        out.append(rec)
        prev = rec
    return out, seen


def _count_events(seen, prev, rec, ids, keys):
    N = rec["N"]
    for r, now in enumerate(rec["speakers"]):
        q = int(keys[r])
        old, new = [int(v) for v in rec["before"][q]], [int(v) for v in rec["after"][q]]
        if len(now) < N:
            assert new.count(-1) == SLOTS - len(now)
            seen[EVENTS[3]] += 1
        dup = [j for j in range(N) if old[j] >= 0 and old[j] in old[:j] and old[j] in now]
        if dup:
            assert all(new[old.index(old[j])] == old[j] and new[j] != old[j] for j in dup)
            seen[EVENTS[6]] += 1
            continue
        elsewhere = set(int(ids[b]) for b in np.flatnonzero((rec["tick"]["rooms"] >= 0) & (rec["tick"]["rooms"] != [0, 1][r])))
        if any(v in elsewhere for v in old[:N]):
            assert not any(v in elsewhere for v in new)
            seen[EVENTS[5]] += 1
        if prev is None or r >= len(prev["speakers"]):
            continue
        was = prev["speakers"][r]
        if prev["N"] > N and any(v >= 0 for v in old[N:]):
            assert all(v == -1 for v in new[N:])
            seen[EVENTS[4]] += 1
        if prev["N"] != N:
            continue
        if set(was) == set(now) and was != now and len(now) > 1:
            assert new == old
            seen[EVENTS[0]] += 1
        gone, come = [v for v in was if v not in now], [v for v in now if v not in was]
        if len(gone) == 1 and len(come) == 1 and len(now) == len(was) and gone[0] in old:
            assert new.index(come[0]) == old.index(gone[0]) and all(new[j] == old[j] for j in range(SLOTS) if old[j] != gone[0])
            seen[EVENTS[1]] += 1
        if len(come) == 2 and all(v not in old for v in come):
            first, second = sorted(come, key=now.index)          # (selection order: the louder one first)
            assert new.index(first) < new.index(second)
            free = [j for j in range(N) if old[j] not in now or old[j] < 0]
            assert new.index(first) == free[0] and new.index(second) == free[1]
            seen[EVENTS[2]] += 1
