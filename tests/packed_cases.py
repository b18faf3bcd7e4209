"""The tests of the span calls on a packed external-rate buffer (include/lyra_hip_spans_packed.h): the flat buffer and its check,
the layout restated in Python.  No tests here; torch and lyra_amd are imported inside the functions."""
import numpy as np

from span_cases import FILL16

HOPS = {8000: 160, 16000: 320, 32000: 640, 48000: 960}
# the layout of tests/test_gpu_spans_rates.py: (stream id, frames, rate)
LAYOUT = [(7, 140, 48000), (11, 1, 8000), (3, 0, 32000), (20, 60, 8000), (5, 5, 16000), (9, 3, 32000), (13, 61, 16000)]
LAYOUT_OFFSETS = [0, 134400, 134560, 134560, 144160, 145760, 147680]
LAYOUT_TOTAL = 167200


def _back_to_back(frames, rates):
    """offsets and total of the back-to-back layout, or None for what the library refuses"""
    at, offsets = 0, []
    for n, r in zip(frames, rates):
        if r not in HOPS or n < 0:
            return None
        offsets.append(at)
        at += n * HOPS[r]
    return offsets, at


def _scattered(frames, rates, order, gap=8):
    """offsets that put the spans into the flat buffer in `order`, `gap` samples of filler in front of each and behind the
    last: offsets by span, total"""
    at, offsets = gap, [0] * len(frames)
    for s in order:
        offsets[s] = at
        at += frames[s] * HOPS[rates[s]] + gap
    return offsets, at


def _flat(spans, rates, ext_by_id, offsets, total):
    """the flat buffer [total]: span s's samples from offsets[s], FILL16 everywhere else"""
    buf = np.full(total, FILL16, np.int16)
    for (i, _, n), r, off in zip(spans, rates, offsets):
        buf[off:off + n * HOPS[r]] = np.asarray(ext_by_id[i], np.int16).reshape(-1)
    return buf


def _check_flat(where, got, spans, rates, offsets, want_by_id):
    """span s's n * rate / 50 samples from offsets[s] equal the twin's rows; every other sample still holds the filler"""
    untouched = np.ones(len(got), bool)
    for (i, _, n), r, off in zip(spans, rates, offsets):
        hop = HOPS[r]
        untouched[off:off + n * hop] = False
        if not n:
            continue
        rows, want = got[off:off + n * hop].reshape(n, hop), np.asarray(want_by_id[i]).reshape(n, hop)
        diff = np.flatnonzero((rows != want).any(axis=1))
        assert len(diff) == 0, f"{where}: stream {i} ({r} Hz) differs at hops {diff[:8].tolist()} ({len(diff)} of {n})"
    assert (got[untouched] == FILL16).all(), f"{where}: samples in front of, behind or between the spans were written"


def _check_offsets(frames, rates, offsets, n_ext):
    """the offset check of a packed call restated: True = accepted (lyra_amd/csrc/spans_packed_plan.h)"""
    if n_ext < 0:
        return False
    ranges = []
    for n, r, off in zip(frames, rates, offsets):
        if r not in HOPS or n < 0 or off < 0 or off % 8:
            return False
        if n:
            if off + n * HOPS[r] > n_ext or off >= 1 << 34:
                return False
            ranges.append((off, off + n * HOPS[r]))
    ranges.sort()
    return all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:]))
