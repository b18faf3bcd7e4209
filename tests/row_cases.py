"""The GPU tests of the per-row device calls (a bit count, a sample rate or a packet size per row): sentinel rows and their check,
the per-row draws, the rates call, the comparison of exported state.  No tests here; torch is imported inside the functions."""
import numpy as np

from gpu_plumbing import _dev, _t
from signals import EXT_ROW, RATES

ROW = EXT_ROW                             # samples between two rows of external-rate PCM
SENTINEL = 0xA5                           # every byte of a packet buffer before the call
ENC_BITS = (64, 120, 184, 4, 100, 180)    # bit counts drawn per row: the three bitrates and other multiples of 4


def _rates(B):
    """Fixed per stream; with every third stream silent (DTX input) every rate has silent and speaking streams from B = 12."""
    return np.array([RATES[(b // 3) % 4] for b in range(B)], np.int32)


def _draw_bits(rng, B):
    return rng.choice(ENC_BITS, size=B, p=[0.25, 0.25, 0.25, 0.08, 0.09, 0.08]).astype(np.int32)


def _check_sentinel_rows(got_pk, got_pb, want_pk, want_pb, where):
    """packet_bytes equal, every row equal up to its size, the sentinel behind it"""
    assert np.array_equal(got_pb, want_pb), (where, "packet_bytes differ in rows", np.flatnonzero(got_pb != want_pb)[:8], got_pb, want_pb)
    for b in range(got_pb.size):
        n = int(got_pb[b])
        assert np.array_equal(got_pk[b, :n], want_pk[b, :n]), (where, b, "the packet differs")
        assert (got_pk[b, n:] == SENTINEL).all(), (where, b, "bytes past packet_bytes were written")


def _decode_rates(a, ids, pk_t, sz_t, rates, dn=None):
    """decode_lossy_rates_dev -> (pcm16, ext rows over 0x3333, is_noise, is_comfort_noise); dn: a persistent is_noise buffer
    (default: a fresh one of -3)."""
    import torch
    B = ids.size
    d16 = torch.zeros((B, 320), dtype=torch.int16, device=_dev())
    dx = torch.full((B, ROW), 0x3333, dtype=torch.int16, device=_dev())
    if dn is None:
        dn = torch.full((B,), -3, dtype=torch.int32, device=_dev())
    dc = torch.full((B,), -3, dtype=torch.int32, device=_dev())
    a.decode_lossy_rates_dev(_t(ids), _t(pk_t), _t(sz_t), _t(rates), d16, dx, dn, dc)
    a.synchronize()
    return d16.cpu().numpy(), dx.cpu().numpy(), dn.cpu().numpy(), dc.cpu().numpy()


def _same_state(a, u, ids, where):
    sa, su = a.export_streams(ids), u.export_streams(ids)
    bad = np.flatnonzero((sa != su).any(axis=1))
    assert bad.size == 0, (where, "exported state differs for rows", bad[:8],
                           "first byte", int(np.flatnonzero(sa[bad[0]] != su[bad[0]])[0]) if bad.size else None)
