"""The convs that close the fp32 stage kernels (enc_s0 k10/s5, enc_s1 k4/s2, dec_s1 tconv k10/s5, dec_s2 tconv k64/s16)
stream their weights through a ring deeper than their activations' (lyra_dev.h gemm_f32_core PFB) and request the ring's
first stages in front of the barrier that precedes them.  Only the points at which loads are issued moved: features, packets
and PCM stay the CPU oracle's bit for bit -- at one stream, either side of a 4-stream tile (the 64-channel stages), either
side of an 8-stream tile (the 128-channel stages) and with a ragged last tile of both, over 20 hops: more than the 18 ring
phases, so the carried rows of every strided / transposed conv wrap.
"""
import numpy as np
import pytest

import signals

pytestmark = pytest.mark.gpu

BITS, HOPS, BMAX = 184, 20, 17
BATCHES = [1, 3, 4, 5, 8, 9, 17]


@pytest.fixture(scope="module")
def ctx():
    import lyra_amd
    c = lyra_amd.LyraHip(max_streams=8192)
    assert c.requant == "xnnpack"
    yield c
    c.close()


@pytest.fixture(scope="module")
def reference(oracle_default):
    """One oracle run for every case: streams are independent, so batch B is the first B streams of the largest one."""
    from oracle import lyra_oracle
    pcm = signals.synth(BMAX, HOPS, seed=0xC105)
    pcm[5:7] //= 64   # some quiet hops too
    r = lyra_oracle.run_batch(oracle_default, pcm, BITS // 4, do_decode=True, threads=4, want_feats=True)
    for a in (pcm, r["feats"], r["packets"], r["pcm"]):
        a.setflags(write=False)
    return pcm, r


@pytest.mark.parametrize("B", BATCHES)
def test_closing_convs_vs_oracle_bit_exact(ctx, oracle_default, reference, B):
    pcm, r = reference
    ctx.reset()
    ids = np.random.default_rng(B).permutation(4000)[:B].astype(np.int32)   # scattered stream ids
    for t in range(HOPS):
        feat = ctx.extract(pcm[t, :B], ids)
        assert np.array_equal(feat, r["feats"][t][:B]), f"features differ at hop {t}"
        idx = ctx.rvq_encode(feat, BITS)
        pk = oracle_default.pack(idx, BITS // 4)
        assert np.array_equal(pk, r["packets"][t][:B]), f"packets differ at hop {t}"
        out = ctx.decode(pk, BITS, ids)
        assert np.array_equal(out, r["pcm"][t][:B]), f"PCM not bit-exact at hop {t}"
