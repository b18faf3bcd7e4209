"""CPU checks of tests/state_bridge.py, the bridge between the oracle's per-stream state and the product's stream blob:
the tensor table covers the stage regions exactly, a fresh oracle stream becomes the product's reset blob, and
oracle state -> blob -> oracle state is the identity at ring phases before, at and after every wrap-around (a dilation-9
ring wraps after 9 hops, the phase word after 18)."""
import subprocess

import numpy as np
import pytest

from oracle_states import directed_oracle_run
import state_bridge
from state_bridge import _reset_blob, _verdicts

MODES = ["xnnpack", "exact", "gemmlowp_double", "builtin_mixed"]


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    return state_bridge.compile_tool(tmp_path_factory.mktemp("blob_tool"))


@pytest.fixture(scope="module")
def bridge(tool):
    return state_bridge.Bridge(tool)


@pytest.fixture(scope="module")
def oracles(oracle_default, oracle_exact, oracle_double, oracle_mixed):
    return {"xnnpack": oracle_default, "exact": oracle_exact, "gemmlowp_double": oracle_double, "builtin_mixed": oracle_mixed}


def _noise(seed, hops):
    return np.random.default_rng(seed).integers(-32768, 32768, size=(hops, 320), dtype=np.int16)


def _hop(oracle, stream, pcm, packet=None):
    """one hop of everything that moves the table's tensors: log-mel, encode at 184 bits, decode (own packet or `packet`)"""
    mel = stream.logmel(pcm)
    feat = stream.encode(pcm)
    idx = oracle.rvq_encode(feat, 46)
    pk = oracle.pack(idx, 46)[0]
    use = pk if packet is None else packet
    out = stream.decode(oracle.rvq_decode(oracle.unpack(use, 46))[0])
    return mel, pk, out


def _same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


def test_table_covers_the_stage_regions_exactly_once(bridge):
    use, scope = bridge.use_count(), bridge.scope()
    assert use.max() == 1, "two table rows (or a row and a phase word) claim the same byte"
    assert not use[~scope].any(), "a table row reaches outside the six stage regions and M_PREV"
    names = [t.name for t in bridge.tensors]
    assert len(names) == len(set(names)) == 33            # the 32 tensors of the stage regions + mel_prev
    # the stage regions hold 4 phase words; what the table leaves over is the header padding of the four ringed regions
    # (HDR - 4 bytes each) plus each region's alignment tail, and nothing else
    K, left = bridge.K, 0
    for r in state_bridge.ENC_REGIONS + state_bridge.DEC_REGIONS:
        off, n = bridge.region(r)
        ts = sorted((t.off, t.off + t.nbytes) for t in bridge.tensors if t.region == r)
        first = K["HDR"] if r in state_bridge.PHASED else 0
        assert ts[0][0] == first, (r, ts[0])
        assert all(a[1] == b[0] for a, b in zip(ts, ts[1:])), f"region {r}: a gap or an overlap between tensors"
        assert 0 <= n - ts[-1][1] < 256, f"region {r}: more than alignment behind its last tensor"
        left += (first - 4 if first else 0) + n - ts[-1][1]
    assert int(bridge.padding().sum()) == left
    m = bridge.by_name["mel_prev"]
    assert m.off == K["M_PREV"] and m.nbytes == 640
    # every oracle tensor has a row of the same size
    from oracle import lyra_oracle
    s = lyra_oracle.Stream(lyra_oracle.Oracle(mode="xnnpack"))
    st = s.state()
    assert list(st) == names
    for t in bridge.tensors:
        assert st[t.name].size == t.R * t.C and st[t.name].dtype == (np.float64 if t.dtype == "i16" else np.float32)
        assert t.ring == (t.T < t.R)
    assert sorted(t.name for t in bridge.tensors if t.ring) == sorted(
        ["e_r1[1]", "e_r1[2]", "e_r2[1]", "e_r2[2]", "e_bott", "d_head", "d_r0[1]", "d_r0[2]", "d_r1[1]", "d_r1[2]"])


def _reset_zero_points():
    """the seven zero points as lyra_hip_reset_streams takes them (model.hip: the INPUT zero point of the layer that reads
    the history), read from other container entries than the table's producer entries"""
    q = state_bridge.read_pack()
    return [int(q[k][1]) for k in ("enc.dw.7.q", "enc.dw.8.q", "enc.conv.21.q", "enc.conv.22.q", "dec.dw.0.q", "dec.dw.1.q", "dec.dw.2.q")]


@pytest.mark.parametrize("mode", MODES)
def test_fresh_oracle_stream_is_the_reset_blob(bridge, tool, oracles, tmp_path, mode):
    from oracle import lyra_oracle
    m = state_bridge.MODES[mode]
    plain = _reset_blob(tool, tmp_path, mode=m)            # validate()'s stand-in: int8 histories zero
    path = str(tmp_path / "reset_z.bin")
    subprocess.check_call([tool, "reset", path, str(m)] + [str(z) for z in _reset_zero_points()])
    product = np.fromfile(path, np.uint8)                  # ... and holding their zero points, as after a reset on the device
    s = lyra_oracle.Stream(oracles[mode])
    blob = bridge.to_blob(s.state(), 0, 0, mode, plain)
    assert np.array_equal(blob, product), np.flatnonzero(blob != product)[:8]
    i8 = np.zeros(bridge.bytes, bool)
    for t in bridge.tensors:
        if t.dtype == "i8":
            a, b = bridge.span(t)
            i8[a:b] = True
            assert (blob[a:b].view(np.int8) == t.zero).all()
    assert np.array_equal(blob[~i8], plain[~i8])           # outside the int8 histories: the stand-in byte for byte
    assert _verdicts(tool, tmp_path, np.stack([blob, product]), mode=m) == [0, 0]
    _same_state(bridge.from_blob(blob), s.state())


@pytest.mark.parametrize("mode", MODES)
def test_round_trip_and_continuation(bridge, tool, oracles, tmp_path, mode):
    from oracle import lyra_oracle
    oracle = oracles[mode]
    header = _reset_blob(tool, tmp_path, mode=state_bridge.MODES[mode])
    pcm = _noise(20251, 37 + 20)
    s = lyra_oracle.Stream(oracle)
    blobs = []
    for hop in range(37):
        _hop(oracle, s, pcm[hop])
        if hop + 1 in (1, 9, 18, 37):
            st = s.state()
            blob = bridge.to_blob(st, hop + 1, hop + 1, mode, header)
            _same_state(bridge.from_blob(blob), st)
            assert bridge.phases(blob) == {r: (hop + 1) % 18 for r in state_bridge.PHASED}
            assert not blob[bridge.padding()].any()
            blobs.append(blob)
            if hop + 1 in (9, 37):      # mid-way and at the end: a restored stream continues like the original
                twin = lyra_oracle.Stream(oracle)
                twin.set_state(bridge.from_blob(blob))
                keep = s.state()
                for k in range(20):
                    a, b = _hop(oracle, s, pcm[37 + k]), _hop(oracle, twin, pcm[37 + k])
                    for x, y in zip(a, b):
                        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (hop + 1, k)
                _same_state(s.state(), twin.state())
                s.set_state(keep)       # ... and the original goes on from where it was
    assert _verdicts(tool, tmp_path, np.stack(blobs), mode=state_bridge.MODES[mode]) == [0] * len(blobs)
    # frame counts that differ between the sides land in their own regions' phase words
    blob = bridge.to_blob(s.state(), 5, 22, mode, header)
    assert bridge.phases(blob) == {state_bridge.R_E1: 5, state_bridge.R_E2: 5, state_bridge.R_D0: 4, state_bridge.R_D1: 4}


def test_to_blob_refuses_a_float_that_is_no_code(bridge, tool, oracle_default, tmp_path):
    from oracle import lyra_oracle
    s = lyra_oracle.Stream(oracle_default)
    _hop(oracle_default, s, _noise(3, 1)[0])
    st = s.state()
    header = _reset_blob(tool, tmp_path)
    t = bridge.by_name["d_r0[1]"]
    st["d_r0[1]"] = st["d_r0[1]"].copy()
    st["d_r0[1]"][7] = np.nextafter(dequant_one(t, 3), np.float32(1e9))
    with pytest.raises(AssertionError, match=r"d_r0\[1\]: element 7"):
        bridge.to_blob(st, 1, 1, "xnnpack", header)
    st["d_r0[1]"][7] = np.float32(t.scale) * np.float32(200)       # a multiple of the scale, but no int8 code
    with pytest.raises(AssertionError, match=r"d_r0\[1\]: element 7"):
        bridge.to_blob(st, 1, 1, "xnnpack", header)


def dequant_one(t, code):
    return state_bridge.dequantize(np.array([code]), t.scale, t.zero)[0]


@pytest.mark.parametrize("mode", MODES)
def test_directed_run_meets_its_conditions_on_the_oracle(bridge, oracles, mode):
    """the oracle's half of tests/test_gpu_state_vs_oracle.py::test_directed_states_one_hop_at_a_time, which asserts on the
    reference alone: finite state and outputs, every int8 tap at both rails on hop 1, PCM at both rails -- and that the
    directed states are states the blob can hold (every int8 float is a code)"""
    states0, pe, pd, _, _, per_hop, counts = directed_oracle_run(bridge, oracles[mode])
    assert len(counts) == 8 and all(lo > 0 and hi > 0 for lo, hi, _ in counts.values()), counts
    assert set(int(v) for v in pe) | set(int(v) for v in pd) >= {0, 17}     # both ends of the phase range are drawn
    for t in bridge.tensors:      # every code value of every int8 tensor occurs in the batch
        if t.dtype == "i8":
            codes = np.concatenate([bridge.codes_of(t, st[t.name].reshape(t.R, t.C)).ravel() for st in states0])
            assert np.unique(codes).size == 256, t.name
