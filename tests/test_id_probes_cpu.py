"""CPU checks of tests/id_probes.py, the probe ids of tests/test_gpu_id_range.py: with a made-up layout and with the
product's own (slot sizes from tests/stream_state/blob_tool.cc compiled over stream_blob.h, as tests/state_bridge.py takes
them), the set holds both sides of every 2^31 crossing, the witnesses are no probes, the last slot under the cap ends inside
2^32 in every region, and the cap is the number lyra_hip_create's refusal prints."""
import ctypes
import re

import pytest

import id_probes
import state_bridge

# stage slots of a made-up layout: two that never reach 2^31 under the cap, one that hits it exactly, one that is no multiple
# of 256, the widest; side slots narrower than the widest
FAKE_STAGE = [1000, 16384, 9984, 12345, 20000, 8192]
FAKE_ALL = FAKE_STAGE + [768, 4096, 4096, 512, 512, 8448]


@pytest.fixture(scope="module")
def bridge(tmp_path_factory):
    return state_bridge.Bridge(state_bridge.compile_tool(tmp_path_factory.mktemp("blob_tool")))


def _check_plan(stage, all_bytes):
    cap = id_probes.cap_of(all_bytes)
    plan = id_probes.probe_plan(stage, cap)
    probes, order, wit = plan["probes"], plan["order"], plan["witnesses"]
    assert probes == sorted(set(probes)) and sorted(order) == probes
    assert all(0 <= p < cap for p in probes)
    for b in all_bytes:                                   # (cap - 1 + 1) * bytes <= 2^32: the last slot ends inside 32 bits
        assert (cap - 1 + 1) * b <= 1 << 32
    assert (cap + 1) * max(all_bytes) > 1 << 32           # ... and the cap is the largest such count
    for r, b in enumerate(stage):                         # both sides of every crossing
        k = -(-(1 << 31) // b)
        if k <= cap - 1:
            assert plan["cross"][r] == k and k in probes and k - 1 in probes
            assert k * b >= 1 << 31 > (k - 1) * b
        else:
            assert r not in plan["cross"] and (cap - 1) * b < 1 << 31
    for p in (0, 1, id_probes.OLD_EDGE - 1, id_probes.OLD_EDGE, cap - 2, cap - 1):
        assert p in probes
    fixed = {0, 1, id_probes.OLD_EDGE - 1, id_probes.OLD_EDGE, cap - 2, cap - 1}
    fixed |= {k - d for k in plan["cross"].values() for d in (0, 1)}
    assert sum(p >= cap // 2 for p in probes if p not in fixed) >= 8, "eight drawn ids in the upper half"
    assert len(probes) % id_probes.TILE != 0
    for t in range(0, len(order), id_probes.TILE):         # every tile of the call mixes both ends of the arena
        tile = order[t:t + id_probes.TILE]
        assert min(tile) < cap // 2 <= max(tile), tile
    assert wit and not set(wit) & set(probes) and all(0 <= w < cap for w in wit)
    for p in probes:
        for q in (p - 1, p + 1):
            assert q in wit or q in probes or not 0 <= q < cap
    again = id_probes.probe_plan(stage, cap)
    assert again == plan, "the plan is a pure function of its arguments"
    return cap, plan


def test_probe_plan_of_a_made_up_layout():
    cap, plan = _check_plan(FAKE_STAGE, FAKE_ALL)
    assert cap == (1 << 32) // 20000
    assert sorted(plan["cross"]) == [1, 3, 4]              # 16384 crosses exactly at 2^31, 9984 and 8192 and 1000 never do
    assert plan["cross"][1] * 16384 == 1 << 31


def test_probe_plan_of_the_product_layout(bridge):
    stage = [bridge.region(r)[1] for r in range(id_probes.N_STAGE_REGIONS)]
    all_bytes = [bridge.region(r)[1] for r in range(len(bridge.L["region_bytes"]))]
    assert all_bytes == bridge.L["region_bytes"]
    cap, plan = _check_plan(stage, all_bytes)
    # worked by hand from state_layout.h, as a cross-check of the helper (the GPU tests take the ids from the helper)
    assert cap == 289262 and (1 << 32) - cap * max(all_bytes) == 5120
    assert plan["cross"] == {state_bridge.R_E0: 262144, state_bridge.R_E1: 147169, state_bridge.R_E2: 215093,
                             state_bridge.R_D0: 204601, state_bridge.R_D1: 144632}
    assert plan["cross"][state_bridge.R_E0] * stage[state_bridge.R_E0] == 1 << 31
    print(f"cap {cap}; {len(plan['probes'])} probes in call order {plan['order']}; {len(plan['witnesses'])} witnesses")


def test_cap_is_what_create_refuses_above(bridge):
    import lyra_amd
    lyra_amd.build_library()
    lib = ctypes.CDLL(lyra_amd.library_path())
    lib.lyra_hip_create.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.lyra_hip_last_error.restype = ctypes.c_char_p
    cap = id_probes.cap_of(bridge.region(r)[1] for r in range(len(bridge.L["region_bytes"])))
    h = ctypes.c_void_p()
    rc = lib.lyra_hip_create(lyra_amd.default_model_dir().encode(), 0, cap + 1, 0, ctypes.byref(h))
    assert rc == -1 and not h.value, rc                   # LYRA_HIP_EINVAL, with or without a GPU: the check comes first
    m = re.search(rb"at most (\d+) streams", lib.lyra_hip_last_error(None))
    assert m and int(m.group(1)) == cap, lib.lyra_hip_last_error(None)
