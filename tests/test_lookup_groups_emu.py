"""Colliding hashes and the small group structures of the lookup multiplicities (tests/lookup_groups.py) on the CPU emulation.
Keys of equal lk_hash start their probe chains at one slot here as on the device; the wave groups themselves are the device's
(tests/test_gpu_lookup_groups.py) -- the emulation's every lane leads a group of one."""
import pytest

import lookup_groups as LG


def test_the_restated_hash_and_the_pairs():
    assert LG.lk_hash(0) == LG.lk_hash(0) and LG.lk_hash(0) != LG.lk_hash(1)
    pairs = LG.colliding_pairs()
    assert len(pairs) >= 8 and len({v for p in pairs for v in p}) == 2 * len(pairs)
    for a, b in pairs:
        assert a != b and LG.lk_hash(a) == LG.lk_hash(b) and a >> 224 == 0 and 0 < b >> 224 < 1 << 29
    import numpy as np
    reps = [a for a, _ in pairs] + [b for _, b in pairs]
    words = np.array([[(r >> (32 * i)) & 0xFFFFFFFF for i in range(8)] for r in reps], dtype=np.uint32)
    assert LG._states(words).tolist() == [LG.lk_hash(r) for r in reps]     # the numpy restatement and the Python one agree


@pytest.mark.parametrize("field", LG.E.FIELDS)
@pytest.mark.parametrize("k", range(len(LG.pair_cases(0))), ids=[c.name for c in LG.pair_cases(0)])
def test_colliding_pairs(emu_lib, field, k):
    LG.check_case(emu_lib, field, LG.pair_cases(field)[k])


@pytest.mark.parametrize("field", LG.E.FIELDS)
@pytest.mark.parametrize("kind", LG.STRUCTURES)
def test_group_structures(emu_lib, field, kind):
    for case in LG.structure_cases(field):
        if case.name.startswith(f"t {kind} "):
            LG.check_case(emu_lib, field, case)


@pytest.mark.parametrize("field", LG.E.FIELDS)
def test_more_hot_values_than_workgroup_slots(emu_lib, field):
    for case in LG.count_cases(field, big=False):
        LG.check_case(emu_lib, field, case)
