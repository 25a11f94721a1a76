"""-m gpu: wave groups and colliding hashes in the lookup multiplicities (tests/lookup_groups.py) on the GPU build, where the
match-any loop over the ballot, the leader's slot handed to its group, the once-per-group minimum and -- through keys of equal
hash -- the non-leader that probes for itself all run.  Expected m, h and g are Python's; every case runs twice under each hash
mode with byte-identical m."""
import pytest

import lookup_groups as LG

pytestmark = pytest.mark.gpu


def test_the_pairs_collide():
    pairs = LG.colliding_pairs()
    assert len(pairs) >= 8 and len({v for p in pairs for v in p}) == 2 * len(pairs)


@pytest.mark.parametrize("field", LG.E.FIELDS)
@pytest.mark.parametrize("k", range(len(LG.pair_cases(0))), ids=[c.name for c in LG.pair_cases(0)])
def test_colliding_pairs(gpu_lib, field, k):
    LG.check_case(gpu_lib, field, LG.pair_cases(field)[k])


@pytest.mark.parametrize("field", LG.E.FIELDS)
@pytest.mark.parametrize("k", range(len(LG.structure_cases(0))), ids=[c.name for c in LG.structure_cases(0)])
def test_group_structures(gpu_lib, field, k):
    LG.check_case(gpu_lib, field, LG.structure_cases(field)[k])


@pytest.mark.parametrize("field", LG.E.FIELDS)
@pytest.mark.parametrize("k", range(2))
def test_more_hot_values_than_workgroup_slots(gpu_lib, field, k):
    LG.check_case(gpu_lib, field, LG.count_cases(field, big=False)[k])


def test_second_trip_of_the_grid_stride_loop(gpu_lib):
    """2048 * 256 + 100 elements of l (16 MiB): workgroup 0 makes a second, partial trip; one value is counted by every workgroup"""
    LG.check_case(gpu_lib, LG.E.FIELD_FR, LG.count_cases(LG.E.FIELD_FR)[2])
