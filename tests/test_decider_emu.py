"""The deciders on the CPU emulation of the kernels (decide_kernels.cuh through the C ABI of the test-only build): compare-and-
count, field sums, the permutation check, the row sweep and is_sat / is_sat_relaxed end to end.  Bodies: tests/decider_cases.py;
the GPU suite (tests/test_gpu_decider.py) runs the same."""
import pytest

import decider_cases as DC
from mira_amd import _lib


@pytest.fixture
def lib(emu_lib):
    yield emu_lib
    emu_lib.tune(_lib.TUNE_DECIDE_GRID, -1)


@pytest.mark.parametrize("field", DC.FIELDS)
@pytest.mark.parametrize("n,grid", DC.SHAPES)
def test_count_ne(lib, field, n, grid):
    DC.run_count_ne(lib, field, n, grid)


@pytest.mark.parametrize("field", DC.FIELDS)
@pytest.mark.parametrize("n,grid", DC.SHAPES)
def test_sum_sub(lib, field, n, grid):
    DC.run_sum_sub(lib, field, n, grid)


@pytest.mark.parametrize("field", DC.FIELDS)
def test_noncanonical_input_is_an_error(lib, field):
    DC.run_noncanonical(lib, field)


@pytest.mark.parametrize("field", DC.FIELDS)
@pytest.mark.parametrize("num_io", [0, 2])
def test_perm_copy_constraints(lib, field, num_io):
    DC.run_perm_copy_constraints(lib, field, num_io)


@pytest.mark.parametrize("field", DC.FIELDS)
def test_perm_general_matrix(lib, field):
    DC.run_perm_general(lib, field)


@pytest.mark.parametrize("field", DC.FIELDS)
def test_perm_three_workgroups(lib, field):
    DC.run_perm_large(lib, field)


@pytest.mark.parametrize("field", DC.FIELDS)
def test_graph_check(lib, field):
    assert DC.run_graph_check(lib, field) is None


@pytest.mark.parametrize("field", DC.FIELDS)
def test_is_sat_and_is_sat_relaxed_end_to_end(lib, field):
    DC.run_end_to_end(lib, field)


def test_grid_knob_is_bounded(lib):
    lib.tune(_lib.TUNE_DECIDE_GRID, 3)
    lib.tune(_lib.TUNE_DECIDE_GRID, 2048)
    for knob, value in ((_lib.TUNE_DECIDE_GRID + 1, 1), (_lib.TUNE_DECIDE_GRID, 0), (_lib.TUNE_DECIDE_GRID, 2049)):
        with pytest.raises(_lib.MiraError) as err:
            lib.tune(knob, value)
        assert err.value.code == _lib.MIRA_E_BAD_ARG
