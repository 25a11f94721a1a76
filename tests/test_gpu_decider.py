"""-m gpu: the deciders through libmira_gpu.so -- the bodies of tests/decider_cases.py on the device, and the row sweep once more
through run-time specialised kernels."""
import pytest

import decider_cases as DC
from mira_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture
def lib(gpu_lib):
    yield gpu_lib
    gpu_lib.tune(_lib.TUNE_DECIDE_GRID, -1)


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
def test_graph_check_specialized(lib, field):
    """the same handles after mira_graph_specialize give the same numbers"""
    reason = DC.run_graph_check(lib, field, specialize=True)
    if reason is not None:
        pytest.skip(reason)


@pytest.mark.parametrize("field", DC.FIELDS)
def test_is_sat_and_is_sat_relaxed_end_to_end(lib, field):
    DC.run_end_to_end(lib, field)
