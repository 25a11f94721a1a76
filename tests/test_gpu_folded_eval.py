"""mira_graph_eval_folded_device / mira_graph_eval_folded_reduce on the GPU (tests/folded_eval.py has the cases)."""
import pytest

import folded_eval as FE

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("field", FE.FIELDS)
def test_leaves_against_python_integers(gpu_lib, field):
    FE.check_leaves(gpu_lib, field)


@pytest.mark.parametrize("field", FE.FIELDS)
def test_identities_against_the_plain_evaluation(gpu_lib, field):
    FE.check_identities(gpu_lib, field)


@pytest.mark.parametrize("field", FE.FIELDS)
def test_worst_case_operands(gpu_lib, field):
    FE.check_worst_case(gpu_lib, field)


@pytest.mark.parametrize("field", FE.FIELDS)
def test_reduce_against_the_definition(gpu_lib, field):
    FE.check_reduce(gpu_lib, field)


@pytest.mark.parametrize("k,satisfied,num_traces", [(6, True, 1), (9, False, 2), (10, True, 3)])
def test_pipeline(gpu_lib, k, satisfied, num_traces):
    FE.check_pipeline(gpu_lib, k, satisfied, num_traces)


@pytest.mark.parametrize("field", FE.FIELDS)
def test_refusals(gpu_lib, field):
    FE.check_refusals(gpu_lib, field)


@pytest.mark.parametrize("field", FE.FIELDS)
def test_guard_bands(gpu_lib, field):
    FE.check_guarded(gpu_lib, field)


@pytest.mark.parametrize("field", FE.FIELDS)
def test_scratch_state(gpu_lib, field):
    FE.check_scratch_state(gpu_lib, field)


def test_specialised_handles_are_interpreted(gpu_lib):
    FE.check_specialised(gpu_lib, pytest.skip)
