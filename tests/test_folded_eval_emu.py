"""mira_graph_eval_folded_device / mira_graph_eval_folded_reduce on the CPU emulation of the kernels (tests/folded_eval.py has the
cases).  The emulation is built with the bound tracking of field29.cuh: a folded value that entered the program above the
bound the compiler assumed for a column would abort the process here.  Its workgroups are 32 lanes (OS threads that meet at
every barrier of the in-workgroup tree), so a row count of 2^11 is 64 row blocks."""
import pytest

import folded_eval as FE


@pytest.mark.parametrize("field", FE.FIELDS)
def test_leaves_against_python_integers(emu_lib, field):
    FE.check_leaves(emu_lib, field)


@pytest.mark.parametrize("field", FE.FIELDS)
def test_identities_against_the_plain_evaluation(emu_lib, field):
    FE.check_identities(emu_lib, field)


@pytest.mark.parametrize("field", FE.FIELDS)
def test_worst_case_operands_stay_in_the_budget(emu_lib, field):
    FE.check_worst_case(emu_lib, field)


@pytest.mark.parametrize("field", FE.FIELDS)
def test_reduce_against_the_definition(emu_lib, field):
    FE.check_reduce(emu_lib, field)


@pytest.mark.parametrize("k,satisfied,num_traces", [(2, True, 1), (3, False, 2), (3, True, 3)])
def test_pipeline(emu_lib, k, satisfied, num_traces):
    FE.check_pipeline(emu_lib, k, satisfied, num_traces)


@pytest.mark.parametrize("field", FE.FIELDS)
def test_refusals(emu_lib, field):
    FE.check_refusals(emu_lib, field)


@pytest.mark.parametrize("field", FE.FIELDS)
def test_guard_bands(emu_lib, field):
    FE.check_guarded(emu_lib, field)


@pytest.mark.parametrize("field", FE.FIELDS)
def test_scratch_state(emu_lib, field):
    FE.check_scratch_state(emu_lib, field)
