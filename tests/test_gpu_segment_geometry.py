"""-m gpu: the segment geometry of k_accumulate (tests/segment_geometry.py) on the GPU build, where the staged entry stream is
global_load_lds into LDS and its waits are real.  MIRA_TUNE_MIN_SEGMENT sweeps 1 .. 65; the shaped vectors put run ends, segment
ends and block boundaries where the model says, the dense ones fill the sorted buffer to its last word; every launch sequence
that ends in k_accumulate runs at a reduced list.  Every point is compared with the C oracle's, byte for byte."""
import pytest

import segment_geometry as SG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bench(gpu_lib):
    with SG.Bench(gpu_lib) as b:
        yield b


def test_the_cases_reach_every_class():
    reachable, reached = SG.check_coverage()
    assert reachable == reached


def test_unsupported_values_of_the_knob_are_refused(gpu_lib):
    SG.check_knob_refusals(gpu_lib)


@pytest.mark.parametrize("k", range(len(SG.cases())), ids=[c.name for c in SG.cases()])
def test_shaped(bench, k):
    SG.run_case(bench, SG.cases()[k])


@pytest.mark.parametrize("vector", range(len(SG.dense_vectors())))
def test_dense_sweep(bench, vector):
    """one dense vector at every L of the sweep; a full one behind a trim, so that the sorted buffer ends where its entries end"""
    for case in SG.dense_cases(vectors=(vector,)):
        SG.run_case(bench, case)


@pytest.mark.parametrize("L", SG.REDUCED)
@pytest.mark.parametrize("name", SG.OTHER_SEQUENCES)
def test_launch_sequences(bench, name, L):
    SG.run_sequence(bench, name, L, (L + len(name)) % 2)
