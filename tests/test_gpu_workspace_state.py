"""-m gpu: stale internal workspaces (tests/workspace_state.py) on the GPU build.  The library's grow-only buffers are shared by
every key and every call and never cleared; these runs put every route of the MSM table after every other one -- A at 12293 pairs,
B at 4097 on another key, another kind of vector and, for half of the pairs, the other curve, B a second time, then small A and
large B -- on prefixes of one synthetic key of 12293 points per curve, with `fresh` (mira_trim(0)) as one more A.  The other
workspaces go large, small, large: the transforms with their cache of twiddle tables, the lookup's hash table, the inversion,
the deciders, the trees, the graph engines (run-time specialised kernels among them) and the folds; one seeded schedule
interleaves all families; and every error path that runs kernels before it refuses is followed by valid calls.

Every point is compared with the C oracle's, everything else with Python integers, byte for byte.  (Poisoned workspaces are the
emulation's business, tests/test_workspace_state_emu.py: on a device the fill would be an out-of-range index.)"""
import pytest

import workspace_state as WS

pytestmark = pytest.mark.gpu

LARGE, SMALL = 12293, 4097


@pytest.fixture(scope="module")
def bench(gpu_lib):
    with WS.Bench(gpu_lib, LARGE) as b:
        yield b


@pytest.mark.parametrize("a", [WS.FRESH] + WS.route_names())
def test_route_b_after_a(gpu_lib, bench, a):
    """the full square of the table, one row a test"""
    WS.check_pairs(gpu_lib, a, WS.route_names(), LARGE, SMALL, bench=bench)


def test_ntt_sequence(gpu_lib):
    WS.check_ntt_sequence(gpu_lib)


@pytest.mark.parametrize("field", WS.E.FIELDS)
def test_lookup_and_inversion_sequence(gpu_lib, field):
    WS.check_lookup_sequence(gpu_lib, field)


@pytest.mark.parametrize("field", WS.E.FIELDS)
def test_decider_sequence(gpu_lib, field):
    WS.check_decider_sequence(gpu_lib, field)


@pytest.mark.parametrize("field", WS.E.FIELDS)
def test_tree_and_fold_sequences(gpu_lib, field):
    WS.check_pow_tree_sequence(gpu_lib, field)
    WS.check_fold_sequence(gpu_lib, field)


@pytest.mark.parametrize("field", WS.E.FIELDS)
def test_graph_sequence(gpu_lib, field):
    """interpreter, compiled engine and batch at 2048 -> 64 -> 2048 -> 300 rows; then the same graphs through kernels of their own at
    2048 -> 64 -> 300 rows (one run-time compilation serves all three)"""
    WS.check_graph_sequence(gpu_lib, field)
    WS.check_graph_sequence(gpu_lib, field, specialise=True, rows=(2048, 64, 300))


def test_interleaved_schedule(gpu_lib, bench):
    WS.check_schedule(gpu_lib, LARGE, SMALL, WS.route_names(), bench=bench)


def test_calls_after_a_refusal(gpu_lib, tmp_path):
    WS.check_refusals(gpu_lib, tmp_dir=str(tmp_path))
