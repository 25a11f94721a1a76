"""P = Q, P = -Q and the identity through every stage and mode of the MSM on the GPU: the cases of tests/exceptional_points.py
under the same forced configuration as tests/test_exceptional_points_emu.py, whose branch census says which exits of the group
law each of them takes -- here the DPP-quad versions (quad29.cuh) really share their multiplications, with some quads of a wave
in xyzz29_double_quad or at the identity exit while others go on through quad_mul4.  Every result is byte for byte
(sum_i s_i k_i mod r) G from Python integers.

Beside the shared cases, what the emulation cannot cover:
  - the constants that `#ifdef MIRA_CPU_EMU` changes on the MSM path (msm_kernels.cuh, msm_host.cuh, ctx.h).  Launch geometry --
    HEAVY_BLOCK_A (256 lanes: up to 16 quads per sub-job, 32 under emulation), FIXUP_HEAVY_BLOCKS / FIXUP_HEAVY_GRID (256 / 1024,
    1 / 4), SET_FINISH_BLOCK (256, 32), REDUCE_SMALL_WG (workgroup sizes of the bucket tree) -- is the GPU's own in every test
    here.  MEDIUM_AS_CHAINS_FROM (1 024 medium runs, 8 under emulation) decides where medium runs are summed: the "chains" case
    has nine, sub-jobs of the heavy section on the GPU; test_medium_runs_as_chains floods the light section with more than 3 000
    (counted and asserted by the builder).
  - real widths 17 and 20, the every-bucket-heavy shapes of test_every_bucket_heavy, 2^19 pairs through the staged sort."""
import pytest

import exceptional_points as X
from mira_amd import _lib

pytestmark = pytest.mark.gpu


def _check(res):
    assert res
    bad = [label for label, got, want in res if not (got == want).all()]
    assert not bad, bad


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("mode", list(X.MODES))
def test_modes(gpu_lib, mode, cid):
    _check(X.run_mode(gpu_lib, mode, cid))


@pytest.mark.parametrize("cid", [0, 1])
def test_glv_forced_widths(gpu_lib, cid):
    _check(X.run_mode(gpu_lib, "glv", cid, widths=X.GLV_FORCED_WIDTHS, only=X.FEW))


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("bits", [20, 22])
def test_fixed_base_tables(gpu_lib, bits, cid):
    _check(X.run_tables(gpu_lib, cid, bits))


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("c", X.WIDE_WIDTHS)
def test_wide_windows(gpu_lib, c, cid):
    """real 17- and 20-bit windows (the two-level front without its knob): the shared cases and 2^12 pairs of each structured key"""
    _check(X.run_mode(gpu_lib, "plain", cid, widths=(c,), only=X.FEW))
    for key in ("all_g", "periodic"):
        _check(X.run_big(gpu_lib, X.wide_case(cid, c, key), c))


@pytest.mark.parametrize("key", ["all_g", "periodic"])
@pytest.mark.parametrize("cid,n,c", [(0, 1 << 17, 8), (1, 1 << 13, 5), (0, 20000, 4)])
def test_every_bucket_heavy(gpu_lib, cid, n, c, key):
    """the shapes of test_gpu_msm.py::test_every_bucket_heavy (4, 16 and 8 quads per sub-job) with every partial of a bucket the
    same point, or the partials of a bucket in equal and opposite groups"""
    _check(X.run_big(gpu_lib, X.big_case(f"heavy_{key}", cid, c, n, key, seed=n % 1000 + c), c))


def test_staged_sort_2p19(gpu_lib):
    _check(X.run_big(gpu_lib, X.big_case("staged_periodic", 1, 13, 1 << 19, "periodic", seed=19), 13, knobs=[(_lib.TUNE_STAGED_MIN_N, 1)]))


@pytest.mark.parametrize("cid", [0, 1])
def test_medium_runs_as_chains(gpu_lib, cid):
    _check(X.run_big(gpu_lib, X.medium_flood_case(cid), 8))
