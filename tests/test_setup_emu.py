"""CommitmentKey::setup by hash-to-curve (src/commitment.rs:52-76; csrc/setup_kernels.cuh, csrc/setup.hip) on the CPU
emulation of the kernel sources, against the plain-Python restatement tests/setup_ref.py -- and the restatement against the
checksums recorded for it.  Parity: equal to the restatement and those checksums, unpinned against halo2curves."""
import os
import subprocess

import pytest

import setup_cases as SC
import setup_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 6


@pytest.fixture(scope="module")
def lib(emu_lib):
    return emu_lib


# ---- the restatement itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,k,label", sorted(R.CHECKSUMS))
def test_restatement_reproduces_the_checksums(curve, k, label):
    key = R.key_bytes(curve, k, label)
    assert len(key) == 64 << k and SC.sha256(key) == R.CHECKSUMS[(curve, k, label)]
    assert all(R.on_curve(P, curve) for P in SC.points_of(key, curve))


def test_restatement_first_point():
    assert R.setup_points(0, b"", 0, 1)[0] == R.FIRST_POINT_BN256_EMPTY


@pytest.mark.parametrize("curve", SC.CURVES)
def test_find_z_svdw_is_one(curve):
    assert R.find_z_svdw(curve) == 1


def test_restatement_constants():
    assert R.svdw_constants(0)[1] == 4
    assert R.svdw_constants(0)[3] == 0x16789af3a83522eb353c98fc6b36d713d5d8d1cc5dffffffa
    assert R.svdw_constants(1)[3] == 0x2cf135e7506a45d66a7931f8d66dae274453478a4c627115c


def test_restatement_takes_all_three_branches():
    for curve in SC.CURVES:
        branches = [b for m in R.messages(b"mira setup test", 0, 64) for u in R.hash_to_field(m, curve) for b in [R.map_to_curve(u, curve)[1]]]
        assert set(branches) == {1, 2, 3}


# ---- the library ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", SC.LABELS)
@pytest.mark.parametrize("curve", SC.CURVES)
def test_setup_bases_equal_the_restatement(lib, curve, label):
    SC.check_key(lib, curve, K, label, -1)


@pytest.mark.parametrize("curve", SC.CURVES)
def test_chunk_boundaries_inside_a_sponge_block(lib, curve):
    # 24 points = 768 bytes = 5 blocks of 136 and 88 bytes: every chunk but the first starts inside a block
    SC.check_key(lib, curve, K, SC.LABELS[1], 24)


@pytest.mark.parametrize("curve", SC.CURVES)
def test_a_range_equals_the_slice(lib, curve):
    SC.check_range(lib, curve, K, SC.LABELS[1], 24)
    assert SC.setup_bytes(lib, curve, SC.LABELS[1], 9, 0) == b""


@pytest.mark.parametrize("curve", SC.CURVES)
def test_hash_to_field(lib, curve):
    SC.check_hash_to_field(lib, curve, 64)


@pytest.mark.parametrize("curve", SC.CURVES)
def test_map_to_curve_exceptional_inputs(lib, curve):
    SC.check_map_chosen(lib, curve)


@pytest.mark.parametrize("curve", SC.CURVES)
def test_map_to_curve_random_pairs_take_every_branch(lib, curve):
    SC.check_map_random(lib, curve)


def test_k_32_is_refused(lib):
    SC.check_k32_refused(lib)


def test_chunk_knob_is_bounded(lib):
    from mira_amd import _lib
    for value in (0, 15, (1 << 24) + 1):
        with pytest.raises(_lib.MiraError) as err:
            lib.tune(_lib.TUNE_SETUP_CHUNK, value)
        assert err.value.code == _lib.MIRA_E_BAD_ARG
    lib.tune(_lib.TUNE_SETUP_CHUNK, 16)
    lib.tune(_lib.TUNE_SETUP_CHUNK, -1)


def test_registered_key_is_the_same_key(lib):
    """mira_msm_setup_bases writes the resident layout directly: downloaded, it is the key of mira_setup_bases_device"""
    from mira_amd import commitment as cm
    for curve in SC.CURVES:
        key = cm.CommitmentKey.setup(curve, 4, SC.LABELS[1], lib=lib)
        assert len(key) == 16 and key.bases().tobytes() == R.key_bytes(curve, K, SC.LABELS[1])[:16 * 64]
        key.check_on_curve()
        key.close()


# ---- the 512-bit reduction, as a host program (plain and under the address and undefined-behaviour sanitizers) -----------------
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_reduce512_against_long_division(flags, tmp_path):
    exe = str(tmp_path / "test_setup_reduce")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-pthread", *flags, "-x", "c++", os.path.join(ROOT, "tests", "emu", "test_setup_reduce.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and all(line in res.stdout.splitlines() for line in ["Fq29: ok", "Fr29: ok"]), res.stdout + res.stderr
