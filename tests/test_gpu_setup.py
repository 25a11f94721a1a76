"""CommitmentKey::setup by hash-to-curve on the device (k_setup_hash, k_setup_map; src/commitment.rs:52-76) against the
plain-Python restatement tests/setup_ref.py: the cases of tests/test_setup_emu.py at k = 10 with chunks of 192 points (24
sponge blocks: 5 1/3 chunks, several workgroups each and a ragged last one), then the key through commit, the cache file
and one larger key checked by its properties.  Parity: the restatement and its checksums, unpinned against halo2curves."""
import os

import numpy as np
import pytest

import setup_cases as SC
import setup_ref as R

pytestmark = pytest.mark.gpu
K = 10
CHUNK = 192
LABEL = SC.LABELS[1]


@pytest.mark.parametrize("label", SC.LABELS)
@pytest.mark.parametrize("curve", SC.CURVES)
def test_setup_bases_equal_the_restatement(gpu_lib, curve, label):
    SC.check_key(gpu_lib, curve, K, label, CHUNK)


@pytest.mark.parametrize("curve", SC.CURVES)
def test_default_chunk_gives_the_same_key(gpu_lib, curve):
    SC.check_key(gpu_lib, curve, K, LABEL, -1)


@pytest.mark.parametrize("curve", SC.CURVES)
def test_a_range_equals_the_slice(gpu_lib, curve):
    SC.check_range(gpu_lib, curve, K, LABEL, CHUNK)
    SC.check_range(gpu_lib, curve, K, LABEL, CHUNK, first=771, n=253)          # to the key's end, from inside a chunk


@pytest.mark.parametrize("curve", SC.CURVES)
def test_hash_to_field(gpu_lib, curve):
    SC.check_hash_to_field(gpu_lib, curve, 64)
    SC.check_hash_to_field(gpu_lib, curve, 193)                                # four workgroups, the last with one lane


@pytest.mark.parametrize("curve", SC.CURVES)
def test_map_to_curve_exceptional_inputs(gpu_lib, curve):
    SC.check_map_chosen(gpu_lib, curve)


@pytest.mark.parametrize("curve", SC.CURVES)
def test_map_to_curve_random_pairs_take_every_branch(gpu_lib, curve):
    SC.check_map_random(gpu_lib, curve)


def test_k_32_is_refused(gpu_lib):
    SC.check_k32_refused(gpu_lib)
    from mira_amd import commitment as cm
    with pytest.raises(ValueError):
        cm.CommitmentKey.setup(0, 32, LABEL)


@pytest.mark.parametrize("curve", SC.CURVES)
def test_commit_over_a_setup_key(gpu_lib, curve):
    from mira_amd import commitment as cm
    from oracle import cref as C
    key = cm.CommitmentKey.setup(curve, K, LABEL)
    bases = np.frombuffer(R.key_bytes(curve, K, LABEL), dtype=np.uint64).reshape(-1, 8)
    assert (key.bases() == bases).all()
    sc = C.synth_scalars(curve, 1 << K, kind=curve)
    assert (key.commit(sc) == C.commit(curve, bases, sc)).all()
    key.close()


@pytest.mark.parametrize("curve", SC.CURVES)
def test_save_and_load_round_trip(gpu_lib, curve, tmp_path):
    from mira_amd import commitment as cm
    key = cm.CommitmentKey.setup(curve, K, LABEL)
    path = tmp_path / "key.bin"
    key.save_to_file(path)
    assert path.read_bytes() == R.key_bytes(curve, K, LABEL)
    back = cm.CommitmentKey.load_from_file(curve, path, K, validate=True)
    assert (back.bases() == key.bases()).all()
    key.close()
    back.close()


@pytest.mark.parametrize("curve", SC.CURVES)
def test_load_or_setup_cache_with_the_hash_generator(gpu_lib, curve, tmp_path):
    from mira_amd import commitment as cm
    label = LABEL.decode()
    key = cm.CommitmentKey.load_or_setup_cache(curve, str(tmp_path), label, K, generator="hash")
    path = os.path.join(str(tmp_path), label, f"{K}.bin")
    with open(path, "rb") as f:
        assert SC.sha256(f.read()) == R.CHECKSUMS[(curve, K, LABEL)]
    again = cm.CommitmentKey.load_or_setup_cache(curve, str(tmp_path), label, K, generator="hash")      # now loaded and validated
    assert (again.bases() == key.bases()).all()
    with pytest.raises(ValueError):
        cm.CommitmentKey.load_or_setup_cache(curve, str(tmp_path), label, K, generator="other")
    key.close()
    again.close()


def test_larger_key_by_its_properties(gpu_lib):
    """k = 16 on Grumpkin with the default chunk: on the curve, no x-coordinate twice, and its first 2^10 points are the k = 10 key"""
    from mira_amd import commitment as cm
    key = cm.CommitmentKey.setup(1, 16, LABEL)
    key.check_on_curve()
    bases = key.bases()
    assert len(np.unique(bases[:, :4], axis=0)) == 1 << 16
    assert bases[:1 << K].tobytes() == R.key_bytes(1, K, LABEL)
    key.close()
