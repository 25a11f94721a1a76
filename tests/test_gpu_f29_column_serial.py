"""The column-serial multipliers of field29.cuh on the device.  tests/gpu/f29_forms.hip is a stand-alone program: 4 096 lanes
apply the device forms (the only build in which the multiply-add chain is pinned with inline asm) and the in-place reference
to the operands of tests/emu/f29_operands.h, for both fields, and it prints how many limbs differ -- the one place where the
asm path is compared limb by limb.  Then the same code through the library: a commit per curve under 16-bit and 13-bit
windows whose scalars include the edge values of the signed-digit and GLV splits, against the oracle, and an NTT round trip."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

from helpers import glv_edge_scalars, scalar_field_id
from mira_amd import commitment as cm
from mira_amd import fft as F
from oracle import cref as C
from oracle import pyref as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 13


@pytest.fixture(scope="module")
def forms_exe(gpu_lib, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("f29_forms") / "f29_forms")
    subprocess.check_call([os.environ.get("HIPCC", "hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950",
                           os.path.join(ROOT, "tests", "gpu", "f29_forms.hip"), "-o", exe])
    return exe


def test_device_forms_limb_by_limb(forms_exe):
    res = subprocess.run([forms_exe], capture_output=True, text=True, timeout=60)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert [ln.split(":")[0] for ln in lines] == ["Fq29", "Fr29"], res.stdout
    for ln in lines:
        m = re.fullmatch(r"F[qr]29: (\d+) calls, (\d+) limbs differ \(device reference\), (\d+) limbs differ \(host reference\), column-serial (\d)", ln)
        assert m, ln
        calls, dev, host, form = (int(x) for x in m.groups())
        assert calls > 10000 and dev == 0 and host == 0, ln
        assert form == 1, "the library's default form is the column-serial one"


def edge_scalars(cid, c):
    """canonical scalars: the GLV edge list, and per window one digit of the signed-digit boundary list at widths c"""
    r = P.CURVES[cid].r
    rng = random.Random(0xF29 + cid + c)
    digits = [0, 1, 2, (1 << (c - 1)) - 1, 1 << (c - 1), (1 << c) - 2, (1 << c) - 1]
    out = glv_edge_scalars(r) + [r - 3, (r - 1) // 2, (r + 1) // 2]
    out += [sum(rng.choice(digits) << (c * w) for w in range(252 // c)) for _ in range(64)]
    out += [sum(d << (c * w) for w in range(252 // c)) for d in digits]
    assert all(0 <= s < r for s in out)
    return out


@pytest.fixture(scope="module")
def commit_case():
    """per curve: bases, scalars (random, with the edge values of both widths spread over the vector) and the oracle's point"""
    out = {}
    for cid in (0, 1):
        bases = C.synth_bases(cid, N, seed=0x2900 + cid)
        sc = C.synth_scalars(cid, N, seed=0x2910 + cid).copy()
        edge = edge_scalars(cid, 16) + edge_scalars(cid, 13)
        rows = C.to_mont(scalar_field_id(cid), np.array([P.limbs4(s) for s in edge], dtype=np.uint64).reshape(-1, 4))
        where = random.Random(0x2920 + cid).sample(range(N), len(edge))
        sc[where] = rows
        out[cid] = (bases, sc, C.commit(cid, bases, sc))
    return out


@pytest.mark.parametrize("c", [16, 13])
@pytest.mark.parametrize("cid", [0, 1])
def test_commit_against_oracle(gpu_lib, commit_case, cid, c):
    bases, sc, want = commit_case[cid]
    key = cm.CommitmentKey(cid, bases, lib=gpu_lib)
    try:
        key.set_window_bits(c)
        assert (key.commit(sc) == want).all()
    finally:
        key.close()


def test_ntt_round_trip(gpu_lib):
    a = C.synth_scalars(0, 1 << 12, seed=0x2930)
    spec = F.fft(a, 12)
    assert (spec == C.fft(a, 12)).all()
    assert (F.ifft(spec, 12) == a).all()
