"""Guard bands (tests/guarded.py) around every device-resident call of the CPU emulation of the kernels: every operand of a
call lies inside one allocation between 64 KiB bands of unique, non-canonical guard elements, at byte offsets 0, 32 and 96 from
a 256-byte boundary.  Every call must give exact values (Python integers, the C oracle), leave both bands of every operand
untouched and leave its inputs alone.  On the emulation a stray store lands in host heap nobody looks at afterwards, exactly as
it lands in allocator slack on the device.

The arena itself is tested first, on a library that does nothing but copy: it must see a changed guard byte on either side of
an operand and a changed input, and name them."""
import numpy as np
import pytest

import edge_operands as E
import guarded as GD


# ---- the arena ------------------------------------------------------------------------------------------------------------------
def test_guard_elements_are_unique_and_non_canonical():
    g = GD.guard_fill(5, 4096)
    vals = E.from_array(g)
    assert len(set(vals)) == len(vals) and all(v >= 1 << 255 for v in vals) and (g[:, 3] == np.uint64(GD.ALL_ONES)).all()
    assert [int(x) for x in g[:, 0]] == list(range(5, 5 + 4096))
    assert all(v > max(E.MODULUS[f] for f in E.FIELDS) for v in vals[:8])


def test_arena_layout(emu_lib):
    with GD.Arena(emu_lib) as A:
        ops = [A.place(np.arange(n * 4, dtype=np.uint64), off) for n, off in ((1, 0), (65, 1), (7, 3))] + [A.place(5, 1), A.place(np.zeros(33, np.uint8), 3)]
        assert [(op.ptr - off * 32) % 256 for op, off in zip(ops, (0, 1, 3, 1, 3))] == [0] * 5
        assert ops[0].start >= A.guard and all(b.lo - a.hi >= A.guard * 32 for a, b in zip(ops, ops[1:]))
        assert A.image.nbytes - ops[-1].hi >= A.guard * 32
        assert A.check("nothing ran") == []
        assert (GD.elems(A.check("nothing ran", [ops[3]])[0]) == GD.guard_fill(ops[3].start, 5)).all()      # an output starts as guard fill


@pytest.mark.parametrize("where,expect", [(lambda op: op.hi, "guard after operand 'b' changed at byte +0 past its end"),
                                          (lambda op: op.hi + 32 * 1000 + 31, "guard after operand 'b' changed at byte +32031 past its end (element +1000)"),
                                          (lambda op: op.lo - 1, "guard before operand 'b' changed at byte -1 before its start"),
                                          (lambda op: op.lo + 40, "operand 'b' (not an output of this call) changed at byte 40 of 2080")])
def test_arena_names_what_changed(emu_lib, where, expect):
    with GD.Arena(emu_lib) as A:
        A.place(np.ones((3, 4), dtype=np.uint64), 0, "a")
        b, c = A.place(np.ones((65, 4), dtype=np.uint64), 3, "b"), A.place(9, 1, "c")
        A.check("untouched")
        at = where(b)
        emu_lib.upload(A.origin + at, np.array([A.image[at] ^ 0x10], dtype=np.uint8))
        with pytest.raises(AssertionError) as err:
            A.check("poke", [c])
        assert "poke: " + expect in str(err.value)


def test_arena_names_a_read_of_guard_fill(emu_lib):
    """the deciders refuse a non-canonical element: a sweep that takes in one guard element says so, and the driver names the call"""
    from mira_amd import decider as DC
    with GD.Arena(emu_lib) as A:
        a = A.place(np.ones((5, 4), dtype=np.uint64), 1, "a")
        with A.reading("count_ne n=5"):
            assert DC.count_ne_device(0, a.ptr, None, 5, lib=emu_lib) == (5, 0)
        with pytest.raises(AssertionError, match="count_ne n=5 \\+ 1: read outside its operands"):
            with A.reading("count_ne n=5 + 1"):
                DC.count_ne_device(0, a.ptr, None, 6, lib=emu_lib)


# ---- the drivers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", E.FIELDS)
def test_fold(emu_lib, field):
    GD.check_fold(emu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_lincomb(emu_lib, field):
    GD.check_lincomb(emu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_batch_invert(emu_lib, field):
    GD.check_batch_invert(emu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_lookup(emu_lib, field):
    GD.check_lookup(emu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_deciders(emu_lib, field):
    GD.check_deciders(emu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_pow_tree(emu_lib, field):
    GD.check_pow_tree(emu_lib, field)


@pytest.mark.parametrize("field", E.FIELDS)
def test_graph(emu_lib, field):
    GD.check_graph(emu_lib, field)


@pytest.mark.parametrize("curve", [0, 1])
def test_generators(emu_lib, curve):
    GD.check_generators(emu_lib, curve)


@pytest.mark.parametrize("curve", [0, 1])
def test_msm_io(emu_lib, curve):
    """Two departures from the lengths of the device run, both for time: 2^12 + 1 pairs stand in for 2^13 + 1 (13 s a width on the
    emulation against 9 s; both lie past 2^12, from where a commit may take a key's tables and runs its width trials), and
    mira_msm_partial_to_device runs at the planner's width at one length and offset only -- a partial's default width is 16 bits
    whatever n, so that no shorter length makes it cheaper, five seconds a call here; at 9 bits it runs at every length and offset.
    The planned-width partial at the other lengths and offsets is covered by the device run alone (tests/test_gpu_guarded.py runs
    every case of the table)."""
    GD.check_msm_io(emu_lib, curve, lengths=(1, 63, 65, 1025, 4097), partial_planned={(65, 1)})


def test_copy(emu_lib):
    GD.check_copy(emu_lib)


# ---- the device-resident transforms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(10))
def test_ntt_device(emu_lib, k):
    GD.check_ntt_device(emu_lib, k)


@pytest.mark.parametrize("wave", [1, 0])
@pytest.mark.parametrize("max_line,ks", [(3, (4, 5, 6, 7, 8, 9)), (4, (9, 11)), (2, (5, 6))])
def test_ntt_device_pass_schedules(emu_lib, max_line, ks, wave):
    """the two- and three-pass schedules of test_emu_kernels.py's test_emu_ntt_pass_schedules, on both kernels"""
    for k in ks:
        GD.check_ntt_device(emu_lib, k, wave=wave, max_log_line=max_line)


@pytest.mark.parametrize("wave", [1, 0])
def test_ntt_device_full_twiddle_table(emu_lib, wave):
    """SINGLE_TW_LOG = 3 beside MAX_LOG_LINE = 3, as in test_emu_kernels.py's test_emu_ntt_full_twiddle_table: a transform of one
    pass builds no post-twiddle table at all, so the lines are cut to 8 points -- 2^5 points take two passes, 2^8 and 2^9 three.
    The exponent range of the first boundary is log_n bits (ntt_prepare_tables: range[0]), more than the 3 of the knob at every
    one of these sizes: the first post-twiddle comes from the table of n entries.  The second boundary of 2^8 and 2^9 points has a
    range of 5 and 6 bits, again more than 3: the product of two table entries."""
    for k in (5, 8, 9):
        GD.check_ntt_device(emu_lib, k, wave=wave, max_log_line=3, single_tw_log=3)


@pytest.mark.parametrize("k,max_line", [(5, None), (8, 3)])
def test_ntt_other_primitive_roots(emu_lib, k, max_line):
    GD.check_ntt_roots(emu_lib, k, max_log_line=max_line)
