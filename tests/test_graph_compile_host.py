"""The cross-term graph compiler (mira_amd/csrc/graph_compile.hip) on the host, on its own: tests/emu/test_graph_compile.cpp, built
by the system C++ compiler and run as a child process, compiles a fixed set of flattened graphs -- random and gate-like
expressions, the cross-term evaluators of the MainGate fold step, hand-written edge cases and malformed code -- and prints
what came out: error and message, or instruction and slot counts, the columns read, the constant pool and challenge forms,
the instruction stream (a hash of it for long graphs) and hashes of the kernel source graph_jit.hpp writes for it.  The
output must match tests/golden/graph_compile.txt line for line.  After a deliberate change of a compiler rule, regenerate
that file from the program's output and review its diff."""
import os
import random
import subprocess

from graph_cases import gate_like_expression, random_expression
from harness import graph_evaluator as G
from harness import main_gate as MG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, I, COL, CH = G.SRC_CONSTANT, G.SRC_INTERMEDIATE, G.SRC_COLUMN, G.SRC_CHALLENGE


def _words(calcs):
    words = []
    for op, srcs in calcs:
        words.append(op | ((len(srcs) - 2) << 8 if op == G.OP_HORNER else 0))
        words += [(k << 29) | p for k, p in srcs]
    return words


def _col(c, rot=0):
    return (COL, c | rot << 20)


def _hand_cases():
    """(name, field, code words, calculations, constants, challenges, columns, rotations)"""
    A, S, M, SQ, D, N, H, ST = G.OP_ADD, G.OP_SUB, G.OP_MUL, G.OP_SQUARE, G.OP_DOUBLE, G.OP_NEGATE, G.OP_HORNER, G.OP_STORE
    out = []

    def case(name, calcs, nconst=3, nchal=2, ncols=8, rots=(0,), field=G.FIELD_FR, words=None, ncalc=None):
        out.append((name, field, _words(calcs) if words is None else words, len(calcs) if ncalc is None else ncalc, nconst, nchal, ncols, list(rots)))

    case("empty", [], nconst=0, nchal=0, ncols=0, rots=())
    case("lone_store_constant", [(ST, [(C, 1)])])
    case("lone_store_challenge", [(ST, [(CH, 1)])])
    case("stores_read_at_uses", [(ST, [(C, 0)]), (ST, [(CH, 0)]), (M, [(I, 0), _col(0)]), (A, [(I, 2), (I, 1)]), (M, [(I, 3), (I, 0)])])
    case("mul_read_twice", [(M, [_col(0), _col(1)]), (A, [(I, 0), _col(2)]), (A, [(I, 1), (I, 0)])])
    case("mul_operand_forwarded", [(A, [_col(0), _col(1)]), (M, [(I, 0), _col(2)]), (A, [(I, 1), _col(3)])])
    case("mac_chain", [(M, [(C, 0), _col(0)]), (M, [(C, 1), _col(1)]), (A, [(I, 0), (I, 1)]), (M, [(CH, 0), _col(2)]), (A, [(I, 2), (I, 3)]),
                       (M, [_col(3), _col(4)]), (A, [(I, 5), (I, 4)])])
    case("mac_free_addend", [(M, [_col(0), _col(1)]), (A, [(C, 2), (I, 0)]), (M, [(CH, 1), (C, 0)]), (A, [(I, 2), (I, 1)])])
    sums = [(A, [_col(0), _col(1)]), (A, [(I, 0), (I, 0)]), (A, [(I, 1), (I, 1)])]        # bounds 2, 4, 8 P
    case("sub_bias", sums + [(S, [_col(2), _col(0)]), (S, [_col(2), (I, 0)]), (S, [_col(3), (I, 1)]), (S, [_col(4), (I, 2)]),
                             (A, [(I, 3), (I, 4)]), (A, [(I, 7), (I, 5)]), (A, [(I, 8), (I, 6)])])
    case("neg_bias", sums + [(N, [_col(2)]), (N, [(I, 0)]), (N, [(I, 1)]), (N, [(I, 2)]), (N, [(C, 1)]),
                             (A, [(I, 3), (I, 4)]), (A, [(I, 8), (I, 5)]), (A, [(I, 9), (I, 6)]), (A, [(I, 10), (I, 7)])])
    case("square_double_forms", [(SQ, [_col(0)]), (SQ, [(CH, 0)]), (M, [(I, 0), (I, 1)]), (D, [(I, 2)]), (SQ, [(I, 3)]), (A, [(I, 4), _col(1)]),
                                 (D, [(C, 2)]), (M, [(I, 5), (I, 6)])])
    case("rotations", [(M, [_col(0, 1), _col(1, 2)]), (A, [(I, 0), _col(2, 3)]), (M, [(I, 1), _col(0, 0)]), (S, [(I, 2), _col(3, 1)])],
         rots=(0, 1, -1, 5))
    case("horner", [(A, [_col(0), _col(1)]), (H, [(I, 0), (CH, 0), _col(2), (C, 0), _col(3, 1)]), (H, [(C, 1), (I, 1), (CH, 1), _col(4)])],
         rots=(0, -2))
    case("shared_subexpression_two_forms", [(M, [(CH, 0), _col(0)]), (M, [(I, 0), _col(1)]), (A, [(I, 0), _col(2)]), (M, [(I, 1), (I, 2)])])
    case("fq_field", [(M, [_col(0), (C, 0)]), (S, [(I, 0), (CH, 1)])], field=G.FIELD_FQ)
    # malformed code: every message of the validation
    case("err_ends_inside_head", [(ST, [(C, 0)])], ncalc=2)
    case("err_ends_inside_operands", [], words=[A, (COL << 29)], ncalc=1)
    case("err_unknown_op", [], words=[9, 0], ncalc=1)
    case("err_internal_op", [], words=[0xFE, 0, 0, 0], ncalc=1)
    case("err_nparts_on_add", [], words=[A | 1 << 8, 0, 0], ncalc=1)
    case("err_constant_index", [(ST, [(C, 3)])])
    case("err_intermediate_early", [(ST, [(I, 0)])])
    case("err_challenge_index", [(ST, [(CH, 2)])])
    case("err_column_index", [(ST, [_col(8)])])
    case("err_rotation_index", [(ST, [_col(0, 1)])])
    case("err_source_kind", [(ST, [(4, 0)])])
    case("err_trailing", [], words=_words([(ST, [(C, 0)])]) + [0], ncalc=1)
    return out


def _expression_cases():
    out = []
    for seed, depth in [(1, 1), (2, 2), (3, 3), (4, 3), (5, 4), (6, 4), (7, 5), (8, 5), (9, 6), (10, 7)]:
        rng = random.Random(1000 + seed)
        field = seed % 2
        ev = G.GraphEvaluator.new(random_expression(rng, depth, 12, 3), field)
        out.append((f"random_s{seed}_d{depth}", field, ev, 3, 12))
    for seed, nterms, depth in [(5, 6, 7), (11, 4, 6), (12, 8, 5)]:
        rng = random.Random(seed)
        ev = G.GraphEvaluator.new(gate_like_expression(rng, nterms, depth, 12, 3), seed % 2)
        out.append((f"gate_s{seed}_t{nterms}_d{depth}", seed % 2, ev, 3, 12))
    for gates in (1, 2):
        cg, ctx = MG.compressed_circuit(5, gates)
        for field in (G.FIELD_FQ, G.FIELD_FR):
            plan = G.CrossTermPlan.from_compressed_gates(cg, ctx, field)
            ncols = ctx.num_selectors + ctx.num_fixed + 2 * ctx.num_advice
            for k, ev in enumerate(plan.evaluators):
                out.append((f"main_gate_g{gates}_f{field}_point{k}", field, ev, 2 * ctx.num_challenges, ncols))
    return out


def write_cases(path):
    """One graph per line: name field calculations constants challenges columns, the rotations, the code words (counted)."""
    lines = []
    for name, field, words, ncalc, nconst, nchal, ncols, rots in _hand_cases():
        lines.append(" ".join(str(v) for v in [name, field, ncalc, nconst, nchal, ncols, len(rots), *rots, len(words), *words]))
    for name, field, ev, nchal, ncols in _expression_cases():
        code, consts, rots = ev.flatten()
        lines.append(" ".join(str(int(v)) if not isinstance(v, str) else v
                              for v in [name, field, len(ev.calculations), len(consts), nchal, ncols, len(rots), *rots, len(code), *code]))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def test_compiled_graphs_are_pinned(tmp_path):
    cases, exe = str(tmp_path / "graphs.txt"), str(tmp_path / "test_graph_compile")
    write_cases(cases)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DMIRA_CPU_EMU", "-x", "c++",
                           os.path.join(ROOT, "tests", "emu", "test_graph_compile.cpp"), os.path.join(ROOT, "mira_amd", "csrc", "graph_compile.hip"),
                           "-o", exe])
    res = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    with open(os.path.join(ROOT, "tests", "golden", "graph_compile.txt")) as f:
        want = f.read().splitlines()
    got = res.stdout.splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}:\n  got  {g}\n  want {w}"
    assert len(got) == len(want), f"{len(got)} lines, want {len(want)}"
