"""The library's internal workspaces (tests/workspace_state.py) on the CPU emulation of the kernels.

Fresh, poisoned workspaces: a child process runs under glibc's MALLOC_PERTURB_ -- the emulation's device allocator is
aligned_alloc, so every workspace comes back filled with 0xA5 (huge indices, non-canonical elements) or with 0x01 (small,
plausible counts and indices) -- and behind a proxy that releases every workspace before every compute entry point.  Whatever a
call reads without having written it in the same call is fill, not the zero of a fresh page.  The child proves the fill active
before it runs anything; the variable is set for the child alone.

Stale workspaces: every route of the MSM table after every other on the session's one emulated library, the other workspaces
large then small then large, one interleaved schedule of all families, and the calls that follow a refusal.

Every comparison is byte for byte with the C oracle or Python integers."""
import json
import os
import subprocess
import sys

import pytest

import workspace_state as WS

HERE = os.path.dirname(os.path.abspath(__file__))
FILLS = (90, 254)                                       # MALLOC_PERTURB_ = 90 fills with 0xA5, 254 with 0x01
LARGE, SMALL = 4097, 1500
# the routes whose commit of 1500 pairs stays under half a second here: the full square runs over these
SQUARE = ["plain", "c5", "glv", "glv9", "shared12", "hostchunks"]
OTHERS = [name for name in WS.route_names() if name not in SQUARE]
HEAVY_A = "c4"                                          # eight buckets a window: every bucket heavy, every heavy-run list written


def spec(name, **kwargs):
    return name + (":" + json.dumps(kwargs, sort_keys=True) if kwargs else "")


def run_child(emu_lib, mode, *specs, fill=None, timeout=900):
    """python tests/workspace_state.py <emu lib> <mode> <specs>: exit status 0 and one `ok` line per spec; on a signal or a failure
    the case that was running is named"""
    env = dict(os.environ)
    env.pop("MALLOC_PERTURB_", None)
    if fill is not None:
        env["MALLOC_PERTURB_"] = str(fill)
    res = subprocess.run([sys.executable, os.path.join(HERE, "workspace_state.py"), emu_lib.path, mode, *specs], capture_output=True, text=True, timeout=timeout, env=env)
    lines = res.stdout.splitlines()
    if fill is not None:
        if res.returncode == 0 and lines and lines[0].startswith("skip:"):                 # the child skips only where the C library is not glibc
            pytest.skip(lines[0])
        assert f"fill {~fill & 0xFF:#04x} active" in lines, f"the child did not prove the fill (exit status {res.returncode})\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    done = [line for line in lines if line.startswith("ok ")]
    assert res.returncode == 0 and done == [f"ok {s}" for s in specs], \
        f"exit status {res.returncode} in case {specs[len(done)] if len(done) < len(specs) else '-'}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"


# ---- the tables themselves ------------------------------------------------------------------------------------------------------
def test_route_table():
    names = WS.route_names()
    for must in ("plain", "c5", "c13", "c16", "staged", "wide", "glv", "glv9", "shared12", "shared8", "hostchunks", "tables20", "batch_host", "batch_device",
                 "partial", "partial_to_device", "passes", "c4", "stats_plain", "stats_glv", "stats_shared"):
        assert must in names
    assert set(SQUARE) <= set(WS.route_names("fast")) and HEAVY_A in names and set(SQUARE) | set(OTHERS) == set(names)
    assert WS.ROUTE["shared8"].pre == (12, 8) and WS.ROUTE["c4"].width == 4 and WS.ROUTE["staged"].knobs["STAGED_MIN_N"] == 1
    from mira_amd import _lib
    assert all(hasattr(_lib, "TUNE_" + k) for r in WS.ROUTES for k in r.knobs)
    # statistics are collected only from MIRA_TUNE_PLAN_HIST_MIN_N pairs on (2^15 by default) and never under a forced width
    for name in ("planned", "stats_plain", "stats_glv", "stats_shared"):
        assert WS.ROUTE[name].knobs["PLAN_HIST_MIN_N"] == 1 and WS.ROUTE[name].width == 0 and WS.ROUTE[name].call == "device"


def test_schedule_is_fixed_and_draws_from_every_family():
    a, b = WS.schedule(LARGE, SMALL, SQUARE), WS.schedule(LARGE, SMALL, SQUARE)
    assert a == b and len(a) == 60
    assert sum(1 for family, _ in a if family == "msm") >= 10 and {kw["n"] for family, kw in a if family == "msm"} >= {LARGE, SMALL}


def test_the_proxy_trims_before_compute_calls_only():
    class Fake:
        def __init__(self):
            self.log = []

        def __getattr__(self, name):
            return lambda *args: self.log.append(name) or 0
    fake = Fake()
    c = WS.TrimFirst(fake)
    for name in ("mira_dev_alloc", "mira_set_tuning", "mira_msm_set_window_bits", "mira_last_error", "mira_msm_last_plan", "mira_set_timing", "mira_get_timings", "mira_trim"):
        getattr(c, name)()
    assert fake.log.count("mira_trim") == 1 and c.trims == 0
    fake.log.clear()
    for name in ("mira_msm_device", "mira_fft_bn256_fr", "mira_lookup_m_device", "mira_perm_check_device", "mira_msm_setup_bases"):
        getattr(c, name)()
    assert fake.log == [x for name in ("mira_msm_device", "mira_fft_bn256_fr", "mira_lookup_m_device", "mira_perm_check_device", "mira_msm_setup_bases")
                        for x in ("mira_trim", name)] and c.trims == 5


def test_a_child_without_the_fill_says_so(emu_lib):
    """MALLOC_PERTURB_ = 0 switches the fill off: the child must refuse to run, not pass"""
    import platform
    env = dict(os.environ, MALLOC_PERTURB_="0")
    res = subprocess.run([sys.executable, os.path.join(HERE, "workspace_state.py"), emu_lib.path, "poison", "is_sat_perm"], capture_output=True, text=True, timeout=300, env=env)
    if platform.libc_ver()[0] == "glibc":
        assert res.returncode != 0 and "the fill is not active" in res.stderr and "ok is_sat_perm" not in res.stdout, res.stdout + res.stderr


# ---- fresh, poisoned workspaces -------------------------------------------------------------------------------------------------
ROUTE_GROUPS = {"square": SQUARE, "narrow and planned": ["planned", "shared8", "passes", "c4"], "statistics": ["stats_plain", "stats_glv", "stats_shared"], "sorts": ["c13", "staged", "wide"],
                "entry points": ["batch_host", "batch_device", "partial", "partial_to_device"]}
assert sorted(sum(ROUTE_GROUPS.values(), []) + ["c16", "tables20"]) == sorted(WS.route_names())
# the routes that collect bit-length statistics run after `fresh`, after the heavy A and after one another (each B runs twice)
assert {"planned", "stats_plain", "stats_glv", "stats_shared"} <= set(OTHERS)


@pytest.mark.parametrize("group", list(ROUTE_GROUPS))
@pytest.mark.parametrize("fill", FILLS)
def test_poisoned_routes(emu_lib, fill, group):
    """the route table at 1500 pairs: both curves, the dense and the witness-like vector, the half-repeated one on one curve a route"""
    run_child(emu_lib, "poison", *[spec("routes", n=SMALL, routes=[name]) for name in ROUTE_GROUPS[group]], fill=fill)


@pytest.mark.parametrize("fill", FILLS)
def test_poisoned_widest_routes(emu_lib, fill):
    """16-bit windows (2^15 buckets a window, four to five seconds a commit here) once per curve; the 20-bit tables (one set of 2^19
    buckets) with the vectors of every other route"""
    run_child(emu_lib, "poison", spec("routes", n=SMALL, routes=["c16"], once=["c16"]), spec("routes", n=SMALL, routes=["tables20"]), fill=fill)


@pytest.mark.parametrize("field", WS.E.FIELDS)
@pytest.mark.parametrize("fill", FILLS)
def test_poisoned_field_kernels(emu_lib, fill, field):
    """the drivers of edge_operands.py as they are: fold, lincomb, the tree, the inversion and the lookup's h / g with small chunks,
    both groups of graphs"""
    run_child(emu_lib, "poison", spec("edge_fold_pairs", field=field), spec("edge_fold_targets", field=field), spec("edge_fold_lengths", field=field),
              spec("edge_lincomb", field=field), spec("edge_pow_tree", field=field), spec("edge_batch_invert", field=field, chunk=2),
              spec("edge_lookup_h_g", field=field, chunk=2), spec("edge_graph", field=field, group="gate"), spec("edge_graph", field=field, group="chain"), fill=fill)


@pytest.mark.parametrize("fill", FILLS)
def test_poisoned_ntt(emu_lib, fill):
    """2^5, 2^9 and 2^12 points with the forced kernels and line lengths of test_edge_operands_emu.py, all five operations"""
    ops = list(WS.E.NTT_OPS)
    run_child(emu_lib, "poison", spec("edge_ntt", k=5, wave=1, ops=ops, limit=2), spec("edge_ntt", k=5, wave=0, ops=ops, limit=2),
              spec("edge_ntt", k=9, wave=1, ops=ops, limit=2), spec("edge_ntt", k=9, wave=0, ops=ops, limit=2),
              spec("edge_ntt", k=12, max_log_line=12, ops=ops, limit=1, roundtrip=False),
              spec("edge_ntt", k=12, max_log_line=4, wave=1, ops=ops, limit=1), fill=fill)


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("fill", FILLS)
def test_poisoned_guarded_calls(emu_lib, fill, which):
    """the guarded drivers at their smallest lengths (`which`: the field, and the curve), the hash table forced by turns, key setup
    of 2^6 points in chunks of 24, is_sat_perm once"""
    run_child(emu_lib, "poison", spec("guarded_deciders", field=which, lengths=[1, 255, 257]),
              spec("guarded_lookup", field=which, shapes=[[1, 1], [65, 63], [257, 255]], hashes=[None, 1]),
              spec("guarded_pow_tree", field=which, sizes=[1, 6]), spec("guarded_generators", curve=which, lengths=[1, 63]),
              spec("guarded_msm_io", curve=which, lengths=[1, 63, 65], partial_planned=[]), spec("guarded_ntt_device", k=5 if which else 9),
              spec("setup", curve=which, k=6, chunk=24), spec("is_sat_perm", field=which), fill=fill)


# ---- stale workspaces -----------------------------------------------------------------------------------------------------------
# One child process runs every case below on one library and one set of keys (a planted fault of this kind ends the process with a
# segmentation fault as often as with a wrong point); each test then asks for the `ok` line of its own case.
PAIRS = dict(bs=SQUARE, large=LARGE, small=SMALL)
SLOWER = dict(bs=OTHERS, large=LARGE, small=SMALL, reverse=False)
STALE = {("pairs", a): spec("pairs", a=a, **PAIRS) for a in [WS.FRESH] + SQUARE}                    # (every B runs a second time)
STALE.update({("slower", a): spec("pairs", a=a, **SLOWER) for a in (WS.FRESH, HEAVY_A)})
STALE["ntt"] = spec("ntt_sequence")
for _field in WS.E.FIELDS:
    STALE.update({("lookup", _field): spec("lookup_sequence", field=_field), ("deciders", _field): spec("decider_sequence", field=_field),
                  ("pow_tree", _field): spec("pow_tree_sequence", field=_field), ("fold", _field): spec("fold_sequence", field=_field),
                  ("graph", _field): spec("graph_sequence", field=_field)})
STALE["schedule"] = spec("schedule", large=LARGE, small=SMALL, routes=SQUARE + [HEAVY_A, "passes", "batch_device", "partial"])
STALE["refusals"] = spec("refusals")


@pytest.fixture(scope="module")
def stale_child(emu_lib):
    specs = list(STALE.values())
    env = dict(os.environ)
    env.pop("MALLOC_PERTURB_", None)
    res = subprocess.run([sys.executable, os.path.join(HERE, "workspace_state.py"), emu_lib.path, "plain", *specs], capture_output=True, text=True, timeout=1800, env=env)
    sections, at = {}, None                                               # what the child printed between `run CASE` and the next one
    for line in res.stdout.splitlines():
        if line.startswith("run "):
            at = line[4:]
        sections.setdefault(at, []).append(line)
    return res, sections


def ran(stale_child, key):
    res, sections = stale_child
    case = STALE[key]
    lines = sections.get(case)
    if lines and f"ok {case}" in lines:
        return
    if lines and f"failed {case}" in lines:
        pytest.fail("\n".join(lines)[-4000:], pytrace=False)
    if lines:                                                              # it began and neither passed nor raised: the process ended in it
        pytest.fail(f"exit status {res.returncode} in case {case}\n" + "\n".join(lines)[-2000:] + "\n" + res.stderr[-4000:], pytrace=False)
    last = [c for c in sections if c][-1] if any(sections) else None
    pytest.fail(f"not reached: the child ended with exit status {res.returncode} in the earlier case {last}\n{res.stderr[-1500:]}", pytrace=False)


@pytest.mark.parametrize("a", [WS.FRESH] + SQUARE)
def test_route_b_after_a(stale_child, a):
    """the full square over the quick routes: A at 4097 pairs, B at 1500 -- on the other curve for half of the pairs, always with another
    kind of vector --, and B again; then small A and large B"""
    ran(stale_child, ("pairs", a))


@pytest.mark.parametrize("a", [WS.FRESH, HEAVY_A])
def test_slower_route_b_after_a(stale_child, a):
    """the slower routes after `fresh` (buffers of exactly their own size) and after an A whose every bucket is heavy"""
    ran(stale_child, ("slower", a))


def test_ntt_sequence(stale_child):
    ran(stale_child, "ntt")


@pytest.mark.parametrize("family", ["lookup", "deciders", "pow_tree", "fold", "graph"])
@pytest.mark.parametrize("field", WS.E.FIELDS)
def test_family_sequence(stale_child, field, family):
    """large, small, large through the lookup's hash table and the inversion, the deciders (is_sat_perm with two compiled matrices by
    turns), the weighted tree, the folds and the graph engines at two row counts"""
    ran(stale_child, (family, field))


def test_interleaved_schedule(stale_child):
    ran(stale_child, "schedule")


def test_calls_after_a_refusal(stale_child):
    ran(stale_child, "refusals")
