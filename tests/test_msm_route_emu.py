"""The route every MSM entry point takes, as the C ABI shows it (tests/msm_route_trace.py), on the test-only host emulation of
the kernel sources: the library must answer the fixed list of calls as tests/golden/msm_route_trace.txt records it -- return
codes and error texts, mira_msm_last_plan, mira_msm_last_table_bits, the shape of every partial, and the oracle's point.  That
file was recorded on the library as it was before the routing moved from capi.hip into msm_route.hip."""
import msm_route_trace


def test_routes_through_the_abi_are_the_recorded_ones(emu_lib):
    msm_route_trace.assert_same_lines(msm_route_trace.run(emu_lib), msm_route_trace.golden_lines())
