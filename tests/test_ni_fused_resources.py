"""The one-kernel Behler route (ANNP_HIP_NI_EVAL=fused, meng_zhang_amd/csrc/ni_fused_kernels.hpp) as the compiler reports it
(`make asm`, no GPU needed): every instantiation the driver can launch exists, none spills, and the steady-state one of an MD run
(shipped shape, record capacity compiled in, no virial tally) keeps three waves per SIMD."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SHIPPED = "annp::annp_ni_fused<3, 24, 2, 3, 4, 268698113u, 328193u, "
GENERIC = "annp::annp_ni_fused<8, 32, 0, 0, 0, 0u, 0u, "


@pytest.fixture(scope="module")
def kernels():
    import kernel_resources
    return {k["kernel"]: k for k in kernel_resources.collect()}


def test_every_instantiation_the_driver_launches_is_there(kernels):
    for virial in ("false", "true"):
        for tail in ("false, 20>", "false, 0>", "true, 0>"):         # FIX, CAP
            assert SHIPPED + "%s, %s" % (virial, tail) in kernels
        for tail in ("false, 0>", "true, 0>"):
            assert GENERIC + "%s, %s" % (virial, tail) in kernels


def test_no_fused_kernel_spills(kernels):
    fused = {n: k for n, k in kernels.items() if n.startswith("annp::annp_ni_fused<")}
    assert len(fused) == 10
    bad = {n: (k["scratch"], k["vgpr_spill"]) for n, k in fused.items() if k["scratch"] or k["vgpr_spill"]}
    assert not bad, bad


def test_steady_state_keeps_three_waves_per_simd(kernels):
    k = kernels[SHIPPED + "false, false, 20>"]
    assert k["vgpr"] <= 168 and k["occupancy"] >= 3, k
    # with the virial tally the compiler is given 2 waves per SIMD (at 3 it spills: the header says so); still no scratch
    k = kernels[SHIPPED + "true, false, 20>"]
    assert k["vgpr"] <= 256 and k["occupancy"] >= 2 and k["scratch"] == 0, k


def test_lds_of_the_steady_state_leaves_room_for_three_workgroups():
    """the sizing helper is constexpr and the header asserts the bound at compile time; the same formula here, so that the number
    DESIGN.md quotes (54 016 bytes at capacity 20) is the header's"""
    src = open(os.path.join(ROOT, "meng_zhang_amd", "csrc", "ni_fused_kernels.hpp")).read()
    assert re.search(r"static_assert\(ni_fused_lds_block\(NI_CAP_FIXED, false\) <= 53 \* 1024", src)
    cap, ga, cstride, tslots, waves = 20, 4, 34, 128, 4
    r = ga * cap + 2
    plist = (cap * (cap - 1) // 2 + 7) // 8 * 8
    per_wave = r * 10 * 8 + ga * cstride * 8 + tslots * 28 + r * 8 + 2 * ga * 4 + ga * plist * 2 + ga * 4 + ga * 8
    per_wave = (per_wave + 15) // 16 * 16
    assert per_wave == 13504 and per_wave * waves <= 53 * 1024
    assert 3 * per_wave * waves <= 160 * 1024
