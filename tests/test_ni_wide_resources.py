"""The wide Behler route's kernels (meng_zhang_amd/csrc/ni_wide_kernels.hpp, grade_kernels.hpp) as the compiler reports them (`make asm`,
no GPU needed): they exist, none uses scratch, their static LDS leaves room for two or more workgroups per CU -- and the kernels that
were there before report what profiles/r06_kernel_resources.json recorded (registers, scratch) for the tuned Behler passes and the
twelve network-pass instantiations."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
WIDE = ["annp::annp_niw_desc", "annp::annp_niw_force<false>", "annp::annp_niw_force<true>", "annp::annp_mlp_wide", "annp::annp_desc_grade_wide"]


@pytest.fixture(scope="module")
def kernels():
    import kernel_resources
    return {k["kernel"]: k for k in kernel_resources.collect()}


def test_wide_kernels_exist_without_scratch(kernels):
    for name in WIDE:
        assert name in kernels, name
        k = kernels[name]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0, (name, k)
        assert k["occupancy"] >= 2, (name, k)


def test_wide_kernels_leave_room_for_two_workgroups_per_cu(kernels):
    # static LDS, so the compiler's number is the whole allocation: records of 128 neighbours for four waves
    lds = {name: kernels[name]["lds_static"] for name in WIDE}
    assert all(v < 64 * 1024 for v in lds.values()), lds
    assert lds["annp::annp_niw_force<false>"] == 4 * (8 * 128 * 8 + 3 * 128 * 8 + 64 * 8 + 128 * 4)         # 49 152 bytes
    src = open(os.path.join(ROOT, "meng_zhang_amd", "csrc", "ni_wide_kernels.hpp")).read()
    assert "constexpr int NIW_CAP = 128;" in src and "ANNP_POISON();" in src


def test_existing_kernels_report_what_was_recorded(kernels):
    rec = {k["kernel"]: k for k in json.load(open(os.path.join(ROOT, "profiles", "r06_kernel_resources.json")))["kernels"]}
    watched = [n for n in rec if n.startswith(("annp::annp_mlp_mfma<", "annp::annp_ni_desc<", "annp::annp_ni_force<"))]
    assert len([n for n in watched if n.startswith("annp::annp_mlp_mfma<")]) == 12
    for n in watched:
        assert n in kernels, n
        for key in ("vgpr", "agpr", "scratch", "vgpr_spill", "occupancy"):
            assert kernels[n][key] == rec[n][key], (n, key, kernels[n][key], rec[n][key])
    assert not [n for n in kernels if n.startswith("annp::annp_mlp_mfma<") and n not in rec]       # no thirteenth instantiation
