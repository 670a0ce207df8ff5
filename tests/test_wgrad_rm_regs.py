"""Register / LDS budget of the row-major weight-gradient kernels (csrc/wgrad_rm.hip), read from the built object's metadata
(scripts/kernel_regs.py), beside tests/test_abi.py::test_register_budget_of_the_surviving_hot_kernels."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_row_major_wgrad_kernels_do_not_spill_and_fit_one_workgroup_per_cu():
    from nu_nerf_amd import build
    build.build(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_regs import kernel_table
    seen = []
    for name, r in kernel_table(os.path.join(ROOT, "nu_nerf_amd", "build", "wgrad_rm.o")):
        if name.startswith("wgrad_rm"):
            seen.append(name)
            assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
            assert r["vgpr"] <= 256, (name, r)                  # two waves per SIMD
            # 256-tile: one workgroup of eight waves per CU; 128-tile: two workgroups of four
            assert r["lds"] <= (160 if name.startswith("wgrad_rm256") else 80) * 1024, (name, r)
    assert len(seen) == 4, seen
