"""The C-ABI library builds for gfx950, loads, and exports every symbol include/nu_nerf.h declares (no GPU needed,
no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from nu_nerf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def declared_functions():
    text = open(os.path.join(ROOT, "include", "nu_nerf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nu_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_expected_surface():
    names = declared_functions()
    for must in ("nu_gemm_nt_ex", "nu_wgrad", "nu_pack_layers", "nu_unpack_grads", "nu_composite_fwd", "nu_composite_bwd",
                 "nu_neus_alpha_fwd", "nu_neus_alpha_bwd", "nu_upsample", "nu_merge_sorted", "nu_shade_combine_fwd",
                 "nu_shade_combine_bwd", "nu_ide", "nu_partition_count", "nu_partition_write"):
        assert must in names
    # network-level entries of SURVEY 8(b) and the fused loss (N1)
    for must in ("nu_sdf_mlp_fwd", "nu_sdf_mlp_normal", "nu_sdf_mlp_bwd", "nu_nerfpp_mlp_fwd", "nu_nerfpp_mlp_bwd", "nu_shading_stack_fwd",
                 "nu_shading_stack_bwd", "nu_ctx_flush", "nu_loss_fwd", "nu_loss_bwd", "nu_sdf_fused_fwd", "nu_lbvh_build", "nu_lbvh_trace",
                 "nu_s2_seg_count", "nu_s2_seg_write", "nu_s2_ddist", "nu_s2_seg_bwd", "nu_s2_composite_fwd", "nu_s2_composite_bwd",
                 "nu_s2_refract_fwd", "nu_s2_refract_bwd", "nu_s2_hit_fwd", "nu_s2_hit_bwd", "nu_s2_far_points", "nu_s2_far_resample",
                 "nu_s2_shade_combine_fwd", "nu_s2_shade_combine_bwd", "nu_s2_neus_alpha_fwd", "nu_s2_neus_alpha_bwd",
                 "nu_skinny_fwd_h16", "nu_skinny_bwd_enqueue_h16", "nu_s2_shell_fwd", "nu_s2_shell_bwd", "nu_embed_n_fwd", "nu_embed_n_bwd", "nu_s2_shade_encode_fwd", "nu_s2_shade_encode_bwd", "nu_unpack_grads_range"):
        assert must in names
    assert len(names) >= 50


def test_library_exports_every_declared_symbol(lib):
    missing = [n for n in declared_functions() if not hasattr(lib, n)]
    assert not missing, missing


def test_struct_layouts_match_python_mirrors(lib):
    from nu_nerf_amd.engine import PackDesc, GemmNT, GemmTN
    assert lib.nu_pack_desc_size() == ctypes.sizeof(PackDesc)
    # natural-alignment sizes of the C structs in include/nu_nerf.h
    assert ctypes.sizeof(GemmNT) == 240 and ctypes.sizeof(GemmTN) == 152
    assert lib.nu_gemm_nt_size() == 240 and lib.nu_gemm_tn_size() == 152 and lib.nu_reduce_desc_size() == 64
    from nu_nerf_amd.engine import OpCtx, SdfNet, SdfBufs, NerfNet, NerfBufs, ShadeNet, ShadeBufs
    for fn, st in (("nu_op_ctx_size", OpCtx), ("nu_sdf_net_size", SdfNet), ("nu_sdf_bufs_size", SdfBufs), ("nu_nerf_net_size", NerfNet),
                   ("nu_nerf_bufs_size", NerfBufs), ("nu_shade_net_size", ShadeNet), ("nu_shade_bufs_size", ShadeBufs)):
        assert getattr(lib, fn)() == ctypes.sizeof(st), fn


def test_workspace_queries_are_pure_host_functions(lib):
    assert lib.nu_wgrad_workspace_bytes(256, 256, 4, 1) == 4 * 256 * 257 * 4
    assert lib.nu_skinny_bwd_workspace_bytes(256, 3) > 0
    assert lib.nu_colsum_workspace_bytes(256) > 0


def declared_parameter_counts():
    """name -> parameter count of every nu_* declaration, NU_RM_ARGS (the remeshing entries' shared parameters) expanded."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nu_nerf.h")).read(), flags=re.S).replace("\\\n", " ")
    rm_args = re.search(r"#define NU_RM_ARGS (.*)", text).group(1)
    text = re.sub(r"\bNU_RM_ARGS\b", rm_args, text)
    return {name: 0 if params.strip() in ("", "void") else params.count(",") + 1
            for name, params in re.findall(r"\b(nu_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}


def test_every_declared_function_is_bound_with_the_header_signature(lib):
    counts = declared_parameter_counts()
    assert sorted(counts) == declared_functions()
    for name, n in counts.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n, (name, fn.argtypes, n)
        assert fn.restype in (ctypes.c_int, ctypes.c_longlong), name
    assert lib.nu_mc_count.argtypes[4] is ctypes.c_float                        # float iso
    assert lib.nu_adam_step.argtypes[2] is ctypes.c_double                       # double lr
    assert lib.nu_wgrad_workspace_bytes.restype is ctypes.c_longlong
    assert lib.nu_mc_count.argtypes[0] is ctypes.c_void_p and lib.nu_mc_count.argtypes[-1] is ctypes.c_void_p   # pointer, stream


def test_long_long_results_keep_all_64_bits(lib):
    nbytes = lib.nu_wgrad_workspace_bytes(1024, 1024, 1024, 1)
    assert nbytes == 1024 * 1024 * 1025 * 4 and nbytes > 2 ** 31


def test_negative_result_raises_naming_the_entry(lib):
    """nu_gemm_nt rejects K % 32 != 0 before any HIP call: NU_ERR_ARG comes back, and the binding raises on it."""
    from nu_nerf_amd._lib import NuNerfLibraryError
    with pytest.raises(NuNerfLibraryError, match=r"nu_gemm_nt failed with code -1"):
        lib.nu_gemm_nt(None, 32, None, 32, 64, 64, 3, None, 64, None, 0, None, None, 0, None, 0, None, 0, 0, 1.0, 0, None)


def test_missing_argument_is_a_type_error_before_the_call(lib):
    with pytest.raises(TypeError):
        lib.nu_wgrad_workspace_bytes(1024, 1024, 1024)


def test_code_object_targets_gfx950_only():
    so = os.path.join(ROOT, "nu_nerf_amd", "libnunerf.so")
    data = open(so, "rb").read()
    assert b"gfx950" in data
    for other in (b"gfx942", b"gfx90a", b"sm_90"):
        assert other not in data


def test_register_budget_of_the_surviving_hot_kernels(lib):
    """Reads the code-object metadata of the built objects (scripts/kernel_regs.py: llvm-readelf --notes on the device ELF inside
    nu_nerf_amd/build/*.o).  The exact-fp32 default kernels -- NT (single problem and batched), the weight-gradient kernels, the
    fused SDF forwards -- must not spill a single VGPR and use no scratch memory.  The bf16-storage NT kernel (gemm_nt16b_kernel) is
    built for THREE workgroups per CU (168 VGPRs): its bf16-operand instantiations may spill at most 16 registers in the per-tile
    prologue / epilogue (none in the chunk loop) -- measured on config 4, same box: the spill-free two-workgroup build is 16 % slower
    per step (44.2 vs 38.2 ms, profiles/r04/README.md), occupancy is what this latency-bound kernel lives on -- and the instantiations
    with an fp32 A operand (one more 16-register prefetch set) at most 36 (Q_SP: 33; one launch per step)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_regs import kernel_table
    bdir = os.path.join(ROOT, "nu_nerf_amd", "build")
    seen = 0
    for obj in ("gemm_nt", "gemm_tn", "fused_sdf"):
        for name, r in kernel_table(os.path.join(bdir, obj + ".o")):
            hot = name.startswith(("gemm_nt2_kernel<", "gemm_nt2b_kernel<", "gemm_tn2_kernel<", "gemm_tn2b_kernel<", "gemm_tnb_kernel<",
                                   "gemm_tn_kernel<false, 0>", "gemm_tn_kernel<true, 0>", "sdf_fused"))
            if hot:
                seen += 1
                assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
    # all of them: NT 18 + batched NT 8, weight gradients 2 + 1 batched + 1 batched 128-tile + 2 first-generation, fused SDF 5
    assert seen == 37
    n16 = 0
    for name, r in kernel_table(os.path.join(bdir, "gemm_nt16.o")):
        if name.startswith("gemm_nt16b_kernel<"):
            n16 += 1
            cap = 16 if ", true>" in name else 36      # (Q_SP 15, bias + ReLU 10, softplus 9, B_RELU 7, the others 0-4 with the per-slab / per-width
            # copies of the epilogue fast path; no scratch instruction between the first and the last MFMA of any of them; config 4 measured 1.6 %
            # faster per step WITH these copies, profiles/r04/epilogue_fast_path_copies_ab.txt)
            assert r["vgpr_spill"] <= cap and r["vgpr"] <= 168, (name, r)
            assert r["lds"] <= 53 * 1024, (name, r)             # three workgroups per CU
    assert n16 == 18

