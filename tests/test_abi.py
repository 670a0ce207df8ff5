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


# sizeof of every struct of include/nu_nerf.h under the natural alignment of the x86-64 / amdgcn ABIs, and offsets a size cannot see
# (two fields swapped, a pointer for a long long).  Literals on purpose: they depend neither on the header reader nor on the library.
STRUCT_BYTES = {"GemmNT": 240, "GemmTN": 152, "ReduceDesc": 64, "PackDesc": 160, "Lin": 80, "WgradItem": 208, "OpCtx": 104,
                "SdfNet": 720, "SdfBufs": 400, "NerfNet": 960, "NerfBufs": 304, "ShadeNet": 1560, "ShadeBufs": 552, "BakeNet": 816,
                "AdamDesc": 48}
SIZE_ENTRIES = {"nu_gemm_nt_size": 240, "nu_gemm_tn_size": 152, "nu_reduce_desc_size": 64, "nu_pack_desc_size": 160,
                "nu_wgrad_item_size": 208, "nu_op_ctx_size": 104, "nu_sdf_net_size": 720, "nu_sdf_bufs_size": 400,
                "nu_nerf_net_size": 960, "nu_nerf_bufs_size": 304, "nu_shade_net_size": 1560, "nu_shade_bufs_size": 552,
                "nu_bake_net_size": 816, "nu_adam_desc_size": 48}
FIELD_OFFSETS = {"GemmNT.lda": 8, "GemmNT.epi": 208, "GemmNT.bf16": 212, "GemmNT.mask": 216, "GemmNT.B6": 232, "GemmTN.bf16": 144,
                 "ReduceDesc.alpha": 56, "PackDesc.w6_row0": 136, "WgradItem.dW": 152, "OpCtx.ndesc": 48, "OpCtx.pend": 88,
                 "SdfBufs.Q": 192, "NerfBufs.dA": 208, "ShadeNet.lut": 1464, "ShadeBufs.dYX": 544, "BakeNet.feat": 800, "AdamDesc.n": 32}


def test_struct_layouts_read_from_the_header():
    """The ctypes structs come from include/nu_nerf.h (nu_nerf_amd/_lib.py); no library and no GPU is needed to build them."""
    from nu_nerf_amd import _lib, engine
    assert set(_lib.STRUCTS) == set(STRUCT_BYTES)
    for name, nbytes in STRUCT_BYTES.items():
        assert ctypes.sizeof(getattr(_lib, name)) == nbytes, name
        assert getattr(_lib, name) is _lib.STRUCTS[name] and issubclass(_lib.STRUCTS[name], ctypes.Structure)
    for path, off in FIELD_OFFSETS.items():
        st, field = path.split(".")
        assert getattr(getattr(_lib, st), field).offset == off, path
    # what the engine builds positionally and the tests / scripts import from it
    assert engine.GemmNT is _lib.GemmNT and engine.GemmTN is _lib.GemmTN and engine.BakeNet is _lib.BakeNet
    assert [f for f, _ in _lib.Lin._fields_] == ["Wp", "WpT", "dWp", "bias", "db_off", "N", "K", "Kp", "ldT", "ldd", "pad_", "Wp16", "WpT16"]
    assert [f for f, _ in _lib.GemmNT._fields_][:9] == ["A", "lda", "B", "ldb", "M", "N", "K", "C", "ldc"]
    assert _lib.GemmNT.A.size == 8 and _lib.GemmNT.alpha.size == 4 and _lib.GemmNT.sA.size == 8 and _lib.WgradItem.g.size == 152
    assert _lib.SdfBufs.H.size == 72 and _lib.SdfNet.lin.size == 720 and _lib.ShadeNet.dbM_off.size == 24


def test_compiled_struct_sizes(lib):
    """Every nu_*_size entry of the header against the literal: the library agrees with the table above, hence with the structs."""
    assert sorted(n for n in declared_functions() if n.endswith("_size")) == sorted(SIZE_ENTRIES)
    for fn, nbytes in SIZE_ENTRIES.items():
        assert getattr(lib, fn)() == nbytes, fn
    from nu_nerf_amd.engine import PackDesc, GemmNT, GemmTN
    assert lib.nu_pack_desc_size() == ctypes.sizeof(PackDesc)
    assert ctypes.sizeof(GemmNT) == 240 and ctypes.sizeof(GemmTN) == 152
    from nu_nerf_amd.engine import OpCtx, SdfNet, SdfBufs, NerfNet, NerfBufs, ShadeNet, ShadeBufs
    for fn, st in (("nu_op_ctx_size", OpCtx), ("nu_sdf_net_size", SdfNet), ("nu_sdf_bufs_size", SdfBufs), ("nu_nerf_net_size", NerfNet),
                   ("nu_nerf_bufs_size", NerfBufs), ("nu_shade_net_size", ShadeNet), ("nu_shade_bufs_size", ShadeBufs)):
        assert getattr(lib, fn)() == ctypes.sizeof(st), fn


def test_header_constants():
    from nu_nerf_amd import _lib, engine
    epi = ("BIAS_NONE", "BIAS_RELU", "BIAS_SOFTPLUS", "MUL_DRELU", "MUL_DSP", "Q_SP", "B_SP", "PLAIN", "B_RELU")
    for value, name in enumerate(epi):
        assert getattr(_lib, "EPI_" + name) == value and getattr(_lib, "NU_EPI_" + name) == value and getattr(engine, "EPI_" + name) == value
    assert _lib.NU_EPI_COUNT == 9
    assert (_lib.NU_OK, _lib.NU_ERR_ARG, _lib.NU_ERR_LAUNCH, _lib.NU_ERR_WORKSPACE) == (0, -1, -2, -3)
    assert (_lib.NU_GEMM_PRESPLIT_ALWAYS, _lib.NU_GEMM_B16, _lib.NU_GEMM_A16, _lib.NU_GEMM_C16, _lib.NU_GEMM_X16) == (4, 8, 16, 32, 64)
    assert (_lib.NU_TN_A0_16, _lib.NU_TN_B0_16, _lib.NU_TN_A1_16, _lib.NU_TN_B1_16) == (16, 32, 64, 128)
    assert (_lib.NU_REDUCE_MAX, _lib.NU_NT_BATCH_MAX, _lib.NU_WGRAD_QUEUE_MAX, _lib.NU_ADAM_MAX) == (48, 8, 32, 80)
    assert not hasattr(_lib, "NU_RM_ARGS") and not hasattr(_lib, "NU_NERF_H")          # no integers: not constants


@pytest.mark.parametrize("text,names", [
    ("typedef struct NuBad { int n; short x; } NuBad;", ("NuBad", "x", "short")),                 # a type the reader does not map
    ("typedef struct NuBad { float* p; unsigned y; } NuBad;", ("NuBad", "y", "unsigned")),
    ("typedef struct NuBad { NuLater z; } NuBad; typedef struct NuLater { int a; } NuLater;", ("NuBad", "z", "NuLater")),
    ("typedef struct NuBad { float* H[NU_NOT_DEFINED]; } NuBad;", ("NuBad", "H", "NU_NOT_DEFINED")),     # array bounds
    ("typedef struct NuBad { int v[NU_ZERO]; } NuBad;", ("NuBad", "v", "NU_ZERO")),
    ("typedef struct NuBad { int v[2 + 2]; } NuBad;", ("NuBad", "v")),                              # declarator shapes
    ("typedef struct NuBad { int (*fn)(int); } NuBad;", ("NuBad", "fn")),
    ("typedef struct NuBad { int bits : 3; } NuBad;", ("NuBad", "bits")),
    ("typedef struct NuBad { int a; } NuOther;", ("NuBad", "NuOther")),
    ("typedef struct NuBad { int a; union { int b; float c; } u; } NuBad;", ("NuBad",)),         # nested bodies are not skipped
    ("struct NuBad { int a; };", ("NuBad",)),
])
def test_header_reader_fails_closed(text, names):
    from nu_nerf_amd._lib import NuNerfLibraryError, _structs
    with pytest.raises(NuNerfLibraryError) as err:
        _structs(text, {"NU_FOUR": 4, "NU_ZERO": 0})
    for name in names:
        assert name in str(err.value), (name, str(err.value))


def test_header_reader_maps_what_the_header_uses():
    from nu_nerf_amd._lib import _structs
    got = _structs("typedef struct NuIn { const float *a, *b; float c, *d; unsigned long long* m; double e; void** v; } NuIn;"
                   "typedef struct NuOut { NuIn one, two[NU_FOUR]; long long s[3]; const NuIn* p; int n; } NuOut;", {"NU_FOUR": 4})
    assert [(f, t.__name__) for f, t in got["In"]._fields_] == [("a", "c_void_p"), ("b", "c_void_p"), ("c", "c_float"), ("d", "c_void_p"),
                                                                ("m", "c_void_p"), ("e", "c_double"), ("v", "c_void_p")]
    assert ctypes.sizeof(got["In"]) == 56 and got["In"].c.offset == 16 and got["In"].d.offset == 24
    assert ctypes.sizeof(got["Out"]) == 56 * 5 + 24 + 8 + 8 and got["Out"].two.offset == 56 and got["Out"].s.offset == 280
    assert got["Out"]._fields_[0][1] is got["In"]


def test_load_rejects_a_struct_whose_compiled_size_differs(lib, monkeypatch):
    """load() compares every struct with its nu_*_size entry: a header out of step with the library is an error naming the struct."""
    from nu_nerf_amd import _lib
    grown = type("AdamDesc", (ctypes.Structure,), {"_fields_": list(_lib.AdamDesc._fields_) + [("extra", ctypes.c_longlong)]})
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.STRUCTS, "AdamDesc", grown)
    with pytest.raises(_lib.NuNerfLibraryError, match=r"NuAdamDesc.*nu_adam_desc_size\(\) = 48.*56"):
        _lib.load()
    monkeypatch.setitem(_lib.STRUCTS, "Orphan", grown)               # a struct without a size entry (other than NuLin)
    monkeypatch.setitem(_lib.STRUCTS, "AdamDesc", _lib.AdamDesc)
    with pytest.raises(_lib.NuNerfLibraryError, match=r"no nu_\*_size entry for struct NuOrphan"):
        _lib.load()


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


# kernel -> (object, LDS bytes its file's header states, SGPR spills: never more than before csrc/fused_mlp.h existed)
FUSED_POINT_KERNELS = {
    "sdf_fused_fwd_kernel<1>": ("fused_sdf", 112144, 0),
    "sdf_fused_fwd_kernel<2>": ("fused_sdf", 150544, 0),
    "material_bake_fwd_kernel": ("bake", 149536, 7),                # 29 with its own copy of the pipeline
    "light_bake_fwd_kernel": ("light_bake", 158784, 37),            # 60
    "surface_shade_fwd_kernel": ("surface_shade", 133152, 65),      # (its own copy of the pipeline)
    "sdf_grad_fwd_kernel": ("sdf_grad", 150800, 0),
    "sdf_jet_fwd_kernel": ("sdf_jet", 150800, 0),
    "sdf_trace_kernel": ("sdf_trace", 153108, 4),
}


def test_register_budget_of_the_fused_point_kernels(lib):
    """The fused per-point kernels (csrc/fused_mlp.h; surface_shade still carries its own copy of the pipeline): no VGPR spill, no
    scratch, the LDS figure each file's header states (one workgroup per CU by LDS), and no more SGPR spills than recorded when the
    header arrived, which is nowhere more than each kernel had with its own copy of the pipeline -- how the header packages the weight
    cursor decides the SGPR allocation around the main loop, and sdf_grad, sdf_jet and the SDF forward had none."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_regs import kernel_table
    bdir = os.path.join(ROOT, "nu_nerf_amd", "build")
    seen = set()
    for kernel, (obj, lds, sgpr_spill) in FUSED_POINT_KERNELS.items():
        for name, r in kernel_table(os.path.join(bdir, obj + ".o")):
            if name.startswith(kernel + "("):
                seen.add(kernel)
                assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
                assert r["lds"] == lds, (name, r)
                assert r["sgpr_spill"] <= sgpr_spill, (name, r)
    assert seen == set(FUSED_POINT_KERNELS)

