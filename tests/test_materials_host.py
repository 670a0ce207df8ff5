"""Material baking, the parts that need no GPU: the C entry is declared and bound, write_ply keeps its bytes and carries colours,
the command's argument handling, predict_materials on every renderer class, the fixtures' spread condition, the kernel's
resource figures."""
import ctypes
import os
import sys

import numpy as np
import pytest

from helpers import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mesh.write_ply(V4, F2) as the commit before vertex colours wrote it (two triangles over four vertices)
V4 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], np.float32)
F2 = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
PLAIN_PLY = bytes.fromhex(
    "706c790a666f726d61742062696e6172795f6c6974746c655f656e6469616e20312e300a656c656d656e742076657274657820340a70726f7065727479"
    "20666c6f617420780a70726f706572747920666c6f617420790a70726f706572747920666c6f6174207a0a656c656d656e74206661636520320a70726f"
    "7065727479206c69737420756368617220696e74207665727465785f696e64696365730a656e645f6865616465720a0000000000000000000000000000"
    "803f0000000000000000000000000000803f000000000000803f0000803f0000003f0300000000010000000200000003010000000300000002000000")


@pytest.fixture(scope="module")
def lib():
    from nu_nerf_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_entry_is_declared_and_bound(lib):
    text = open(os.path.join(ROOT, "include", "nu_nerf.h")).read()
    assert "int nu_material_bake_fwd(const NuBakeNet* net, const float* X, int x_ld, int P," in text
    fn = lib.nu_material_bake_fwd
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 10
    assert fn.argtypes[2] is ctypes.c_int and fn.argtypes[3] is ctypes.c_int
    assert all(fn.argtypes[i] is ctypes.c_void_p for i in (0, 1, 4, 5, 6, 7, 8, 9))
    from nu_nerf_amd.engine import BakeNet
    assert lib.nu_bake_net_size() == ctypes.sizeof(BakeNet)


def test_entry_returns_at_once_for_no_points_and_rejects_bad_arguments(lib):
    """No launch happens on these paths (the checks precede it): P = 0 is NU_OK whatever the pointers; a missing descriptor, a missing
    X and x_ld < 3 are NU_ERR_ARG, which the binding raises on."""
    from nu_nerf_amd._lib import NuNerfLibraryError
    from nu_nerf_amd.engine import BakeNet
    assert lib.nu_material_bake_fwd(None, None, 3, 0, None, None, None, None, None, None) == 0
    n = BakeNet()
    for args in ((None, 16, 3, 4), (ctypes.byref(n), None, 3, 4), (ctypes.byref(n), 16, 2, 4)):
        with pytest.raises(NuNerfLibraryError, match=r"nu_material_bake_fwd failed with code -1"):
            lib.nu_material_bake_fwd(*args, None, None, None, None, None, None)
    with pytest.raises(NuNerfLibraryError, match=r"code -1"):       # an empty descriptor (no tables)
        lib.nu_material_bake_fwd(ctypes.byref(n), 16, 3, 4, None, None, None, None, None, None)


def test_write_ply_without_colours_keeps_its_bytes(tmp_path):
    from nu_nerf_amd.mesh import write_ply, read_ply
    p = tmp_path / "plain.ply"
    write_ply(p, V4, F2)
    assert p.read_bytes() == PLAIN_PLY
    V, F, C = read_ply(p, colors=True)
    assert C is None and np.array_equal(V, V4) and np.array_equal(F, F2)


def test_coloured_ply_round_trips(tmp_path):
    from nu_nerf_amd.mesh import write_ply, read_ply
    albedo = np.array([[0.0, 0.5, 1.0], [0.1, 0.2, 0.3], [1.2, -0.1, 0.999], [0.25, 0.75, 0.0]], np.float32)
    p = tmp_path / "col.ply"
    write_ply(p, V4, F2, colors=albedo)
    V, F, C = read_ply(p, colors=True)
    assert np.array_equal(V, V4) and np.array_equal(F, F2)
    assert C.dtype == np.uint8 and np.array_equal(C, np.clip(np.rint(255.0 * albedo.astype(np.float64)), 0, 255).astype(np.uint8))
    V2, F2b = read_ply(p)                        # the two-value form skips the colours
    assert np.array_equal(V2, V4) and np.array_equal(F2b, F2)
    u8 = np.arange(12, dtype=np.uint8).reshape(4, 3)
    write_ply(p, V4, F2, colors=u8)
    assert np.array_equal(read_ply(p, colors=True)[2], u8)
    with pytest.raises(ValueError):
        write_ply(p, V4, F2, colors=albedo[:3])


def test_command_arguments_and_output_paths():
    from nu_nerf_amd.extract_materials import parse_args, which_of, output_paths
    f = parse_args(['--cfg', 'c.yaml'])
    assert which_of(f) == 'outer' and not f.ply
    assert output_paths(f, 'bear', 300000) == (os.path.join('data', 'meshes', 'bear-300000.ply'),
                                               os.path.join('data', 'materials', 'bear-300000'), None)
    f = parse_args(['--cfg', 'c.yaml', '--stage2'])
    assert which_of(f) == 'inner'
    assert which_of(parse_args(['--cfg', 'c.yaml', '--stage2', '--outer'])) == 'outer'
    assert which_of(parse_args(['--cfg', 'c.yaml', '--stage2', '--inner'])) == 'inner'
    f = parse_args(['--cfg', 'c.yaml', '--mesh', 'm/x_simplified.ply', '--out', 'o/dir', '--ply'])
    assert output_paths(f, 'bear', 7) == ('m/x_simplified.ply', 'o/dir', os.path.join('o/dir', 'x_simplified_albedo.ply'))
    for bad in (['--cfg', 'c.yaml', '--inner'], ['--cfg', 'c.yaml', '--stage2', '--inner', '--outer'], ['--mesh', 'm.ply']):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_every_renderer_class_has_predict_materials():
    from nu_nerf_amd import stage2, stage2_thick
    from nu_nerf_amd.compat.network import renderer as c_std, renderer_zerothick as c_zero
    seen = 0
    for reg in (stage2.name2renderer, stage2_thick.name2renderer, c_std.name2renderer, c_zero.name2renderer):
        assert set(reg) == {'shape', 'stage2'}
        for cls in reg.values():
            assert callable(getattr(cls, 'predict_materials', None)), cls
            seen += 1
    assert seen == 8


def test_which_is_checked_before_anything_runs():
    from nu_nerf_amd.materials import _resolve_which

    class S1:
        pass

    class S2:
        stage1_network = sdf_network_inner = None
    assert _resolve_which(S1(), None) == 'outer' and _resolve_which(S2(), None) == 'inner' and _resolve_which(S2(), 'outer') == 'outer'
    with pytest.raises(ValueError):
        _resolve_which(S1(), 'inner')
    with pytest.raises(ValueError):
        _resolve_which(S2(), 'both')


@pytest.mark.parametrize("name", ["materials_stage1.npz", "materials_stage2_inner.npz"])
def test_fixture_spread(name):
    """A test against the fixture cannot pass on a constant: every channel spans at least 0.02 and none is saturated."""
    g = golden(name)
    n = g['points'].shape[0]
    assert n == 1024 and int(g['n_mesh_vertices']) == 642 and g['faces'].max() < 642
    for k, cols in (('metallic', 1), ('roughness', 1), ('albedo', 3)):
        a = g[k]
        assert a.shape == (n, cols) and a.dtype == np.float32
        for c in range(cols):
            assert a[:, c].max() - a[:, c].min() >= 0.02 and a[:, c].min() >= 0.02 and a[:, c].max() <= 0.98, (k, c)
    assert len([k for k in g if k.startswith('override__')]) == 3
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', name)) < 200 * 1024


def test_resource_figures_of_the_bake_kernel(lib):
    """Code-object metadata of the built object (scripts/kernel_regs.py): no scratch, no VGPR spill, and the LDS layout DESIGN 19
    describes -- 149 536 bytes, one workgroup per CU."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_regs import kernel_table
    rows = [(n, r) for n, r in kernel_table(os.path.join(ROOT, "nu_nerf_amd", "build", "bake.o")) if n.startswith("material_bake_fwd_kernel")]
    assert len(rows) == 1
    r = rows[0][1]
    assert r["scratch"] == 0 and r["vgpr_spill"] == 0, r
    assert r["lds"] == 4 * ((32 * 260 + 4) + (32 * 292 + 4) + 32 * 40 + 2 * 256 * 36) == 149536 and r["lds"] <= 160 * 1024, r
