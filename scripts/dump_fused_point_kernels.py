"""Every output of the fused per-point kernels (csrc/fused_mlp.h and its seven users) on fixed seeded inputs and the parity weights, as ONE
.npz -- to compare two builds of the library bit for bit:

    python scripts/dump_fused_point_kernels.py a.npz            (on one build)
    NU_NERF_LIB=/path/to/other/libnunerf.so python scripts/dump_fused_point_kernels.py b.npz
    python scripts/dump_fused_point_kernels.py --compare a.npz b.npz

Sizes per entry: 1 point, one tile minus one, one tile plus one, and a count that sends the 256-workgroup grid-stride loop into a second
round (8193 points on the 32-row kernels, 16385 on the 64-row SDF forward, 4097 on nu_sdf_grad_fwd, 1537 on nu_sdf_jet_fwd, 16641 rays
on nu_sdf_trace).  The existing tests tie the value paths to the layered path; nothing else ties gradients, Hessians, traced positions and
the light / shade outputs of two builds to each other.  The light and shade points include some beyond radius 0.999 (nu_sph_point rescales
those), and the kernels' test outputs (encoded rows, raw heads, feature columns) are dumped with the public ones."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    keys = sorted(set(a.files) | set(b.files))
    bad = [k for k in keys if k not in a.files or k not in b.files or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
           or a[k].tobytes() != b[k].tobytes()]
    print(f"{len(keys)} arrays, {sum(a[k].nbytes for k in a.files)} bytes: " + ("all equal, bit for bit" if not bad else f"DIFFERENT: {bad}"))
    return 1 if bad else 0


def shell(n, seed):
    """points at radius 0.2 .. 0.95, float32 [n,3]"""
    g = np.random.Generator(np.random.PCG64(seed))
    u = g.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * g.uniform(0.2, 0.95, (n, 1))).astype(np.float32)


def shell_rim(n, seed):
    """shell(n, seed) with every fourth point moved to radius 0.9985 .. 1.3: outside 0.999 the sphere-direction rows scale x by 0.999 / |x|"""
    x = shell(n, seed)
    g = np.random.Generator(np.random.PCG64(seed + 7))
    k = np.arange(0, n, 4)
    x[k] = (x[k] / np.linalg.norm(x[k], axis=1, keepdims=True) * g.uniform(0.9985, 1.3, (len(k), 1))).astype(np.float32)
    return x


def unit(n, seed, lo=1.0, hi=1.0):
    g = np.random.Generator(np.random.PCG64(seed))
    u = g.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * g.uniform(lo, hi, (n, 1))).astype(np.float32)


def main(out_path):
    import torch
    from nu_nerf_amd.renderer import NeROShapeRenderer
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    from nu_nerf_amd.engine import addr
    from nu_nerf_amd.materials import bake_materials
    from nu_nerf_amd.environment import bake_light
    from nu_nerf_amd.surface_shade import TERMS, shade_points
    from nu_nerf_amd.curvature import bake_curvature, bake_normals
    from nu_nerf_amd.sdf_trace import trace_rays

    dev = torch.device('cuda:0')
    out = {}

    def put(name, t):
        out[name] = t.detach().cpu().numpy() if hasattr(t, 'detach') else np.asarray(t)

    def put_dict(prefix, d):
        for k in sorted(d):
            if hasattr(d[k], 'detach'):
                put(f"{prefix}.{k}", d[k])

    def parity_net(cfg, sphere=False):
        net = NeROShapeRenderer(cfg, training=False)
        net.load_param_dict(randomize_for_parity(init_stage1_params(6033, sphere_direction=sphere), seed=1))
        return net.to(dev)

    T = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    net = parity_net({})
    eng = net.engine()
    eng.pack()

    # nu_sdf_fused_fwd: 32-row tiles below 192 x 64 points, 64-row tiles from there on
    for n in (1, 31, 33, 8193, 12287, 12289, 16385):
        x = T(shell(n, 100 + n))
        sdf = torch.empty(n, device=dev)
        eng.lib.nu_sdf_fused_fwd(ctypes.byref(eng._sdf_net), addr(x), 3, n, addr(sdf), eng.stream())
        put(f"sdf_fused.{n}", sdf)
    # nu_sdf_fused16_fwd (the bf16-storage kernels of the same file; their pipeline is their own)
    net16 = parity_net({'mlp_dtype': 'bf16'})
    e16 = net16.engine()
    e16.pack()
    for n in (1, 33, 8193, 30001):
        x = T(shell(n, 200 + n))
        sdf = torch.empty(n, device=dev)
        e16.lib.nu_sdf_fused16_fwd(ctypes.byref(e16._sdf_net), addr(x), 3, n, addr(sdf), e16.stream())
        put(f"sdf_fused16.{n}", sdf)
    # nu_material_bake_fwd
    for n in (1, 31, 33, 8193):
        put_dict(f"material_bake.{n}", bake_materials(net, T(shell(n, 300 + n)), transmission=True, sdf=True, _feat=True))
        put_dict(f"material_bake.raw.{n}", bake_materials(net, T(shell(n, 300 + n)), transmission=True, _raw=True))
    # nu_light_bake_fwd: direct and probe, with and without sphere directions
    for sphere in (False, True):
        ns = parity_net({'shader_config': {'sphere_direction': sphere}}, sphere)
        for n in (1, 31, 33, 8193):
            d, x = T(unit(n, 400 + n)), T(shell_rim(n, 500 + n))
            rho = T(np.random.Generator(np.random.PCG64(600 + n)).uniform(0.02, 1.0, n).astype(np.float32))
            put_dict(f"light_bake.sphere{int(sphere)}.direct.{n}", bake_light(ns, d, rho, x, _enc=True, _raw=True))
            put_dict(f"light_bake.sphere{int(sphere)}.probe.{n}", bake_light(ns, d, rho, x, probe=True, _enc=True, _raw=True))
        # nu_surface_shade_fwd
        for n in (1, 31, 33, 8193):
            x, v, nr = T(shell_rim(n, 700 + n)), T(unit(n, 800 + n, 0.5, 2.0)), T(unit(n, 900 + n, 0.5, 2.0))
            put_dict(f"surface_shade.sphere{int(sphere)}.{n}", shade_points(ns, x, v, nr, terms=tuple(TERMS), _enc=True, _raw=True))
    # nu_sdf_grad_fwd (16 points per tile) and nu_sdf_jet_fwd (6 points per tile)
    for n in (1, 15, 17, 4097):
        put_dict(f"sdf_grad.{n}", bake_normals(net, T(shell(n, 1000 + n))))
    for n in (1, 5, 7, 1537):
        put_dict(f"sdf_jet.{n}", bake_curvature(net, T(shell(n, 1100 + n)), hessian=True))
    # nu_sdf_trace (64 ray slots per workgroup): rays from a sphere of radius 3 towards points near the origin, some of them missing
    for n in (1, 63, 65, 16641):
        g = np.random.Generator(np.random.PCG64(1200 + n))
        o = unit(n, 1300 + n, 3.0, 3.0)
        tgt = (g.standard_normal((n, 3)) * 0.45).astype(np.float32)
        d = tgt - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        put_dict(f"sdf_trace.{n}", trace_rays(net, T(o), T(d.astype(np.float32)), max_iter=48, entry_forward=True))
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez(out_path, **out)
    print(f"{out_path}: {len(out)} arrays, {sum(v.nbytes for v in out.values())} bytes")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == '--compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
