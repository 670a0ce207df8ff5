"""python -m nu_nerf_amd.extract_mesh --cfg CFG [--resolution 1024] [--ckpt PATH] [--out PATH] [--stage2] [--remesh] [--fix ...]
[--decimate N] [--sparse [--block 8] [--lipschitz 2.0]]

extract_mesh_stage1.py on the GPU: the renderer named by the config (`zero_thickness` picks the module set) loads
data/model/{name}/model.pth (train_glue.save_checkpoint format), its SDF is sampled on the [-1,1]^3 grid (mesh.sdf_grid), marching
cubes runs at threshold 0, the faces are flipped (np.fliplr: outward normals) and data/meshes/{name}-{step}.ply is written -- the
raw mesh.  --remesh also writes data/meshes/{name}-{step}_simplified.ply (the file the stage-2 configs' `stage1_mesh_dir` names):
the reference's pymeshlab isotropic remeshing at 0.5 % of the bounding-box diagonal, here remesh.remesh_isotropic on the GPU.
--fix also writes data/meshes/{name}-{step}_fixed.ply: the raw mesh without its floaters (components.remove_floaters; the switches
of python -m nu_nerf_amd.clean_mesh: --keep, --min-area-frac, --min-faces, --drop-cavities, --connectivity), and --remesh then
remeshes the fixed mesh instead of the raw one.  Without --fix every file is written as before.
--decimate N also writes data/meshes/{name}-{step}_decimated.ply: the (fixed) mesh brought down to N faces by quadric-error collapses
(decimate.decimate); it runs after --fix and before --remesh, which then starts from the decimated mesh.

--stage2: extract_mesh_stage2.py -- a stage-2 checkpoint; the field is the inner sdf where the stage-1 sdf is < 0 and 1 elsewhere
(mesh.stage2_inner_grid), no face flip.

--sparse: the same mesh through the block-sparse path (mesh.extract_mesh_sparse / extract_stage2_mesh_sparse): the SDF is
evaluated only in the blocks of --block^3 grid points (4 or 8) that the zero set can reach under the gradient bound --lipschitz; if
the kept blocks turn out to cut the surface the bound is doubled and the extraction repeated.  The vertices and triangles are those
of the dense path, ordered by block.  --fix, --decimate and --remesh follow unchanged; without --sparse nothing changes.
"""
import argparse
import os
import sys


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.extract_mesh", description=__doc__.split("\n\n")[1])
    ap.add_argument('--cfg', type=str, required=True, help="training config (YAML)")
    ap.add_argument('--resolution', type=int, default=1024, help="grid points per axis (default 1024)")
    ap.add_argument('--ckpt', type=str, default=None, help="checkpoint (default data/model/{name}/model.pth)")
    ap.add_argument('--out', type=str, default=None, help="output PLY (default data/meshes/{name}-{step}.ply)")
    ap.add_argument('--stage2', action='store_true', help="inner surface of a stage-2 model (extract_mesh_stage2.py)")
    ap.add_argument('--remesh', action='store_true', help="also write the isotropically remeshed OUT_simplified.ply")
    ap.add_argument('--slab-points', type=int, default=None, help="grid points per SDF evaluation slab (default mesh.SLAB_POINTS)")
    ap.add_argument('--fix', action='store_true', help="also write OUT_fixed.ply without floaters; --remesh then starts from it")
    ap.add_argument('--decimate', type=int, default=None, metavar='N',
                    help="also write OUT_decimated.ply with about N faces (after --fix); --remesh then starts from it")
    ap.add_argument('--sparse', action='store_true', help="evaluate the SDF only in the blocks near the surface (same mesh, ordered by block)")
    ap.add_argument('--block', type=int, default=None, choices=(4, 8), help="--sparse: grid points per block edge (default 8)")
    ap.add_argument('--lipschitz', type=float, default=None, help="--sparse: bound on |grad sdf| used to cull blocks (default 2.0)")
    from .clean_mesh import add_fix_options
    add_fix_options(ap)
    flags = ap.parse_args(argv)
    if not flags.sparse and (flags.block is not None or flags.lipschitz is not None):
        ap.error("--block and --lipschitz belong to --sparse")
    flags.block = 8 if flags.block is None else flags.block
    flags.lipschitz = 2.0 if flags.lipschitz is None else flags.lipschitz
    if not flags.lipschitz > 0:
        ap.error("--lipschitz must be positive")
    if flags.decimate is not None and flags.decimate < 4:
        ap.error("--decimate must be >= 4")
    return flags


def _renderer(cfg):
    if cfg.get('zero_thickness', True):
        from .stage2 import name2renderer          # registers 'stage2' next to the stage-1 'shape'
    else:
        from .stage2_thick import name2renderer
    return name2renderer[cfg['network']](cfg, training=False)


def main(argv=None):
    flags = parse_args(argv)
    import numpy as np
    import torch
    import yaml
    from . import mesh
    from .train_glue import load_checkpoint

    with open(flags.cfg) as fh:
        cfg = yaml.safe_load(fh)
    network = _renderer(cfg)
    ckpt = flags.ckpt or f'data/model/{cfg["name"]}/model.pth'
    _, step = load_checkpoint(ckpt, network, map_location='cpu')
    network = network.eval().to(torch.device('cuda', torch.cuda.current_device()))
    print(f'successfully load {cfg["name"]} step {step}!')
    res = flags.resolution
    if flags.stage2:
        s1_ckpt = network.cfg.get('stage1_ckpt_dir')
        if s1_ckpt and os.path.exists(s1_ckpt):                # extract_mesh_stage2.py:27-34: stage 1 from its own checkpoint
            load_checkpoint(s1_ckpt, network.stage1_network, map_location='cpu')
        if flags.sparse:
            stats = {}
            V, F = mesh.extract_stage2_mesh_sparse(network, res, 0.0, block=flags.block, lipschitz=flags.lipschitz,
                                                   slab_points=flags.slab_points, stats=stats)
            print(f'sparse: {stats}')
        else:
            u = mesh.stage2_inner_grid(network, res, slab_points=flags.slab_points)
            V, F = mesh.marching_cubes(u, 0.0)
            V, F = mesh._to_world(V, res, mesh.BOX_MIN, mesh.BOX_MAX), F.cpu().numpy()
    else:
        if flags.sparse:
            stats = {}
            V, F = mesh.extract_mesh_sparse(network, res, 0.0, block=flags.block, lipschitz=flags.lipschitz,
                                            slab_points=flags.slab_points, stats=stats)
            print(f'sparse: {stats}')
        else:
            V, F = mesh.extract_mesh(network, res, 0.0, slab_points=flags.slab_points)
        F = np.ascontiguousarray(np.fliplr(F))
    out = flags.out or os.path.join('data', 'meshes', f'{cfg["name"]}-{step}.ply')
    os.makedirs(os.path.dirname(out) or '.', exist_ok=True)
    mesh.write_ply(out, V, F)
    print(f'wrote {out}: {len(V)} vertices, {len(F)} triangles')
    if flags.fix:
        from .clean_mesh import fix_kwargs, fixed_path
        V, F = mesh.remove_floaters(V, F, **fix_kwargs(flags))
        out_f = fixed_path(out)
        mesh.write_ply(out_f, V, F)
        print(f'wrote {out_f}: {len(V)} vertices, {len(F)} triangles')
    if flags.decimate is not None:
        from .decimate import decimated_path
        V, F = mesh.decimate(V, F, flags.decimate)
        out_d = decimated_path(out)
        mesh.write_ply(out_d, V, F)
        print(f'wrote {out_d}: {len(V)} vertices, {len(F)} triangles')
    if flags.remesh:
        from .remesh import remesh_isotropic, simplified_path
        Vs, Fs = remesh_isotropic(V, F)
        out_s = simplified_path(out)
        mesh.write_ply(out_s, Vs, Fs)
        print(f'wrote {out_s}: {len(Vs)} vertices, {len(Fs)} triangles')
    return out


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
