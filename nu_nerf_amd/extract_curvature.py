"""python -m nu_nerf_amd.extract_curvature --cfg CFG [--mesh PLY] [--ckpt PATH] [--stage2] [--inner|--outer] [--out DIR]

Per-vertex curvature of the trained surface at the vertices of a mesh, from the SDF's Hessian (curvature.py, one fused kernel): the
renderer named by the config loads data/model/{name}/model.pth (as extract_materials does) and DIR/curvature.npy [V,1] (Gaussian),
DIR/mean_curvature.npy [V] and DIR/sdf_normal.npy [V,3] are written: float32, unclipped, in the vertex order of the PLY.
curvature.npy is what relight --shell-curvature takes.

--mesh defaults to data/meshes/{name}-{step}.ply, --out to data/materials/{name}-{step}.  --stage2: a stage-2 config; --inner (default)
asks the inner SDF, --outer the stage-1 SDF the model carries (the shell: pass the stage-1 mesh as --mesh).  Prints one JSON line: V,
the Gauss-Bonnet ratio sum K A_v / (2 pi chi) when chi != 0, the percentiles of K and the share of vertices outside +-10, and the
same percentiles of the mesh's angle-defect curvature (lbvh.vertex_normals_and_curvature, which clips to +-10) for comparison.
"""
import argparse
import json
import os
import sys

FILES = {'gaussian': 'curvature.npy', 'mean': 'mean_curvature.npy', 'normal': 'sdf_normal.npy'}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.extract_curvature", description=__doc__.split("\n\n")[1])
    ap.add_argument('--cfg', type=str, required=True, help="training config (YAML)")
    ap.add_argument('--mesh', type=str, default=None, help="mesh whose vertices are evaluated (default data/meshes/{name}-{step}.ply)")
    ap.add_argument('--ckpt', type=str, default=None, help="checkpoint (default data/model/{name}/model.pth)")
    ap.add_argument('--stage2', action='store_true', help="the config is a stage-2 config")
    side = ap.add_mutually_exclusive_group()
    side.add_argument('--inner', action='store_true', help="stage 2: the inner SDF (default)")
    side.add_argument('--outer', action='store_true', help="stage 2: the stage-1 SDF of the stage-2 model")
    ap.add_argument('--out', type=str, default=None, help="output directory (default data/materials/{name}-{step})")
    flags = ap.parse_args(argv)
    if (flags.inner or flags.outer) and not flags.stage2:
        ap.error("--inner / --outer need --stage2")
    return flags


def which_of(flags):
    if not flags.stage2:
        return 'outer'
    return 'outer' if flags.outer else 'inner'


def output_paths(flags, name, step):
    """(mesh path, output directory) for config `name` at checkpoint `step`."""
    return (flags.mesh or os.path.join('data', 'meshes', f'{name}-{step}.ply'),
            flags.out or os.path.join('data', 'materials', f'{name}-{step}'))


def save_curvature(out, curv):
    """DIR/curvature.npy [V,1], mean_curvature.npy [V], sdf_normal.npy [V,3], float32 -> the three paths."""
    import numpy as np
    os.makedirs(out, exist_ok=True)
    shapes = {'gaussian': (-1, 1), 'mean': (-1,), 'normal': (-1, 3)}
    paths = []
    for k, fn in FILES.items():
        paths.append(os.path.join(out, fn))
        np.save(paths[-1], np.ascontiguousarray(curv[k], np.float32).reshape(shapes[k]))
    return paths


def report(curv, V, F):
    """The dict of the command's JSON line."""
    import torch
    from . import curvature as C
    from .lbvh import vertex_normals_and_curvature
    rep = {'V': int(len(V)), 'gauss_bonnet': None, 'sdf': C.curvature_stats(curv['gaussian']), 'angle_defect': None}
    if len(F):
        rep['gauss_bonnet'] = C.gauss_bonnet_ratio(curv['gaussian'], V, F)
        defect = vertex_normals_and_curvature(torch.from_numpy(V), torch.from_numpy(F))[1].numpy()
        rep['angle_defect'] = C.curvature_stats(defect)
    return rep


def main(argv=None):
    flags = parse_args(argv)
    import numpy as np
    import torch
    import yaml
    from . import mesh as M
    from .curvature import predict_curvature
    from .extract_mesh import _renderer
    from .train_glue import load_checkpoint

    with open(flags.cfg) as fh:
        cfg = yaml.safe_load(fh)
    network = _renderer(cfg)
    is_s2 = hasattr(network, 'stage1_network')
    if is_s2 != flags.stage2:
        raise SystemExit(f"config network {cfg['network']!r} is{'' if is_s2 else ' not'} a stage-2 model: "
                         f"{'pass' if is_s2 else 'drop'} --stage2")
    ckpt = flags.ckpt or f'data/model/{cfg["name"]}/model.pth'
    _, step = load_checkpoint(ckpt, network, map_location='cpu')
    if flags.stage2:
        s1_ckpt = network.cfg.get('stage1_ckpt_dir')
        if s1_ckpt and os.path.exists(s1_ckpt):                # as extract_mesh --stage2: stage 1 from its own checkpoint
            load_checkpoint(s1_ckpt, network.stage1_network, map_location='cpu')
    network = network.eval().to(torch.device('cuda', torch.cuda.current_device()))
    mesh_path, out = output_paths(flags, cfg['name'], step)
    V, F = M.read_ply(mesh_path)
    V, F = np.ascontiguousarray(V, np.float32), np.ascontiguousarray(F, np.int64)
    curv = predict_curvature(network, (V, F), which_of(flags))
    save_curvature(out, curv)
    print(json.dumps({'name': cfg['name'], 'step': int(step), 'mesh': mesh_path, 'out': out, **report(curv, V, F)}))
    return out


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
