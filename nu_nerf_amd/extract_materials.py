"""python -m nu_nerf_amd.extract_materials --cfg CFG [--mesh PLY] [--ckpt PATH] [--stage2] [--inner|--outer] [--out DIR] [--ply]

extract_materials.py on the GPU: the renderer named by the config loads data/model/{name}/model.pth (train_glue.save_checkpoint
format, as extract_mesh does), the materials are baked at the vertices of the mesh by one fused kernel (materials.bake_materials)
and DIR/metallic.npy [V,1], DIR/roughness.npy [V,1], DIR/albedo.npy [V,3] are written: float32, in the vertex order of the PLY --
the directory relight.py --material takes (blender_backend/relight_backend.py:26-28).

--mesh defaults to data/meshes/{name}-{step}.ply, the file extract_mesh writes for the same checkpoint; --out to
data/materials/{name}-{step}.  --stage2: a stage-2 config; --inner (default) bakes the inner networks, --outer the stage-1 networks
the stage-2 model carries; both also write DIR/ior.npy [V_outer,1], the learned index of refraction at the vertices of the outer
shell (materials.predict_ior) that relight --ior DIR takes.  With --inner the shell is the stage-1 mesh of the config
(stage1_mesh_dir), NOT --mesh: ior.npy is in that file's vertex order, and that same file is what relight --mesh must be given
(relight checks the vertex count only).  A `zero_thickness: false` config (the thin-shell model) additionally gets DIR/shell_ior.npy
and DIR/shell_thickness.npy [V_outer,1] (materials.predict_shell), the directory relight --shell DIR takes.  --ply also writes DIR/{mesh stem}_albedo.ply: the mesh with the albedo as uint8 vertex colours.
"""
import argparse
import os
import sys


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.extract_materials", description=__doc__.split("\n\n")[1])
    ap.add_argument('--cfg', type=str, required=True, help="training config (YAML)")
    ap.add_argument('--mesh', type=str, default=None, help="mesh whose vertices are baked (default data/meshes/{name}-{step}.ply)")
    ap.add_argument('--ckpt', type=str, default=None, help="checkpoint (default data/model/{name}/model.pth)")
    ap.add_argument('--stage2', action='store_true', help="the config is a stage-2 config")
    side = ap.add_mutually_exclusive_group()
    side.add_argument('--inner', action='store_true', help="stage 2: the inner networks (default)")
    side.add_argument('--outer', action='store_true', help="stage 2: the stage-1 networks of the stage-2 model")
    ap.add_argument('--out', type=str, default=None, help="output directory (default data/materials/{name}-{step})")
    ap.add_argument('--ply', action='store_true', help="also write {mesh stem}_albedo.ply with the albedo as vertex colours")
    flags = ap.parse_args(argv)
    if (flags.inner or flags.outer) and not flags.stage2:
        ap.error("--inner / --outer need --stage2")
    return flags


def which_of(flags):
    """The `which` of materials.bake_materials the flags ask for."""
    if not flags.stage2:
        return 'outer'
    return 'outer' if flags.outer else 'inner'


def output_paths(flags, name, step):
    """(mesh path, output directory, albedo PLY path or None) for config `name` at checkpoint `step`."""
    mesh = flags.mesh or os.path.join('data', 'meshes', f'{name}-{step}.ply')
    out = flags.out or os.path.join('data', 'materials', f'{name}-{step}')
    stem = os.path.splitext(os.path.basename(mesh))[0]
    return mesh, out, (os.path.join(out, stem + '_albedo.ply') if flags.ply else None)


def ior_mesh(flags, network, baked):
    """The mesh whose vertices get an index of refraction: the outer shell.  --outer bakes that mesh, so it is `baked`; otherwise the
    stage-1 mesh the stage-2 model refracts through."""
    return baked if flags.outer else network._mesh


def save_ior(out, ior):
    """DIR/ior.npy [V,1] float32: what relight --ior DIR reads."""
    import numpy as np
    ior = np.ascontiguousarray(ior, np.float32).reshape(-1, 1)
    np.save(os.path.join(out, 'ior.npy'), ior)
    return os.path.join(out, 'ior.npy')


def save_shell(out, shell):
    """DIR/shell_ior.npy, DIR/shell_thickness.npy [V,1] float32: what relight --shell DIR reads."""
    import numpy as np
    paths = []
    for k in ('ior', 'thickness'):
        paths.append(os.path.join(out, f'shell_{k}.npy'))
        np.save(paths[-1], np.ascontiguousarray(shell[k], np.float32).reshape(-1, 1))
    return paths


def main(argv=None):
    flags = parse_args(argv)
    import numpy as np
    import torch
    import yaml
    from . import mesh as M
    from .extract_mesh import _renderer
    from .materials import is_thick_stage2, predict_ior, predict_materials, predict_shell
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
    print(f'successfully load {cfg["name"]} step {step}!')
    mesh_path, out, ply_path = output_paths(flags, cfg['name'], step)
    V, F = M.read_ply(mesh_path)
    mats = predict_materials(network, (V, F), which_of(flags))
    os.makedirs(out, exist_ok=True)
    for k in ('metallic', 'roughness', 'albedo'):
        np.save(os.path.join(out, k + '.npy'), mats[k].astype(np.float32))
    print(f'wrote {out}/metallic.npy, roughness.npy, albedo.npy: {len(V)} vertices of {mesh_path}')
    if flags.stage2:
        shell_mesh = ior_mesh(flags, network, (V, F))
        save_ior(out, predict_ior(network, shell_mesh))
        print(f'wrote {out}/ior.npy')
        if is_thick_stage2(network):                         # the non-zero-thickness model: the shell relight --shell takes
            save_shell(out, predict_shell(network, shell_mesh))
            print(f'wrote {out}/shell_ior.npy, shell_thickness.npy')
    if ply_path:
        M.write_ply(ply_path, V, F, colors=mats['albedo'])
        print(f'wrote {ply_path}')
    return out


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
