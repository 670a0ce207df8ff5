"""python -m nu_nerf_amd.bake_textures --cfg CFG [--mesh PLY] [--ckpt PATH] [--size N] [--pad N] [--stage2 --which inner|outer] [--out DIR]
[--decimate N] [--normals sdf]

The materials of a trained model baked into a texture atlas instead of per vertex: the renderer named by the config
loads data/model/{name}/model.pth as extract_materials does, every face of the mesh gets its own triangle of a SIZE x SIZE atlas
(texture.atlas_layout), the material networks are evaluated at the surface point of every owned texel by the fused bake kernel, and
DIR gets
    atlas.npz              albedo [T,T,3], metallic, roughness [T,T] float32, face [T,T] int32, uv [Nf,3,2], size, n_faces, pad
                           -- what relight --texture DIR reads
    albedo.png, orm.png    8-bit textures: sRGB albedo; linear R = 255, G = roughness, B = metallic
    {mesh stem}.obj, .mtl  the mesh with texture coordinates, map_Kd / map_Pr / map_Pm
    {mesh stem}.gltf, .bin glTF 2.0 with baseColorTexture and metallicRoughnessTexture

--mesh defaults to data/meshes/{name}-{step}.ply, --out to data/materials/{name}-{step}/texture.  --size (default 2048) must give every
face a cell of at least 5 + 3 PAD texels; --pad adds texels of margin around every triangle.  --stage2: a stage-2 config; --which inner
(default) bakes the inner networks, outer the stage-1 networks the stage-2 model carries.  --decimate N: the mesh is first brought down
to N faces (decimate.decimate), DIR also gets {mesh stem}_decimated.ply -- the mesh relight --texture DIR needs -- and the
atlas and the exports are built on it, under that stem.  --normals sdf: the SDF's unit normal at every owned texel is
baked as well (one more fused kernel per pass): atlas.npz gains normal [T,T,3] (object space; relight --texture DIR --normal-map shades
with it), DIR gets normal.png (tangent space, per-face flat frames) and the glTF names it as normalTexture with NORMAL / TANGENT to
match; the JSON line printed at the end counts the texels whose normal faces away from their face (normal_backfacing).  The OBJ is unchanged.
"""
import argparse
import os
import sys


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.bake_textures", description=__doc__.split("\n\n")[1])
    ap.add_argument('--cfg', type=str, required=True, help="training config (YAML)")
    ap.add_argument('--mesh', type=str, default=None, help="mesh whose faces are baked (default data/meshes/{name}-{step}.ply)")
    ap.add_argument('--ckpt', type=str, default=None, help="checkpoint (default data/model/{name}/model.pth)")
    ap.add_argument('--size', type=int, default=2048, help="texels a side of the square atlas")
    ap.add_argument('--pad', type=int, default=0, help="further texels of margin around every face's triangle")
    ap.add_argument('--stage2', action='store_true', help="the config is a stage-2 config")
    ap.add_argument('--which', choices=('inner', 'outer'), default=None, help="stage 2: the inner networks (default) or the stage-1 networks")
    ap.add_argument('--out', type=str, default=None, help="output directory (default data/materials/{name}-{step}/texture)")
    ap.add_argument('--decimate', type=int, default=None, metavar='N', help="decimate the mesh to N faces before baking")
    ap.add_argument('--normals', choices=('sdf',), default=None, help="also bake a normal map: sdf = the SDF network's normal at every texel")
    flags = ap.parse_args(argv)
    if flags.decimate is not None and flags.decimate < 4:
        ap.error("--decimate must be >= 4")
    if flags.which is not None and not flags.stage2:
        ap.error("--which needs --stage2")
    if flags.size < 1:
        ap.error("--size must be >= 1")
    from .texture import MAX_PAD, MAX_SIZE
    if flags.size > MAX_SIZE:
        ap.error(f"--size must be <= {MAX_SIZE}")
    if not 0 <= flags.pad <= MAX_PAD:
        ap.error(f"--pad must be in 0..{MAX_PAD}")
    return flags


def which_of(flags):
    """The `which` of materials.bake_materials the flags ask for."""
    if not flags.stage2:
        return 'outer'
    return flags.which or 'inner'


def output_paths(flags, name, step):
    """(mesh path, output directory, file stem of the OBJ / glTF pair) for config `name` at checkpoint `step`."""
    mesh = flags.mesh or os.path.join('data', 'meshes', f'{name}-{step}.ply')
    out = flags.out or os.path.join('data', 'materials', f'{name}-{step}', 'texture')
    return mesh, out, os.path.splitext(os.path.basename(mesh))[0]


def main(argv=None):
    flags = parse_args(argv)
    import torch
    import yaml
    from . import mesh as M
    from . import texture as T
    from .extract_mesh import _renderer
    from .lbvh import vertex_normals_and_curvature
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
        if s1_ckpt and os.path.exists(s1_ckpt):                # as extract_materials --stage2: stage 1 from its own checkpoint
            load_checkpoint(s1_ckpt, network.stage1_network, map_location='cpu')
    network = network.eval().to(torch.device('cuda', torch.cuda.current_device()))
    print(f'successfully load {cfg["name"]} step {step}!')
    mesh_path, out, stem = output_paths(flags, cfg['name'], step)
    V, F = M.read_ply(mesh_path)
    if flags.decimate is not None:
        V, F = M.decimate(V, F, flags.decimate)
        stem += '_decimated'
        os.makedirs(out, exist_ok=True)
        M.write_ply(os.path.join(out, stem + '.ply'), V, F)
        print(f'wrote {os.path.join(out, stem + ".ply")}: {len(V)} vertices, {len(F)} triangles')
    try:
        T.atlas_layout(len(F), flags.size, flags.pad)
    except ValueError as e:
        raise SystemExit(str(e))
    atlas = T.bake_textures(network, V, F, size=flags.size, pad=flags.pad, which=which_of(flags), normals=flags.normals)
    T.write_textures(out, atlas)
    normals = vertex_normals_and_curvature(torch.from_numpy(V), torch.from_numpy(F).long())[0].numpy()
    T.write_obj(os.path.join(out, stem + '.obj'), V, F, atlas['uv'], normals, out)
    T.write_gltf(os.path.join(out, stem + '.gltf'), V, F, atlas['uv'], normals, out, normal_map=atlas if flags.normals else None)
    owned = int((atlas['face'] >= 0).sum())
    print(f'wrote {out}/atlas.npz, albedo.png, orm.png, {stem}.obj, {stem}.mtl, {stem}.gltf, {stem}.bin: {len(F)} faces of {mesh_path} in '
          f'{flags.size} x {flags.size} texels, {owned} owned ({100.0 * owned / flags.size ** 2:.1f} %)')
    if flags.normals:
        import json
        backfacing = T.tangent_normal_image(atlas, V, F, count=True)[1]
        print(json.dumps({'normals': flags.normals, 'normal_png': os.path.join(out, 'normal.png'), 'owned_texels': owned,
                          'normal_backfacing': backfacing}))
    return out


if __name__ == "__main__":
    sys.exit(0 if main() else 1)
