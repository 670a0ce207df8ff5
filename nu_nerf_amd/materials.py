"""Per-vertex material baking: the relightable asset of a trained model (mesh + metallic / roughness / albedo per vertex).

Reference: `predict_materials()` of every renderer class (network/renderer_zerothick.py:846-864, :2037-2055; network/renderer.py:885,
:2379): feature = sdf_network(x)[:, 1:], color_network.predict_materials(x, feature) (network/field.py:779-783) over the vertices of
data/meshes/{name}-300000.ply in chunks of 8192 -> {'metallic' [V,1], 'roughness' [V,1], 'albedo' [V,3]}; relight.py /
blender_backend/relight_backend.py:26-28 read them as <material>/metallic.npy, roughness.npy, albedo.npy, indexed by vertex id.

Here the whole evaluation is ONE launch of the fused kernel of csrc/bake.hip (nu_material_bake_fwd) for any vertex count: no chunk
loop, no workspace.  It is an fp32 evaluation in every `mlp_dtype`: pack() writes the fp32 packed weight tables also on a
bf16-storage ('bf16') or 'bf16x6' engine, and the kernel reads those.

Stage 2: the reference's method names `self.sdf_network`, which its Stage2Renderer never sets (the attribute exists only on the
stage-1 class), so the call raises there.  Defined usefully instead: which='inner' (the default for a stage-2 renderer) bakes
sdf_network_inner + color_network_inner, which='outer' the stage-1 networks the stage-2 model carries.
"""
import os

import numpy as np
import torch

from . import _lib as L

WHICH = ('outer', 'inner')


def _is_stage2(renderer):
    return hasattr(renderer, 'stage1_network') and hasattr(renderer, 'sdf_network_inner')


def _resolve_which(renderer, which):
    if which is None:
        which = 'inner' if _is_stage2(renderer) else 'outer'
    if which not in WHICH:
        raise ValueError(f"which={which!r}: expected 'outer' or 'inner'")
    if which == 'inner' and not _is_stage2(renderer):
        raise ValueError("which='inner': a stage-1 renderer has no inner networks")
    return which


def bake_engine(renderer, which=None):
    """The HIP engine holding the packed SDF + material networks to bake: the renderer's own (stage 1), the stage-1 engine of a
    stage-2 renderer (which='outer') or its inner engine (which='inner', the stage-2 default)."""
    which = _resolve_which(renderer, which)
    if not _is_stage2(renderer):
        return renderer.engine()
    if which == 'outer':
        return renderer.stage1_network.engine()
    return renderer.nets()[1].eng


def _check_points(points, dev):
    if not torch.is_tensor(points):
        points = torch.as_tensor(np.ascontiguousarray(points, dtype=np.float32)).to(dev)
    bad = None
    if not points.is_cuda:
        bad = "not on the GPU"
    elif points.dtype != torch.float32:
        bad = f"dtype {points.dtype}, expected float32"
    elif points.dim() != 2 or points.shape[1] < 3:
        bad = f"shape {tuple(points.shape)}, expected [V, >= 3]"
    elif not points.is_contiguous():
        bad = "not contiguous"
    if bad:
        raise L.NuNerfLibraryError(f"nu_material_bake_fwd failed with code -1 (NU_ERR_ARG): points are {bad}")
    return points


@torch.no_grad()
def bake_materials(renderer, points, *, which=None, transmission=False, sdf=False, _feat=False, _raw=False):
    """Materials at `points` ([V, >= 3] float32 device tensor, contiguous; the first three columns are x) -> dict of device tensors
    'metallic' [V,1], 'roughness' [V,1], 'albedo' [V,3] (the reference's shapes), plus 'transmission' [V,1] and 'sdf' [V] on request.
    One kernel launch for any V.  which: see bake_engine.  _feat / _raw: the kernel's test outputs ('feature' [V,256]; heads before
    the sigmoid)."""
    eng = bake_engine(renderer, which)
    points = _check_points(points, eng.dev)
    V = points.shape[0]
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=eng.dev)      # noqa: E731
    out = {'metallic': e(V, 1), 'roughness': e(V, 1), 'albedo': e(V, 3)}
    if transmission:
        out['transmission'] = e(V, 1)
    if sdf:
        out['sdf'] = e(V)
    if _feat:
        out['feature'] = e(V, 256)
    if V == 0:
        return out
    eng.pack()
    eng.material_bake(points.data_ptr(), points.shape[1], V, out['metallic'], out['roughness'], out['albedo'],
                      out.get('transmission'), out.get('sdf'), out.get('feature'), raw=_raw)
    return out


def mesh_vertices(renderer, mesh=None):
    """Vertices [V,3] float32 of `mesh`: None = data/meshes/{name}-300000.ply like the reference, a PLY path, or a (V, F) pair."""
    if mesh is None:
        mesh = os.path.join('data', 'meshes', f"{renderer.cfg['name']}-300000.ply")
    if isinstance(mesh, (str, os.PathLike)):
        from .mesh import read_ply
        return read_ply(mesh)[0]
    V = mesh[0]
    V = V.detach().cpu().numpy() if torch.is_tensor(V) else np.asarray(V)
    return np.ascontiguousarray(V, dtype=np.float32).reshape(-1, 3)


def predict_materials(renderer, mesh=None, which=None):
    """The reference's predict_materials(): {'metallic' [V,1], 'roughness' [V,1], 'albedo' [V,3]} as float32 numpy arrays in the
    vertex order of the mesh."""
    V = mesh_vertices(renderer, mesh)
    dev = next(renderer.parameters()).device
    out = bake_materials(renderer, torch.from_numpy(V).to(dev), which=which)
    return {k: out[k].cpu().numpy() for k in ('metallic', 'roughness', 'albedo')}


@torch.no_grad()
def predict_ior(renderer, mesh=None):
    """Per-vertex index of refraction [V,1] float32 (numpy) of the OUTER mesh of a stage-2 model, in the vertex order of `mesh` (as
    mesh_vertices reads it): the IoR network as the stage-2 light paths evaluate it (stage2.trace_segments: sigmoid of the network on
    the 6-frequency embedding of the point), turned into the physical index exactly as the refraction kernel does
    (s2_refract_fwd_kernel: eta = 1 / (ior * 1 + 1) entering from air), i.e. index = sigmoid(net(x)) + 1, in (1, 2).  This is what
    relight --ior takes."""
    if not _is_stage2(renderer):
        raise ValueError("predict_ior: only a stage-2 renderer has an index-of-refraction network")
    from . import torch_glue as G
    V = mesh_vertices(renderer, mesh)
    dev = next(renderer.parameters()).device
    x = torch.from_numpy(V).to(dev)
    if x.shape[0] == 0:
        return np.zeros((0, 1), np.float32)
    raw = torch.sigmoid(renderer.nets()[1].ior(G.embed(x, 6)))
    return (raw.reshape(-1, 1) * 1.0 + 1.0).cpu().numpy().astype(np.float32)


def is_thick_stage2(renderer):
    """True for the non-zero-thickness stage-2 renderer (the zero-thickness class carries an unused thickness network too, so the
    class decides)."""
    from .stage2_thick import Stage2Renderer
    return isinstance(renderer, Stage2Renderer)


@torch.no_grad()
def predict_shell(renderer, mesh=None):
    """The shell of the NON-zero-thickness stage-2 model (stage2_thick.Stage2Renderer) at the vertices of the OUTER mesh, in the vertex
    order of `mesh` (as mesh_vertices reads it): {'ior' [V,1], 'thickness' [V,1]} float32 numpy.  The two networks exactly as
    stage2_thick.trace_segments evaluates them (nets.ior_and_thickness on the 6-frequency embedding of the point) and the mapping of
    the crossing (s2_shell_core): glass index = sigmoid(raw) + 0.6 in (0.6, 1.6), wall thickness = 0.01 * sigmoid(raw).  This is what
    relight --shell takes; predict_ior stays the zero-thickness formula."""
    if not is_thick_stage2(renderer):
        raise ValueError("predict_shell: only the non-zero-thickness stage-2 renderer has a shell of learned index and thickness")
    from . import torch_glue as G
    V = mesh_vertices(renderer, mesh)
    dev = next(renderer.parameters()).device
    x = torch.from_numpy(V).to(dev)
    if x.shape[0] == 0:
        return {'ior': np.zeros((0, 1), np.float32), 'thickness': np.zeros((0, 1), np.float32)}
    inner = renderer.nets()[1]
    inner.eng.pack()                   # the packed weight tables the GEMMs read, as every render pass refreshes them first
    ior_raw, thick_raw = inner.ior_and_thickness(G.embed(x, 6))
    ior = torch.sigmoid(ior_raw).reshape(-1, 1) * 1.0 + 0.6
    thickness = torch.sigmoid(thick_raw).reshape(-1, 1) * 0.01
    return {'ior': ior.cpu().numpy().astype(np.float32), 'thickness': thickness.cpu().numpy().astype(np.float32)}
