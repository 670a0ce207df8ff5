"""The learned NeRF++ background of a set of rays, without the volume render.

Reference: color_bkgr of render_core (network/renderer_zerothick.py:757, :777-779) -- the front-to-back composite of a ray's samples
with every inner (|x| <= 1) alpha set to zero, i.e. what outer_nerf alone explains of the picture: the table, the room, and the fog it
places in front of the object.  In training this is a by-product of the layered path (nu_partition_* with its host read, nu_nerf_embed,
ten NT GEMMs, two skinny heads, nu_nerf_act_fwd, nu_composite_fwd: about 11 KB of workspace per outer row); here it is ONE launch of
the fused kernel of csrc/background.hip (nu_background_fwd) for any number of rays, with no workspace and no host read.  It is an fp32
evaluation in every `mlp_dtype`, like the other fused point kernels, and every sample carries the bits of the layered path.  The exact
per-ray arithmetic is stated at nu_background_fwd in include/nu_nerf.h.

default_nodes      rays -> z [R, n_samples + n_bg_samples]: the reference's sample_ray with perturb = 0 and no importance pass
render_background  rays (+ nodes, + a stop distance per ray) -> {'color' [R,3], 'transmittance' [R]}

A stage-2 renderer evaluates the outer_nerf of the stage-1 network it carries (its inner engine never has one).
"""
import torch

from . import _lib as L
from .sdf_trace import _check_rays

_NODE_SLICE = 1 << 17          # rays per nu_sample_coarse launch (it also writes the coarse positions, 12 n_samples bytes a ray)


def _fail(msg):
    raise L.NuNerfLibraryError(f"nu_background_fwd failed with code -1 (NU_ERR_ARG): {msg}")


def background_engine(renderer):
    """The HIP engine whose outer_nerf is the background: the renderer's own (stage 1) or the stage-1 engine of a stage-2 renderer."""
    s1 = getattr(renderer, 'stage1_network', None)
    return (s1 if s1 is not None else renderer).engine()


def _count(v, what, lo):
    if isinstance(v, bool) or int(v) != v or v < lo:
        _fail(f"{what} = {v!r}, expected an integer >= {lo}")
    return int(v)


def _per_ray(v, R, dev, what):
    """near / far / t_stop as a contiguous fp32 [R] device tensor ([R] or [R,1] accepted)."""
    if not torch.is_tensor(v) or v.dtype != torch.float32 or v.numel() != R or v.dim() > 2 or (v.dim() == 2 and v.shape[1] != 1):
        _fail(f"{what} must be a float32 tensor of shape [{R}] or [{R}, 1]")
    if not v.is_cuda or v.device != dev:
        _fail(f"{what} is not on the engine's GPU")
    return v.reshape(R).contiguous()


def _rays(renderer, rays_o, rays_d):
    rays_o, o_ld = _check_rays(rays_o, 'rays_o')
    rays_d, d_ld = _check_rays(rays_d, 'rays_d')
    R = rays_o.shape[0]
    if rays_d.shape[0] != R:
        _fail(f"{R} origins but {rays_d.shape[0]} directions")
    eng = background_engine(renderer)
    for what, x in (('rays_o', rays_o), ('rays_d', rays_d)):
        if not x.is_cuda or x.device != eng.dev:
            _fail(f"{what} is not on the engine's GPU")
    return eng, rays_o, o_ld, rays_d, d_ld, R


@torch.no_grad()
def default_nodes(renderer, rays_o, rays_d, near=None, far=None, n_samples=None, n_bg_samples=None):
    """The nodes of the reference's sample_ray (renderer_zerothick.py:572-612) with perturb = 0 and no importance pass:
    z [R, n_samples + n_bg_samples] = near + (far - near) linspace(0, 1, n_samples), then far / flip(linspace(1e-3, 1 - 1 / (n_bg + 1),
    n_bg)) + 1 / n_bg, by nu_sample_coarse.  near / far ([R] or [R,1]) default to near_far_from_sphere of the rays, the counts to the
    renderer's cfg."""
    eng, rays_o, _, rays_d, _, R = _rays(renderer, rays_o, rays_d)
    dev = eng.dev
    Nc = _count(eng.cfg['n_samples'] if n_samples is None else n_samples, 'n_samples', 1)
    Nbg = _count(eng.cfg['n_bg_samples'] if n_bg_samples is None else n_bg_samples, 'n_bg_samples', 1)
    o, d = rays_o[:, :3].contiguous(), rays_d[:, :3].contiguous()
    if near is None or far is None:
        nr, fr = renderer.near_far_from_sphere(o, d)
        near, far = (nr if near is None else near), (fr if far is None else far)
    near, far = _per_ray(near, R, dev, 'near'), _per_ray(far, R, dev, 'far')
    z = torch.empty(R, Nc + Nbg, dtype=torch.float32, device=dev)
    if R == 0:
        return z
    lin = torch.linspace(0.0, 1.0, Nc).to(dev)
    zo_lin = torch.linspace(1e-3, 1.0 - 1.0 / (Nbg + 1.0), Nbg).to(dev)          # u2 = NULL: `upper` is not read
    n = min(R, _NODE_SLICE)
    zc, zbg, X = (torch.empty(n, c, dtype=torch.float32, device=dev) for c in (Nc, Nbg, 3 * Nc))
    A, S = (lambda t: t.data_ptr()), eng.stream()
    for i in range(0, R, n):
        m = min(n, R - i)
        eng.lib.nu_sample_coarse(A(o[i:]), A(d[i:]), A(near[i:]), A(far[i:]), A(lin), A(zo_lin), A(zo_lin), 0, 0, m, Nc, Nbg, A(zc), A(zbg),
                                 A(X), S)
        eng.lib.nu_concat_cols(A(zc), Nc, A(zbg), Nbg, m, A(z[i:]), S)
    return z


@torch.no_grad()
def render_background(renderer, rays_o, rays_d, *, z=None, t_stop=None, near=None, far=None, n_samples=None, n_bg_samples=None,
                      _dbg=False):
    """The learned background along rays (rays_o, rays_d: [R, >= 3] float32 device tensors, rows contiguous and a fixed number of floats
    apart; the direction is used as given for the sample positions and normalised for the view) -> dict of device tensors
      'color' [R,3]         sum_j alpha_j T_j c_j over the outer (|x| > 1) samples in front of t_stop
      'transmittance' [R]   what is left behind them: prod_j (1 - alpha_j + 1e-7)
    z: ascending nodes [R, S] (None: default_nodes with near / far / n_samples / n_bg_samples).  t_stop: None or [R] float32 -- samples
    whose mid-point is not in front of it are dropped (+inf: none).  One kernel launch for any R.  _dbg: also the kernel's test
    outputs 'enc' [R S,128], 'raw' [R S,4], 'act' [R S,4]."""
    eng, rays_o, o_ld, rays_d, d_ld, R = _rays(renderer, rays_o, rays_d)
    dev = eng.dev
    if z is None:
        z = default_nodes(renderer, rays_o, rays_d, near, far, n_samples, n_bg_samples)
    else:
        if not torch.is_tensor(z) or z.dtype != torch.float32 or z.dim() != 2 or z.shape[0] != R or z.shape[1] < 1:
            _fail(f"z must be a float32 tensor of shape [{R}, >= 1]")
        if not z.is_cuda or z.device != dev:
            _fail("z is not on the engine's GPU")
        z = z.contiguous()
    if t_stop is not None:
        t_stop = _per_ray(t_stop, R, dev, 't_stop')
    S = z.shape[1]
    e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)      # noqa: E731
    out = {'color': e(R, 3), 'transmittance': e(R)}
    dbg = {'enc': e(R * S, 128), 'raw': e(R * S, 4), 'act': e(R * S, 4)} if _dbg else {}
    out.update(dbg)
    if R == 0:
        return out
    eng.pack()
    eng.background(rays_o.data_ptr(), o_ld, rays_d.data_ptr(), d_ld, z, R, t_stop=t_stop, color=out['color'], trans=out['transmittance'],
                   **dbg)
    return out
