"""Test-side restatement of the learned NeRF++ background (nu_nerf_amd/background.py, csrc/background.hip).

background(params, o, d, z, t_stop): color_bkgr of the reference's render_core (network/renderer_zerothick.py:757, :777-779) for rays
with their own nodes, with the kernel's stop test added.  The sample geometry -- section lengths, mid-points, positions and the
inner / live decision -- is formed with fp32 torch eager ops (each one separately rounded, as the reference forms them and as
nu_sample_point states them), so that the SET of samples the network sees is the kernel's; everything behind that decision is float64
over oracle/stage1_oracle.nerf_forward.
default_nodes(...): sample_ray with perturb = 0 and no importance pass, in fp32 torch."""
import torch
import torch.nn.functional as F

from oracle import stage1_oracle as O


def sample_geometry(o, d, z, t_stop=None):
    """fp32: (x [R,S,3], dist [R,S], mid [R,S], inner [R,S] bool, live [R,S] bool)."""
    o, d, z = o.float(), d.float(), z.float()
    S = z.shape[1]
    if S >= 2:
        dist = z[:, 1:] - z[:, :-1]
        dist = torch.cat([dist, dist[:, -1:]], -1)
    else:
        dist = torch.zeros_like(z)
    mid = z + dist * 0.5
    x = o[:, None, :] + d[:, None, :] * mid[..., None]
    sq = x * x
    inner = torch.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2]) <= 1.0
    live = ~inner
    if t_stop is not None:
        live = live & (mid < t_stop.float().reshape(-1, 1))
    return x, dist, mid, inner, live


def background(params, o, d, z, t_stop=None, full=False):
    """-> (color [R,3], transmittance [R]) float64 (full=True: also alpha [R,S], colour [R,S,3], live [R,S])."""
    p64 = {k: v.detach().double() for k, v in params.items() if k.startswith('outer_nerf.')}
    x, dist, _, _, live = sample_geometry(o, d, z, t_stop)
    R, S = z.shape
    alpha = torch.zeros(R, S, dtype=torch.float64)
    color = torch.zeros(R, S, 3, dtype=torch.float64)
    if live.any():
        du = F.normalize(d.double(), dim=-1)[:, None, :].expand(R, S, 3)
        xl = x.double()[live]
        n = torch.norm(xl, dim=-1, keepdim=True)
        sigma, rgb = O.nerf_forward(p64, torch.cat([xl / n, 1.0 / n], -1), -du[live])
        a = 1.0 - torch.exp(-F.softplus(sigma[..., 0]) * dist.double()[live])
        c = O.linear_to_srgb(torch.exp(torch.clamp(rgb, max=5.0)))
        alpha = alpha.index_put((live,), a)
        color = color.index_put((live,), c)
    T = torch.cumprod(torch.cat([torch.ones(R, 1, dtype=torch.float64), 1.0 - alpha + 1e-7], -1), -1)
    col = (color * (alpha * T[:, :-1])[..., None]).sum(1)
    if full:
        return col, T[:, -1], alpha, color, live
    return col, T[:, -1]


def default_nodes(o, d, near, far, n_samples, n_bg_samples):
    """fp32 [R, n_samples + n_bg_samples]: renderer_zerothick.py:572-612 with perturb = 0, without the up-sampling rounds."""
    near, far = near.float().reshape(-1, 1), far.float().reshape(-1, 1)
    z = near + (far - near) * torch.linspace(0.0, 1.0, n_samples, device=near.device)[None, :]
    zo = torch.linspace(1e-3, 1.0 - 1.0 / (n_bg_samples + 1.0), n_bg_samples, device=near.device)
    zo = far / torch.flip(zo, dims=[-1])[None, :] + 1.0 / n_bg_samples
    return torch.cat([z, zo], -1)
