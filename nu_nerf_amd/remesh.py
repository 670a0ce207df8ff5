"""Isotropic explicit remeshing on the GPU (Botsch & Kobbelt 2004): the stage-1 -> stage-2 step the reference does with pymeshlab's
meshing_isotropic_explicit_remeshing(maxsurfdist=0.5 %, targetlen=0.5 %) in extract_mesh_stage1.py:44-50, because a raw
marching-cubes mesh has slivers and a poor discrete curvature (lbvh.Scene's angle-defect curvature drives stage2_thick's shells).

python -m nu_nerf_amd.remesh IN.ply [--out OUT] [--target-len-pct 0.5] [--max-surf-dist-pct 0.5] [--iterations 3]
writes IN_simplified.ply next to the input unless --out is given.

One iteration with target length L (kernels: csrc/remesh.hip):
  split     every unlocked edge longer than 4/3 L at its midpoint (fixed per-face templates, placed by scans)
  collapse  rounds of independent edge collapses of edges shorter than 4/5 L (link condition, no edge above 4/3 L, no flipped or
            zero-area face, every rewritten face within max_surf_dist of the input), until a round has no winner or
            MAX_COLLAPSE_ROUNDS; then the dead faces and unreferenced vertices are dropped
  flip      rounds of independent valence-lowering edge flips (normal turn <= FLIP_MAX_NORMAL_ANGLE_DEG, surface distance), up to
            MAX_FLIP_ROUNDS
  relax     tangential relaxation of every unlocked vertex, then projection onto the input (LBVH closest points)
Edges on a boundary or non-manifold edge are locked, and so are their vertices: never split, collapsed, flipped or moved.
Every step runs on the caller's current stream; the host reads only counts (one read per pass or round); two calls give the same
bits.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

from . import _lib as L

MAX_COLLAPSE_ROUNDS = 64          # collapse rounds per pass (each round is an independent set of collapses)
MAX_FLIP_ROUNDS = 32              # flip rounds per pass
FLIP_MAX_NORMAL_ANGLE_DEG = 30.0  # largest angle a flip may turn a face normal by
SPLIT_FACTOR = 4.0 / 3.0          # split edges longer than 4/3 L
COLLAPSE_FACTOR = 4.0 / 5.0       # collapse edges shorter than 4/5 L
DEFAULT_PCT = 0.5                 # target length and surface distance: 0.5 % of the bounding-box diagonal (the reference's values)


def _f32(x):
    """float64 value rounded once to fp32 (as a Python float)."""
    return float(np.float32(x))


def _lib():
    return L.load()


def _p(t):
    return t.data_ptr()


class Tables:
    """Edge table and vertex -> corner CSR of (V, F) (csrc/remesh.hip): E [3 nf, 4], he_edge, vc_off, vc_corner, vlock, vbound."""

    def __init__(self, V, F):
        lib = _lib()
        S = L.stream(V.device.index)
        self.V, self.F = V, F
        self.nv, self.nf = int(V.shape[0]), int(F.shape[0])
        nh = 3 * self.nf
        dev = V.device
        keys = torch.empty(nh, dtype=torch.int64, device=dev)
        lib.nu_rm_edge_keys(_p(F), self.nf, _p(keys), S)
        skeys, perm = torch.sort(keys, stable=True)
        self.E = torch.empty(nh, 4, dtype=torch.int32, device=dev)
        self.he_edge = torch.empty(nh, dtype=torch.int32, device=dev)
        self.vlock = torch.empty(self.nv, dtype=torch.uint8, device=dev)
        self.vbound = torch.empty(self.nv, dtype=torch.uint8, device=dev)
        lib.nu_rm_edges(_p(F), self.nf, self.nv, _p(skeys), _p(perm), _p(self.E), _p(self.he_edge), _p(self.vlock), _p(self.vbound), S)
        svid, cperm = torch.sort(F.reshape(-1), stable=True)
        self.vc_off = torch.searchsorted(svid, torch.arange(self.nv + 1, dtype=torch.int32, device=dev)).to(torch.int32)
        self.vc_corner = cperm.to(torch.int32)

    def args(self):
        return (_p(self.V), self.nv, _p(self.F), self.nf, _p(self.E), _p(self.he_edge), _p(self.vc_off), _p(self.vc_corner),
                _p(self.vlock), _p(self.vbound))


def split(V, F, max_len2):
    """-> (V', F', number of split edges): the split pass on a compact mesh."""
    lib = _lib()
    S = L.stream(V.device.index)
    T = Tables(V, F)
    nh = 3 * T.nf
    eflag = torch.empty(nh, dtype=torch.int32, device=V.device)
    fcnt = torch.empty(T.nf, dtype=torch.int32, device=V.device)
    lib.nu_rm_split_count(_p(V), _p(F), T.nf, _p(T.E), _p(T.he_edge), max_len2, _p(eflag), _p(fcnt), S)
    vinc, finc = torch.cumsum(eflag, 0), torch.cumsum(fcnt, 0)
    ns, nfo = (int(x) for x in torch.stack([vinc[-1], finc[-1]]).cpu())      # the pass's one host read
    if ns == 0:
        return V, F, 0
    Vo = torch.empty(T.nv + ns, 3, dtype=torch.float32, device=V.device)
    Fo = torch.empty(nfo, 3, dtype=torch.int32, device=V.device)
    voff, foff = vinc - eflag, finc - fcnt          # named: a temporary would be freed before the kernel reads it
    lib.nu_rm_split_write(_p(V), T.nv, _p(F), T.nf, _p(T.E), _p(T.he_edge), _p(eflag), _p(voff), _p(foff), _p(Vo), _p(Fo), S)
    return Vo, Fo, ns


class _Round:
    """Candidates of one collapse (kind 'collapse', params (min_len2, max_len2)) or flip (kind 'flip', params (cos2_max,)) round."""

    def __init__(self, kind, V, F, params):
        self.lib = _lib()
        self.S = L.stream(V.device.index)
        self.kind, self.params = kind, params
        self.T = Tables(V, F)
        nh = 3 * self.T.nf
        self.npts = torch.empty(nh, dtype=torch.int32, device=V.device)
        fn = getattr(self.lib, f"nu_rm_{kind}_count")
        fn(*self.T.args(), *params, _p(self.npts), self.S)
        self.inc = torch.cumsum(self.npts, 0)

    def winners(self, total, bvh, max_d2):
        """win [3 nf] int32 (1 at each winning edge id) after the surface-distance check of `total` query points."""
        T, dev = self.T, self.T.V.device
        nh = 3 * T.nf
        poff = self.inc - self.npts
        pts = torch.empty(max(total, 1), 3, dtype=torch.float32, device=dev)
        getattr(self.lib, f"nu_rm_{self.kind}_points")(*T.args(), *self.params, _p(self.npts), _p(poff), _p(pts), self.S)
        d2 = torch.empty(total, dtype=torch.float32, device=dev)
        idx = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        if total > 0:
            self.lib.nu_lbvh_closest(_p(bvh.buf), bvh.n_faces, _p(pts), total, max_d2, _p(d2), _p(idx), None, self.S)
        ckey = torch.empty(nh, dtype=torch.int64, device=dev)
        claim = torch.empty(T.nv, dtype=torch.int64, device=dev)
        win = torch.empty(nh, dtype=torch.int32, device=dev)
        extra = self.params[:1] if self.kind == 'flip' else ()
        getattr(self.lib, f"nu_rm_{self.kind}_claim")(*T.args(), *extra, _p(self.npts), _p(poff),
                                                      _p(idx), _p(ckey), _p(claim), _p(win), self.S)
        return win

    def apply(self, win):
        T = self.T
        if self.kind == 'collapse':
            self.lib.nu_rm_collapse_apply(*T.args(), _p(win), _p(T.V), _p(T.F), self.S)
        else:
            self.lib.nu_rm_flip_apply(*T.args(), _p(win), _p(T.F), self.S)


def _rounds(kind, V, F, params, bvh, max_d2, max_rounds):
    """Rounds of `kind` on (V, F) in place until a round has no winner or max_rounds; -> rounds with winners.  One host read per
    round: the number of query points of its candidates, together with the previous round's winner count."""
    rnd = _Round(kind, V, F, params)
    total = int(rnd.inc[-1])
    rounds = 0
    while total > 0 and rounds < max_rounds:
        win = rnd.winners(total, bvh, max_d2)
        rnd.apply(win)
        nwin = win.sum()
        rnd = _Round(kind, V, F, params)
        total, nwin = (int(x) for x in torch.stack([rnd.inc[-1], nwin]).cpu())
        if nwin == 0:
            break
        rounds += 1
    return rounds


def compact(V, F):
    """Drop dead faces (-1 rows) and unreferenced vertices, both kept in order."""
    Fk = F[F[:, 0] >= 0]
    used = torch.zeros(V.shape[0], dtype=torch.bool, device=V.device)
    used[Fk.reshape(-1).long()] = True
    remap = torch.cumsum(used, 0, dtype=torch.int32) - 1
    return V[used].contiguous(), remap[Fk.long()].contiguous()


def collapse(V, F, min_len2, max_len2, bvh, max_d2, max_rounds=MAX_COLLAPSE_ROUNDS):
    """-> (V', F' compacted, rounds)."""
    V, F = V.clone(), F.clone()
    rounds = _rounds('collapse', V, F, (min_len2, max_len2), bvh, max_d2, max_rounds)
    V, F = compact(V, F)
    return V, F, rounds


def flip(V, F, cos2_max, bvh, max_d2, max_rounds=MAX_FLIP_ROUNDS):
    """-> (V, F', rounds)."""
    F = F.clone()
    rounds = _rounds('flip', V, F, (cos2_max,), bvh, max_d2, max_rounds)
    return V, F, rounds


def relax(V, F, T=None):
    """Tangential relaxation (Jacobi) of every unlocked vertex.  T: the Tables of (V, F), when the caller has them."""
    T = T or Tables(V, F)
    out = torch.empty_like(V)
    _lib().nu_rm_relax(*T.args(), _p(out), L.stream(V.device.index))
    return out


def project(V, F, bvh, T=None):
    """Every unlocked vertex onto the input surface (its LBVH closest point).  T: Tables of the same faces (only vlock is read)."""
    T = T or Tables(V, F)
    nv = T.nv
    d2 = torch.empty(nv, dtype=torch.float32, device=V.device)
    idx = torch.empty(nv, dtype=torch.int32, device=V.device)
    q = torch.empty(nv, 3, dtype=torch.float32, device=V.device)
    out = torch.empty_like(V)
    lib, S = _lib(), L.stream(V.device.index)
    lib.nu_lbvh_closest(_p(bvh.buf), bvh.n_faces, _p(V), nv, math.inf, _p(d2), _p(idx), _p(q), S)
    lib.nu_rm_project(_p(V), nv, _p(T.vlock), _p(q), _p(out), S)
    return out


def thresholds(target_len, max_surf_dist):
    """(max_len2, min_len2, max_d2, cos2_max) as fp32 values: squares in float64, rounded once."""
    L_ = float(target_len)
    return (_f32((SPLIT_FACTOR * L_) ** 2), _f32((COLLAPSE_FACTOR * L_) ** 2), _f32(float(max_surf_dist) ** 2),
            _f32(math.cos(math.radians(FLIP_MAX_NORMAL_ANGLE_DEG)) ** 2))


def _validate(V, F, who="remesh_isotropic"):
    from .lbvh import EmptyMeshError
    if V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3:
        raise ValueError(f"{who}: V must be [Nv,3] and F [Nf,3], got {tuple(V.shape)} and {tuple(F.shape)}")
    if len(F) == 0 or len(V) == 0:
        raise EmptyMeshError(f"{who}: the mesh has no triangles")
    if 3 * len(F) >= 2 ** 31 or len(V) >= 2 ** 31:
        raise ValueError(f"{who}: the mesh is too large for int32 half-edge ids")
    bad = torch.stack([(F < 0).any() | (F >= len(V)).any(),
                       ((F[:, 0] == F[:, 1]) | (F[:, 1] == F[:, 2]) | (F[:, 2] == F[:, 0])).any(),
                       ~torch.isfinite(V).all()]).cpu().tolist()
    if bad[0]:
        raise ValueError(f"{who}: face index out of range")
    if bad[1]:
        raise ValueError(f"{who}: a face repeats a vertex")
    if bad[2]:
        raise ValueError(f"{who}: vertices must be finite")


@torch.no_grad()
def remesh_isotropic(V, F, target_len=None, max_surf_dist=None, iterations=3, stats=None):
    """Isotropic explicit remeshing of the triangle mesh (V [Nv,3], F [Nf,3]) on the GPU.  target_len and max_surf_dist default
    to 0.5 % of the bounding-box diagonal (the reference's pymeshlab arguments), iterations to 3 (pymeshlab's default).  Returns
    (V float32, F int32) -- numpy arrays for numpy input, device tensors otherwise -- compacted (every vertex referenced), with the
    input's orientation.  stats: a dict that receives target_len, max_surf_dist and per iteration the split edges and the collapse
    and flip rounds used.  Two calls give the same bits."""
    from .lbvh import LBVH
    from .mesh import _as_device_mesh
    host = not torch.is_tensor(V)
    dev = V.device if torch.is_tensor(V) and V.is_cuda else torch.device('cuda', torch.cuda.current_device())
    V0, F0 = _as_device_mesh(V, F, dev)
    _validate(V0, F0)
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError("remesh_isotropic: iterations must be >= 0")
    with torch.cuda.device(dev):
        diag = float(torch.linalg.norm((V0.max(0).values - V0.min(0).values).double()))
        tl = DEFAULT_PCT / 100.0 * diag if target_len is None else float(target_len)
        msd = DEFAULT_PCT / 100.0 * diag if max_surf_dist is None else float(max_surf_dist)
        if not (tl > 0 and msd >= 0 and math.isfinite(tl) and math.isfinite(msd)):
            raise ValueError(f"remesh_isotropic: need target_len > 0 and max_surf_dist >= 0, got {tl} and {msd}")
        max_len2, min_len2, max_d2, cos2 = thresholds(tl, msd)
        bvh = LBVH(V0, F0)                                     # the input's tree, built once
        Vc, Fc = compact(V0, F0)
        log = dict(target_len=tl, max_surf_dist=msd, splits=[], collapse_rounds=[], flip_rounds=[])
        for _ in range(iterations):
            Vc, Fc, ns = split(Vc, Fc, max_len2)
            Vc, Fc, rc = collapse(Vc, Fc, min_len2, max_len2, bvh, max_d2)
            Vc, Fc, rf = flip(Vc, Fc, cos2, bvh, max_d2)
            T = Tables(Vc, Fc)
            Vc = project(relax(Vc, Fc, T), Fc, bvh, T)
            log['splits'].append(ns)
            log['collapse_rounds'].append(rc)
            log['flip_rounds'].append(rf)
    if stats is not None:
        stats.update(log)
    if host:
        return Vc.cpu().numpy(), Fc.cpu().numpy()
    return Vc, Fc


def simplified_path(path):
    """IN.ply -> IN_simplified.ply (the name extract_mesh_stage1.py gives the remeshed file)."""
    return os.path.splitext(path)[0] + "_simplified.ply"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.remesh", description="isotropic remeshing of a triangle mesh (PLY) on the GPU")
    ap.add_argument('input', type=str, help="input mesh (PLY)")
    ap.add_argument('--out', type=str, default=None, help="output PLY (default IN_simplified.ply next to the input)")
    ap.add_argument('--target-len-pct', type=float, default=DEFAULT_PCT, help="target edge length, %% of the bounding-box diagonal")
    ap.add_argument('--max-surf-dist-pct', type=float, default=DEFAULT_PCT,
                    help="largest distance from the input surface, %% of the bounding-box diagonal")
    ap.add_argument('--iterations', type=int, default=3, help="remeshing iterations (default 3)")
    return ap.parse_args(argv)


def remesh_file(src, out=None, target_len_pct=DEFAULT_PCT, max_surf_dist_pct=DEFAULT_PCT, iterations=3):
    """Read a PLY, remesh it (lengths in % of its bounding-box diagonal), write the result; -> (output path, V, F)."""
    from .mesh import read_ply, write_ply
    V, F = read_ply(src)
    diag = float(np.linalg.norm(V.max(0).astype(np.float64) - V.min(0).astype(np.float64))) if len(V) else 0.0
    Vr, Fr = remesh_isotropic(V, F, target_len=target_len_pct / 100.0 * diag, max_surf_dist=max_surf_dist_pct / 100.0 * diag,
                              iterations=iterations)
    out = out or simplified_path(src)
    write_ply(out, Vr, Fr)
    return out, Vr, Fr


def main(argv=None):
    a = parse_args(argv)
    out, V, F = remesh_file(a.input, a.out, a.target_len_pct, a.max_surf_dist_pct, a.iterations)
    print(f"wrote {out}: {len(V)} vertices, {len(F)} triangles")
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
