"""Quadric-error mesh decimation to a face budget on the GPU (Garland & Heckbert 1997; memoryless quadrics, Lindstrom & Turk 1998):
the step between a dense marching-cubes mesh and the texture atlas / the exporters, which want few faces with the detail in the
texture.  remesh_isotropic is uniform and has no budget; this is adaptive (flat regions lose their faces first) and stops at N.

python -m nu_nerf_amd.decimate IN.ply --faces N [--max-surf-dist-pct P] [--out OUT]
writes IN_decimated.ply next to the input unless --out is given, and prints one JSON line of statistics.

One round on a compacted mesh (kernels: csrc/decimate.hip):
  tables    remesh.Tables: the edge table and the vertex -> corner CSR.  Boundary and non-manifold edges are locked with their vertices:
            a locked vertex never moves, an edge between two of them is never collapsed, one with one locked end collapses onto it
  quadrics  per vertex, from its current faces (nothing is carried from round to round)
  eval      per edge: placement, cost, topological and geometric rejections -> cost, position, query-point count
  bound     (max_surf_dist only) the rewritten faces' vertices, centroids and edge midpoints against the input's LBVH, each allowed
            max_surf_dist minus the face's longest edge / sqrt(12): that certifies every point of the face within max_surf_dist, and
            rejects faces longer than sqrt(12) max_surf_dist
  keys      (quantised cost, hashed edge id); the k = min(candidates, (faces - target) // 2) smallest compete, the threshold stays
            on the device
  claim     keys written by 64-bit atomicMin over the ring of both ends; a winner holds both ends and both opposite vertices;
            winners apply in place; then compaction
Every step runs on the caller's current stream; the host reads counts only, once per round (once more with max_surf_dist, for the
size of the query); two calls give the same bits.
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from . import _lib as L
from .remesh import Tables, compact, _f32, _p

NO_KEY = 0x7fffffffffffffff       # csrc/decimate.hip's DM_NO_KEY
MIN_TARGET_FACES = 4              # a tetrahedron


def _lib():
    return L.load()


def cost_floor(lo, hi):
    """1e-12 diag^4 of the bounding box [lo, hi] (sequences of three floats), in float64 without a square root: the cost below
    which candidates are ordered by the hash alone."""
    d = [float(hi[k]) - float(lo[k]) for k in range(3)]
    d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    return 1e-12 * (d2 * d2)


class Round:
    """One round's candidates on the compacted mesh (V, F): tables, quadrics Q [nv,10], cost [nh], pos [nh,3], npts [nh]."""

    def __init__(self, V, F, min_quality2, mark=lambda name: None):
        self.lib, self.S = _lib(), L.stream(V.device.index)
        self.T = T = Tables(V, F)
        mark('tables')
        nh, dev = 3 * T.nf, V.device
        self.Q = torch.empty(T.nv, 10, dtype=torch.float64, device=dev)
        self.lib.nu_dm_quadrics(*T.args(), _p(self.Q), self.S)
        self.cost = torch.empty(nh, dtype=torch.float64, device=dev)
        self.pos = torch.empty(nh, 3, dtype=torch.float32, device=dev)
        self.npts = torch.empty(nh, dtype=torch.int32, device=dev)
        self.lib.nu_dm_eval(*T.args(), _p(self.Q), float(min_quality2), _p(self.cost), _p(self.pos), _p(self.npts), self.S)
        self.ncand = (self.npts > 0).sum()
        mark('eval')

    def keys(self, floor, bvh=None, max_dist=None):
        """ckey [nh] int64; with a tree, candidates with a query point farther from it than the point's allowance (nu_dm_points) get
        NO_KEY (one host read: the number of query points)."""
        T, dev = self.T, self.T.V.device
        nh = 3 * T.nf
        poff = d2 = lim = None
        if bvh is not None:
            inc = torch.cumsum(self.npts, 0)
            total = int(inc[-1])
            poff = inc - self.npts
            if total >= 2 ** 31:
                raise ValueError(f"decimate: {total} surface-distance query points in one round exceed the int32 range of the "
                                 "closest-point query; decimate without max_surf_dist first")
            pts = torch.empty(max(total, 1), 3, dtype=torch.float32, device=dev)
            d2 = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
            lim = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
            if total > 0:
                idx = torch.empty(total, dtype=torch.int32, device=dev)
                self.lib.nu_dm_points(*T.args(), _p(self.pos), _p(self.npts), _p(poff), max_dist, _p(pts), _p(lim), self.S)
                self.lib.nu_lbvh_closest(_p(bvh.buf), bvh.n_faces, _p(pts), total, _f32(max_dist * max_dist), _p(d2), _p(idx), None,
                                         self.S)
        self.ckey = torch.empty(nh, dtype=torch.int64, device=dev)
        self.lib.nu_dm_keys(_p(self.cost), _p(self.npts), None if poff is None else _p(poff), None if d2 is None else _p(d2),
                            None if lim is None else _p(lim), nh, float(floor), _p(self.ckey), self.S)
        return self.ckey

    def threshold(self, need):
        """[1] int64 on the device: the k-th smallest key, k = min(candidates, need) (at least 1; NO_KEY never competes)."""
        skeys = torch.sort(self.ckey).values
        k = torch.clamp(torch.clamp(self.ncand, max=int(need)), min=1)
        self.thr = skeys.gather(0, (k - 1).reshape(1))              # a device index: no host read
        return self.thr

    def winners(self):
        T = self.T
        claim = torch.empty(T.nv, dtype=torch.int64, device=T.V.device)
        self.win = torch.empty(3 * T.nf, dtype=torch.int32, device=T.V.device)
        self.lib.nu_dm_claim(*T.args(), _p(self.ckey), _p(self.thr), _p(claim), _p(self.win), self.S)
        return self.win

    def apply(self):
        T = self.T
        self.lib.nu_dm_apply(*T.args(), _p(self.win), _p(self.pos), _p(T.V), _p(T.F), self.S)


def _compact_counted(V, F, rnd):
    """(V', F', winners, candidates, largest accepted cost) after a round's apply: dead faces and unreferenced vertices dropped, both
    kept in order.  The round's one host read: the sizes and the counts together."""
    nv, nf, dev = V.shape[0], F.shape[0], V.device
    live = F[:, 0] >= 0
    used = torch.zeros(nv + 1, dtype=torch.bool, device=dev)
    used[torch.where(F >= 0, F, nv).reshape(-1).long()] = True
    used = used[:nv]
    won = rnd.win > 0
    top = torch.where(won, rnd.cost, torch.zeros_like(rnd.cost)).max()
    nfo, nvo, nwin, ncand, top = torch.stack([live.sum().double(), used.sum().double(), won.sum().double(), rnd.ncand.double(),
                                              top]).cpu().tolist()
    nfo, nvo = int(nfo), int(nvo)
    remap = torch.cumsum(used, 0, dtype=torch.int32) - 1
    fdst = torch.where(live, torch.cumsum(live, 0) - 1, nfo)            # dead rows land in a spare last row
    vdst = torch.where(used, remap.long(), nvo)
    Fo = torch.empty(nfo + 1, 3, dtype=torch.int32, device=dev).index_copy_(0, fdst, remap[F.clamp(min=0).long()])[:nfo]
    Vo = torch.empty(nvo + 1, 3, dtype=torch.float32, device=dev).index_copy_(0, vdst, V)[:nvo]
    return Vo.contiguous(), Fo.contiguous(), int(nwin), int(ncand), top


def _validate(V, F, target_faces):
    from .remesh import _validate as _mesh_ok
    _mesh_ok(V, F, "decimate")
    if int(target_faces) != target_faces or int(target_faces) < MIN_TARGET_FACES:
        raise ValueError(f"decimate: target_faces must be an integer >= {MIN_TARGET_FACES}, got {target_faces}")


def decimate(V, F, target_faces, max_surf_dist=None, min_quality=0.1, max_rounds=256, tolerance=0.02, stats=None):
    """Decimate the triangle mesh (V [Nv,3], F [Nf,3]) to about target_faces faces by quadric-error edge collapses on the GPU.
    The result has between target_faces and target_faces (1 + tolerance) faces when the run converges, and never fewer than
    target_faces.  max_surf_dist: when set, every point of every face of the result lies within this distance of the input.  A
    rewritten face's vertices, centroid and edge midpoints are queried against the input's LBVH and must stay within max_surf_dist
    minus the face's longest edge / sqrt(12), which bounds the rest of the face; a face longer than sqrt(12) max_surf_dist cannot be
    certified, so the bound also caps the edge length and a run under it may stop above its budget.  min_quality: a collapse may not leave a face whose shape quality (1: equilateral) is both
    below this and below what the face had.  Returns (V float32, F int32) -- numpy arrays for numpy input, device tensors otherwise
    -- compacted, with the input's orientation; a target at or above the input's face count returns the compacted input.  stats: a
    dict that receives rounds, faces_in, faces_out, converged, per_round [(faces, candidates, winners)], max_cost and cost_floor.
    Two calls give the same bits."""
    return _decimate(V, F, target_faces, max_surf_dist, min_quality, max_rounds, tolerance, stats)


@torch.no_grad()
def _decimate(V, F, target_faces, max_surf_dist, min_quality, max_rounds, tolerance, stats, mark=lambda name: None):
    """decimate(); mark(name) is called on the current stream after each phase of a round (scripts/bench_decimate.py times them)."""
    from .mesh import _as_device_mesh
    host = not torch.is_tensor(V)
    dev = V.device if torch.is_tensor(V) and V.is_cuda else torch.device('cuda', torch.cuda.current_device())
    V0, F0 = _as_device_mesh(V, F, dev)
    _validate(V0, F0, target_faces)
    target, max_rounds = int(target_faces), int(max_rounds)
    mq, tol = float(min_quality), float(tolerance)
    if not (0.0 <= mq <= 1.0 and tol >= 0.0 and max_rounds >= 0):
        raise ValueError(f"decimate: need 0 <= min_quality <= 1, tolerance >= 0 and max_rounds >= 0, got {mq}, {tol}, {max_rounds}")
    bvh = msd = None
    if max_surf_dist is not None:
        msd = _f32(max_surf_dist)
        if not (msd >= 0 and math.isfinite(msd)):
            raise ValueError(f"decimate: need max_surf_dist >= 0, got {msd}")
    with torch.cuda.device(dev):
        Vc, Fc = compact(V0, F0)
        nf = faces_in = int(Fc.shape[0])
        log = dict(rounds=0, faces_in=faces_in, faces_out=faces_in, converged=False, per_round=[], max_cost=0.0, cost_floor=0.0)
        if target < nf:
            box = torch.stack([V0.min(0).values, V0.max(0).values]).cpu().tolist()
            floor = log['cost_floor'] = cost_floor(*box)
            if msd is not None:
                from .lbvh import LBVH
                bvh = LBVH(V0, F0)                                 # the input's tree, built once
            while True:                                            # (Vc, Fc) are copies: compact() never returns its input
                if nf <= target * (1.0 + tol) or nf - target < 2:
                    log['converged'] = True
                    break
                if log['rounds'] >= max_rounds:
                    break
                rnd = Round(Vc, Fc, mq * mq, mark)
                rnd.keys(floor, bvh, msd)
                mark('bound' if bvh is not None else 'sort')
                rnd.threshold((nf - target) // 2)
                mark('sort')
                rnd.winners()
                rnd.apply()
                mark('claim')
                Vc, Fc, nwin, ncand, top = _compact_counted(Vc, Fc, rnd)
                mark('compact')
                log['per_round'].append((nf, ncand, nwin))
                if nwin == 0:
                    break
                nf = int(Fc.shape[0])
                log['rounds'] += 1
                log['max_cost'] = max(log['max_cost'], top)
        log['faces_out'] = int(Fc.shape[0])
    if stats is not None:
        stats.update(log)
    if host:
        return Vc.cpu().numpy(), Fc.cpu().numpy()
    return Vc, Fc


def decimated_path(path):
    """IN.ply -> IN_decimated.ply."""
    return os.path.splitext(path)[0] + "_decimated.ply"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m nu_nerf_amd.decimate",
                                 description="quadric-error decimation of a triangle mesh (PLY) to a face budget on the GPU")
    ap.add_argument('input', type=str, help="input mesh (PLY)")
    ap.add_argument('--faces', type=int, required=True, help="face budget")
    ap.add_argument('--max-surf-dist-pct', type=float, default=None,
                    help="largest distance from the input surface, %% of the bounding-box diagonal (default: no bound)")
    ap.add_argument('--out', type=str, default=None, help="output PLY (default IN_decimated.ply next to the input)")
    return ap.parse_args(argv)


def decimate_file(src, faces, max_surf_dist_pct=None, out=None):
    """Read a PLY, decimate it, write the result; -> (output path, V, F, stats)."""
    from .mesh import read_ply, write_ply
    V, F = read_ply(src)
    msd = None
    if max_surf_dist_pct is not None:
        diag = float(np.linalg.norm(V.max(0).astype(np.float64) - V.min(0).astype(np.float64))) if len(V) else 0.0
        msd = max_surf_dist_pct / 100.0 * diag
    stats = {}
    Vd, Fd = decimate(V, F, faces, max_surf_dist=msd, stats=stats)
    out = out or decimated_path(src)
    write_ply(out, Vd, Fd)
    return out, Vd, Fd, stats


def main(argv=None):
    a = parse_args(argv)
    out, V, F, stats = decimate_file(a.input, a.faces, a.max_surf_dist_pct, a.out)
    print(json.dumps(dict(out=out, vertices=len(V), **stats)))
    return out


if __name__ == "__main__":
    main(sys.argv[1:])
