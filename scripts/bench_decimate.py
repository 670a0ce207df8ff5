"""Report aid: decimate.decimate (csrc/decimate.hip) on marching-cubes meshes of the analytic r = 0.5 sphere at 256^3, 512^3 and
1024^3, brought down to --faces (default 100 000): ms per call ([median, min, max] of `--reps` calls after `--warmup`), rounds,
winners per candidate, the device time by phase (tables, eval, bound, sort, claim, compact), optionally under --max-surf-dist-pct, the Hausdorff and mean distance to the input
(mesh.mesh_distance) and the volume change.  Beside it, timed in the same process: remesh_isotropic with its defaults on the same
mesh, and -- with --chain -- "decimate to 4 x the remesh's face count, then remesh" against the remesh alone.  One JSON line per
resolution on stderr, all of them on stdout at the end."""
import argparse
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from bench_remesh import sphere_mesh
from nu_nerf_amd.decimate import _decimate
from nu_nerf_amd.mesh import decimate, mesh_distance, remesh_isotropic


class Phases:
    """Device time per phase of the rounds: an event on the current stream at every mark, read once at the end."""

    def __init__(self):
        self.spans, self.last = [], self._event()

    @staticmethod
    def _event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def __call__(self, name):
        e = self._event()
        self.spans.append((name, self.last, e))
        self.last = e

    def totals(self):
        torch.cuda.synchronize()
        out = {}
        for name, a, b in self.spans:
            out[name] = out.get(name, 0.0) + a.elapsed_time(b)
        return {k: round(v, 3) for k, v in out.items()}


def volume(V, F):
    W = V.double()
    a, b, c = W[F[:, 0].long()], W[F[:, 1].long()], W[F[:, 2].long()]
    return float((a * torch.linalg.cross(b, c)).sum() / 6.0)


def timed(fn, warmup, reps):
    """(last result, [median, min, max] ms of `reps` calls, each between its own pair of device events)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return out, [round(ms[len(ms) // 2], 2), round(ms[0], 2), round(ms[-1], 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--res', type=int, nargs='+', default=[256, 512, 1024])
    ap.add_argument('--faces', type=int, default=100_000)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--max-surf-dist-pct', type=float, default=None, help="surface bound, %% of the bounding-box diagonal (default: none)")
    ap.add_argument('--no-remesh', action='store_true', help="skip the remesh_isotropic comparison")
    ap.add_argument('--chain', action='store_true', help="also time decimate (4 x the remesh's faces) + remesh")
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    rows = []
    for res in args.res:
        V, F = sphere_mesh(res, dev)
        msd = None
        if args.max_surf_dist_pct is not None:
            msd = args.max_surf_dist_pct / 100.0 * float(torch.linalg.norm((V.max(0).values - V.min(0).values).double()))
        (Vd, Fd), ms = timed(lambda: decimate(V, F, args.faces, max_surf_dist=msd), args.warmup, args.reps)
        stats, phases = {}, Phases()
        _decimate(V, F, args.faces, msd, 0.1, 256, 0.02, stats, mark=phases)
        d = mesh_distance((Vd, Fd), (V, F), n_samples=1_000_000)
        v0, v1 = volume(V, F), volume(Vd, Fd)
        per = stats['per_round']
        row = {'res': res, 'faces_in': int(len(F)), 'faces_out': int(len(Fd)), 'ms': ms, 'rounds': stats['rounds'],
               'converged': stats['converged'], 'winners_per_candidate': round(sum(r[2] for r in per) / max(sum(r[1] for r in per), 1), 4),
               'phase_ms': phases.totals(), 'max_surf_dist': msd, 'a_to_b_max': d['a_to_b_max'], 'max_cost': stats['max_cost'], 'hausdorff': d['hausdorff'], 'chamfer': d['chamfer'],
               'volume_change': (v1 - v0) / v0}
        if not args.no_remesh:
            rs = {}
            (Vr, Fr), row['remesh_ms'] = timed(lambda: remesh_isotropic(V, F, stats=rs), args.warmup, args.reps)
            row['remesh_faces_out'], row['remesh_collapse_rounds'] = int(len(Fr)), rs['collapse_rounds']
            if args.chain:
                diag = float(torch.linalg.norm((V.max(0).values - V.min(0).values).double()))

                def chain():
                    Vm, Fm = decimate(V, F, 4 * len(Fr))
                    return remesh_isotropic(Vm, Fm, target_len=0.005 * diag, max_surf_dist=0.005 * diag)
                (Vc, Fc), row['chain_ms'] = timed(chain, args.warmup, args.reps)
                row['chain_faces_out'] = int(len(Fc))
                row['chain_hausdorff'] = mesh_distance((Vc, Fc), (V, F), n_samples=1_000_000)['hausdorff']
                row['remesh_hausdorff'] = mesh_distance((Vr, Fr), (V, F), n_samples=1_000_000)['hausdorff']
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
