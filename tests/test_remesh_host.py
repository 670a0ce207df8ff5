"""Isotropic remeshing, host side (no GPU): the numpy ports of tests/remesh_oracle.py on their own (split, one collapse round,
one flip round, relaxation keep a closed mesh closed and oriented), the C ABI surface, the thresholds and the CLI arguments."""
import os
import re

import numpy as np

import remesh_oracle as O
from test_mesh_host import directed_edge_defects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def perturbed_icosphere(subdiv=2, amp=0.15, seed=0):
    from nu_nerf_amd.lbvh import icosphere
    V, F = icosphere(subdiv, 0.5)
    rng = np.random.default_rng(seed)
    edge = np.linalg.norm(V[F[0, 0]] - V[F[0, 1]])
    return (V + rng.uniform(-amp, amp, V.shape) * edge).astype(np.float32), F


def euler(V, F):
    return len(np.unique(F)) - 3 * len(F) // 2 + len(F)


def test_header_declares_the_remesh_entries():
    text = open(os.path.join(ROOT, "include", "nu_nerf.h")).read()
    for name in ("nu_rm_edge_keys", "nu_rm_edges", "nu_rm_split_count", "nu_rm_split_write", "nu_rm_collapse_count",
                 "nu_rm_collapse_points", "nu_rm_collapse_claim", "nu_rm_collapse_apply", "nu_rm_flip_count", "nu_rm_flip_points",
                 "nu_rm_flip_claim", "nu_rm_flip_apply", "nu_rm_relax", "nu_rm_project"):
        assert re.search(r"\b%s\s*\(" % name, text), name


def test_oracle_tables_lock_boundary_edges():
    V, F = perturbed_icosphere()
    T = O.Tables(V, F)
    assert not T.vlock.any() and not T.vbound.any()
    assert int((T.E[:, 2] == 2).sum()) == 3 * len(F) // 2
    Fo = F[3:]                                      # open: three faces removed
    T = O.Tables(V, Fo)
    border = np.unique(F[:3])
    assert set(np.nonzero(T.vlock)[0]) == set(border.tolist()) and set(np.nonzero(T.vbound)[0]) == set(border.tolist())


def test_oracle_split_is_closed_and_exact():
    V, F = perturbed_icosphere()
    lens = np.linalg.norm(V[F] - V[np.roll(F, -1, 1)], axis=2)
    max_len2 = np.float32(np.median(lens) ** 2)
    V2, F2 = O.split(V, F, max_len2)
    n_split = len(V2) - len(V)
    assert 0 < n_split < 3 * len(F) // 2
    assert len(F2) == len(F) + 2 * n_split          # every split edge adds a face on each side
    assert directed_edge_defects(F2) == 0 and euler(V2, F2) == 2
    assert V2[:len(V)].tobytes() == V.tobytes()


def test_oracle_rounds_keep_the_mesh_closed():
    V, F = perturbed_icosphere()
    lens = np.linalg.norm(V[F] - V[np.roll(F, -1, 1)], axis=2)
    L = float(np.median(lens)) / 0.8 * 1.05
    params = ((0.8 * L) ** 2, (4 / 3 * L) ** 2)
    T, win = O.round_winners('collapse', V, F, V, F, params, np.inf)
    assert win
    rings = [set(int(u) for v in T.quad(e)[:2] for g in T.faces_of(v) for u in T.F[g]) for e in win]
    for i in range(len(rings)):                     # an independent set
        for j in range(i):
            assert not rings[i] & rings[j]
    V2, F2 = O.collapse_apply(T, win)
    F2 = F2[F2[:, 0] >= 0]
    assert len(F2) == len(F) - 2 * len(win)
    assert directed_edge_defects(F2) == 0 and euler(V2, F2) == 2
    T, fw = O.round_winners('flip', V2, F2, V, F, (np.cos(np.radians(30.0)) ** 2,), np.inf)
    F3 = O.flip_apply(T, fw)
    assert directed_edge_defects(F3) == 0
    V4 = O.relax(V2, F3)
    assert np.isfinite(V4).all() and not np.array_equal(V4[np.unique(F3)], V2[np.unique(F3)])


def test_thresholds_and_cli_arguments():
    from nu_nerf_amd import remesh as R
    max_len2, min_len2, max_d2, cos2 = R.thresholds(0.03, 0.01)
    assert max_len2 == float(np.float32((4 / 3 * 0.03) ** 2)) and min_len2 == float(np.float32((0.8 * 0.03) ** 2))
    assert max_d2 == float(np.float32(1e-4)) and abs(cos2 - 0.75) < 1e-6
    a = R.parse_args(["m.ply"])
    assert a.out is None and a.target_len_pct == 0.5 and a.max_surf_dist_pct == 0.5 and a.iterations == 3
    assert R.simplified_path(os.path.join("d", "golden-1234.ply")) == os.path.join("d", "golden-1234_simplified.ply")
    from nu_nerf_amd.extract_mesh import parse_args
    assert parse_args(["--cfg", "x.yaml", "--remesh"]).remesh and not parse_args(["--cfg", "x.yaml"]).remesh
