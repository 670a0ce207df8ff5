"""Derives the bound of the white-furnace test of tests/test_relight_gpu.py on the CPU, from the float64 oracle alone.

Per material (metallic, roughness; albedo 0.8) of the test's grid:
  gap    max over N.V in [0.2, 1] of | oracle estimator at S = 65536 - (diffuse + F0 A + B from assets/bsdf_256_256.bin) |: what separates
         the shipped masking term from the table (the Monte-Carlo error at 32 768 Hammersley points per lobe is far below it);
  sigma  the largest standard deviation, over N.V, of the estimator at the test's S = 64 across 256 pixel shifts.
The test compares bin means over at least N_MIN pixels: bound = gap + 4 sigma / sqrt(N_MIN) + FACET (samples a facet's own horizon
clips on the 81 920-face sphere: at most the cosine-weighted mass within 1.1 degrees of the horizon, sin^2 < 4e-4, rounded up to 1e-3).
Also prints the same gap for the Schlick k = alpha / 2 masking the project did not ship.

    python scripts/relight_furnace_bound.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import relight_oracle as O   # noqa: E402
from nu_nerf_amd.params import load_fg_lut   # noqa: E402

ALBEDO, S_TEST, N_MIN, FACET = 0.8, 64, 300, 1e-3
GRID = [(m, r) for m in (0.0, 1.0) for r in (0.3, 0.6, 0.9)]


def expected(lut, nov, metallic, roughness):
    ab = O.fg_lookup(lut, np.asarray(nov), np.asarray(roughness))
    f0 = 0.04 + (ALBEDO - 0.04) * metallic
    return (1.0 - metallic) * ALBEDO + f0 * ab[..., 0] + ab[..., 1]


def main():
    lut = load_fg_lut()[0].astype(np.float64)
    novs = np.linspace(0.2, 1.0, 41)
    for metallic, roughness in GRID:
        gaps = {}
        for name, g1 in (('smith', O.g1_smith), ('schlick', O.g1_schlick)):
            est = np.array([O.furnace_estimate(n, ALBEDO, metallic, roughness, 65536, [0], g1=g1)[0, 0] for n in novs])
            gaps[name] = np.abs(est - expected(lut, novs, metallic, roughness)).max()
        sig = max(O.furnace_estimate(n, ALBEDO, metallic, roughness, S_TEST, range(256))[:, 0].std() for n in novs[::5])
        bound = gaps['smith'] + 4.0 * sig / np.sqrt(N_MIN) + FACET
        print(f"metallic {metallic:.1f} roughness {roughness:.1f}: gap smith {gaps['smith']:.5f} (schlick {gaps['schlick']:.5f})  "
              f"sigma(S={S_TEST}) {sig:.5f}  bound {bound:.5f}", flush=True)


if __name__ == '__main__':
    main()
