"""Writes tests/golden/environment_stage1.npz: the learned-illumination query as the REFERENCE's own modules compute it on the CPU
(network/field.py:447-464, :594-604, :636-667).

Run once on a machine with the reference checkout, from its directory (the import shims are those of oracle/gen_golden.py):

    cd <reference> && python <repo>/scripts/gen_environment_golden.py

The test suite needs neither this script nor the reference, only the .npz file.  Parameters and rows are seed-generated
(randomize_for_parity(init_stage1_params(6033, sphere_direction=...), seed=1) plus environment_oracle.head_gain_overrides;
environment_oracle.rows(512, ROW_SEED)), so the fixture holds expected arrays, the overrides and measured deviations only.

Per `sphere_direction` setting (keys sd0__* / sd1__*), on the same 512 rows -- the poles, the axes, rho cycling through 0, 0.03, 0.5, 1,
points inside the unit ball of which the last 16 lie beyond radius 0.999 (offset_points_to_sphere's branch):
  direct                     exp head of outer_light on sph_enc(d, rho) (| sph_enc of the sphere point, through offset_points_to_sphere and
                             get_sphere_intersection) -- the reference's modules, called as predict_specular_lights calls them
  light, indirect, occ_raw   what predict_specular_lights ITSELF returns for reflective = d (human_light off): the blend, the indirect
                             light times the clamped occlusion, the occlusion before the clamp
  dev_*                      the largest deviation of these fp32 results from the float64 oracle (tests/environment_oracle.py): relative for
                             the radiances (|a - b| / |b|), absolute for the occlusion
  valid                      rows on which the reference's result exists: its IDE is NaN on the poles +-z ((0 + 0i)^m as a complex power), so
                             the two pole rows are left out of every comparison with the fixture (the occlusion, which has no IDE, exists)
  override__*                the head gains
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from gen_golden import install_shims, to_t   # noqa: E402
import environment_oracle as EO              # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden')
ROW_SEED = 2025
N_ROWS = 512
EXP_MAX = 3.0


def gen(rfield, sd, res):
    from nu_nerf_amd.params import init_stage1_params, randomize_for_parity
    p = randomize_for_parity(init_stage1_params(6033, sphere_direction=sd), seed=1)
    over = EO.head_gain_overrides(p)
    p.update(over)
    col = rfield.AppShadingNetwork({'sphere_direction': sd, 'light_exp_max': EXP_MAX})
    col.load_state_dict(to_t({k[len('color_network.'):]: v for k, v in p.items() if k.startswith('color_network.')}), strict=True)
    assert col.cfg['light_pos_freq'] == 6 and not col.cfg['human_light']
    d, rho, x = EO.rows(N_ROWS, ROW_SEED)
    assert int((np.linalg.norm(x.astype(np.float64), axis=1) > 0.999).sum()) >= 16
    dt, rt, xt = torch.from_numpy(d), torch.from_numpy(rho).reshape(-1, 1), torch.from_numpy(x)
    with torch.no_grad():
        enc = col.sph_enc(dt, rt)
        if sd:
            sp = rfield.offset_points_to_sphere(xt)
            sp = F.normalize(sp + dt * rfield.get_sphere_intersection(sp, dt), dim=-1)
            enc = torch.cat([enc, col.sph_enc(sp, rt)], -1)
        direct = col.outer_light(enc)
        light, _, occ_raw, indirect, human = col.predict_specular_lights(xt, None, dt, rt, None, 0)
        # the blend written out from the modules: what predict_specular_lights must have returned
        pts = col.pos_enc(xt)
        ind = col.inner_light(torch.cat([pts, col.sph_enc(dt, rt)], -1))
        occ = torch.clamp(col.inner_weight(torch.cat([pts, col.dir_enc(dt)], -1)) * 0.5 + 0.5, min=0, max=1)
        # the reference evaluates (x + i y)^m as a complex power with a real exponent, which is NaN at x = y = 0: its own result does
        # not exist on the poles +-z.  Those rows are recorded (`valid`) and left out of every comparison WITH THE FIXTURE; the
        # float64 oracle and the layered path cover them
        valid = torch.isfinite(light).all(1)
        assert torch.equal(valid, ~((dt[:, 0] == 0) & (dt[:, 1] == 0))) and int((~valid).sum()) == 2
        assert torch.allclose((ind * occ + direct * (1 - occ))[valid], light[valid], rtol=1e-6, atol=0)
        assert torch.allclose((ind * occ)[valid], indirect[valid], rtol=1e-6, atol=1e-7)
    assert human == 0
    o = EO.light64(p, d, rho, x, sphere=sd, exp_max=EXP_MAX, probe=True)
    v = valid.numpy()
    rel = lambda a, b: float((np.abs(a.numpy().astype(np.float64) - b) / np.abs(b))[v].max())      # noqa: E731
    pre = f'sd{int(sd)}__'
    res.update({pre + 'direct': direct.numpy(), pre + 'light': light.numpy(), pre + 'indirect': indirect.numpy(),
                pre + 'occ_raw': occ_raw.numpy().reshape(-1), pre + 'valid': v,
                pre + 'dev_direct': np.asarray(rel(direct, o['direct'])), pre + 'dev_light': np.asarray(rel(light, o['light'])),
                pre + 'dev_indirect': np.asarray(float(np.abs(indirect.numpy().astype(np.float64) - o['indirect'])[v].max())),
                pre + 'dev_occ': np.asarray(float(np.abs(occ_raw.numpy().reshape(-1).astype(np.float64) - o['occ_raw']).max()))})
    res.update({pre + 'override__' + k: v for k, v in over.items()})
    sh = EO.shares(o, EXP_MAX)
    assert sh[5] >= 0.1 and max(sh[4], sh[6]) >= 0.1, sh      # the occlusion's interior and one of its clamps are both in the fixture
    spread = float(o['light'].max() / o['light'].min())
    assert spread > 1.1, spread
    print(f'sphere_direction {sd}: light in [{o["light"].min():.3f}, {o["light"].max():.3f}], occ shares (0, interior, 1) {np.round(sh[4:], 3)}, '
          f'fp32 reference vs float64: direct {res[pre + "dev_direct"]:.2e} light {res[pre + "dev_light"]:.2e} (relative), '
          f'indirect {res[pre + "dev_indirect"]:.2e} occ {res[pre + "dev_occ"]:.2e} (absolute)')


def main():
    install_shims()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import network.field as rfield
    res = {'row_seed': np.asarray(ROW_SEED), 'n_rows': np.asarray(N_ROWS), 'exp_max': np.asarray(EXP_MAX, np.float32)}
    for sd in (False, True):
        gen(rfield, sd, res)
    np.savez_compressed(os.path.join(OUT, 'environment_stage1.npz'), **res)
    print('wrote', os.path.join(OUT, 'environment_stage1.npz'))


if __name__ == '__main__':
    main()
