"""Host-side checks of the learned-background feature (no GPU): the C entry's declaration, the float64 oracle against the reference's
recorded color_bkgr, the node restatement against the oracle's sampler, the AOV names and the command line."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import background_oracle as BO
from helpers import golden, oracle_cfg, parity_params
from oracle import stage1_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = ["step0_r48", "step20000_r48", "step500_r32_noperturb"]


def test_header_declares_and_source_defines_the_entry():
    from nu_nerf_amd import _lib as L
    sig = {name: args for name, _, args in L._signatures()}
    assert 'nu_background_fwd' in sig and len(sig['nu_background_fwd']) == 15
    with open(os.path.join(ROOT, 'include', 'nu_nerf.h')) as fh:
        text = fh.read()
    assert text.index('int nu_nerfpp_mlp_bwd(') < text.index('int nu_background_fwd(') < text.index('typedef struct NuShadeNet')
    with open(os.path.join(ROOT, 'nu_nerf_amd', 'csrc', 'background.hip')) as fh:
        src = fh.read()
    assert re.search(r'extern "C" int nu_background_fwd\(const NuNerfNet\* net,', src)
    assert '__global__' in src and '#include "fused_mlp.h"' in src


@pytest.fixture(scope="module")
def params():
    return parity_params()


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_reproduces_the_reference_color_bkgr(tag, params):
    """At the fixtures' own z_vals, t_stop = None: out_color_bkgr at the tolerance test_oracle_golden.py holds the oracle's render_core
    to for the same quantity; the fp32 geometry reproduces the recorded inner mask point for point."""
    g, c = golden(f"train_{tag}.npz"), golden(f"core_{tag}.npz")
    o = torch.from_numpy(g['rays_o'])
    dn = torch.nn.functional.normalize(torch.from_numpy(g['rays_d']), dim=-1)
    z = torch.from_numpy(c['z_vals'])
    _, _, _, inner, live = BO.sample_geometry(o, dn, z)
    assert np.array_equal(inner.numpy(), c['inner_mask'])
    n_out = live.sum(1)
    assert int(n_out.min()) >= 30 and int(n_out.max()) <= z.shape[1]              # every ray has outer samples: not vacuous
    col, trans = BO.background(params, o, dn, z)
    assert float(g['out_color_bkgr'].min()) > 0.5
    np.testing.assert_allclose(col.numpy(), g['out_color_bkgr'], rtol=1e-4, atol=1e-5)
    assert bool(((trans > 0) & (trans < 1.0 + 1e-5)).all())
    # a stop in front of everything leaves nothing; a stop behind everything changes nothing
    col0, tr0 = BO.background(params, o, dn, z, torch.zeros(o.shape[0]))
    assert bool((col0 == 0).all()) and np.allclose(tr0.numpy(), (1.0 + 1e-7) ** z.shape[1], rtol=1e-12)
    coli, tri = BO.background(params, o, dn, z, torch.full((o.shape[0],), float('inf')))
    assert torch.equal(coli, col) and torch.equal(tri, trans)


def test_node_restatement_equals_the_oracle_sampler(params):
    """sample_ray with n_importance = 0, perturb = 0.  The sampler's loop (renderer_zerothick.py:601-609) runs `up_sample_steps` rounds
    of n_importance // up_sample_steps nodes each and its inverse-CDF draw divides by that count, so "no importance pass" is
    spelled n_importance = 0 WITH up_sample_steps = 0: the coarse and the background nodes, nothing else."""
    g = golden("train_step500_r32_noperturb.npz")
    o = torch.from_numpy(g['rays_o'])
    dn = torch.nn.functional.normalize(torch.from_numpy(g['rays_d']), dim=-1)
    for near, far in (O.near_far_from_sphere(o, dn), (torch.full((o.shape[0], 1), 0.8), torch.full((o.shape[0], 1), 4.5))):
        for nc, nbg in ((32, 16), (64, 32), (5, 3)):
            cfg = oracle_cfg(n_samples=nc, n_bg_samples=nbg, n_importance=0, up_sample_steps=0)
            with torch.no_grad():
                ref = O.sample_ray(params, cfg, o, dn, near, far, 0)
            z = BO.default_nodes(o, dn, near, far, nc, nbg)
            assert z.shape == ref.shape == (o.shape[0], nc + nbg)
            assert torch.equal(z, ref)
            assert bool((z[:, 1:] >= z[:, :-1]).all())


def test_aov_names():
    from nu_nerf_amd import sdf_trace as T
    assert T.BACKGROUND_AOVS == ('background', 'transmittance', 'frame')
    assert not set(T.BACKGROUND_AOVS) & set(T.ALL_AOVS)
    assert T._check_aovs(T.ALL_AOVS + T.BACKGROUND_AOVS) == T.ALL_AOVS + T.BACKGROUND_AOVS
    assert T._check_aovs('frame') == ('frame',)
    for bad in ('color', 'rgba', ('frame', 'color')):
        with pytest.raises(ValueError):
            T._check_aovs(bad)


def test_command_line():
    from nu_nerf_amd import render_surface as R
    f = R.parse_args(['--cfg', 'c.yaml', '--aovs', 'frame', 'background'])
    assert f.aovs == ('frame', 'background') and f.white_background is None
    assert R.parse_args(['--cfg', 'c.yaml', '--aovs', 'frame', '--white-background']).white_background is True
    assert R.parse_args(['--cfg', 'c.yaml', '--aovs', 'transmittance', '--no-white-background']).white_background is False
    assert R.parse_args(['--cfg', 'c.yaml']).aovs == R.DEFAULT_AOVS
    with pytest.raises(SystemExit):
        R.parse_args(['--cfg', 'c.yaml', '--aovs', 'color'])


def test_frame_paths():
    from nu_nerf_amd import render_surface as R
    p = R.frame_paths('out', 3, ('frame',))
    assert p == {'frame': os.path.join('out', '3_frame.png'), 'background': os.path.join('out', '3_background.png')}
    p = R.frame_paths('out', 0, ('background', 'transmittance', 'depth'))
    assert set(p) == {'background', 'transmittance', 'depth', 'depth.npy'} and p['transmittance'].endswith('0_transmittance.png')
    assert R.frame_paths('out', 1, ('rgb',)) == {'rgb': os.path.join('out', '1_rgb.png')}


def test_argument_errors_are_library_errors():
    from nu_nerf_amd._lib import NuNerfLibraryError
    from nu_nerf_amd.background import _per_ray, _count
    from nu_nerf_amd.sdf_trace import _check_rays
    with pytest.raises(NuNerfLibraryError):
        _check_rays(torch.zeros(4, 2), 'rays_o')
    with pytest.raises(NuNerfLibraryError):
        _per_ray(torch.zeros(3), 4, torch.device('cpu'), 't_stop')
    with pytest.raises(NuNerfLibraryError):
        _count(0, 'n_samples', 1)


def test_compile_record():
    """The compile record (read like tests/test_abi.py reads the siblings': scripts/kernel_regs.py on the built object).  No VGPR spill, no scratch, and the LDS figure the file's header states: one workgroup per CU."""
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        from kernel_regs import kernel_table
    finally:
        sys.path.pop(0)
    from nu_nerf_amd import build as B
    B.build(verbose=False)
    obj = os.path.join(ROOT, 'nu_nerf_amd', 'build', 'background.o')
    table = dict(kernel_table(obj))
    assert list(table) == ['background_fwd_kernel(BgNet)']
    r = table['background_fwd_kernel(BgNet)']
    print("background_fwd_kernel:", r)
    with open(os.path.join(ROOT, 'nu_nerf_amd', 'csrc', 'background.hip')) as fh:
        head = fh.read().split('#include')[0]
    stated = int(head.split('(weight stages) =')[1].split('B of the CU')[0].replace(' ', ''))
    assert r['vgpr_spill'] == 0 and r['scratch'] == 0
    assert r['lds'] == stated == 120464 and r['lds'] <= 163840 and 2 * r['lds'] > 163840
