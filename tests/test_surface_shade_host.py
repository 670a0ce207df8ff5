"""Surface shading, the parts that need no GPU: the float64 wrapper (tests/surface_shade_oracle.py) against the reference's recorded
shading rows, the AOV names of render_surface, the command's parser and the C header."""
import os

import numpy as np
import pytest

import surface_shade_oracle as SO
from helpers import golden, oracle_cfg, parity_params


@pytest.fixture(scope="module")
def ops():
    return golden("ops.npz")


@pytest.fixture(scope="module")
def fixture_terms(ops):
    return SO.shade64(parity_params(), oracle_cfg(), ops['shade_pts'], ops['shade_view'], normals=ops['shade_nrm'], feats=ops['shade_feats'])


def test_wrapper_reproduces_the_reference_shading_rows(ops, fixture_terms):
    """The tolerance of test_oracle_golden.test_shading (the fixture is the reference's own fp32 result)."""
    o = fixture_terms
    np.testing.assert_allclose(o['rgb'], ops['shade_color'], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(o['reflective'], ops['shade_reflective'], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(o['occ_prob'][:, None], ops['shade_occ_prob'].reshape(-1, 1), rtol=2e-5, atol=2e-6)


def test_restated_terms_agree_with_the_oracle_colour(fixture_terms):
    """The terms are restated from the formulas shading_forward evaluates: in float64 the two colours agree to rounding, and the terms
    recombine to the colour."""
    o = fixture_terms
    np.testing.assert_allclose(o['rgb_terms'], o['rgb'], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(o['occ_prob'], o['occ_prob_oracle'], rtol=1e-12, atol=1e-13)
    assert o['raw'].shape == (o['rgb'].shape[0], 20) and not o['raw'][:, 19].any()
    assert (o['reflection_weight'] >= 0.04 - 1e-12).all() and (o['reflection_weight'] <= 1.0).all()
    occ = np.clip(o['occ_prob'], 0.0, 1.0)[:, None]
    np.testing.assert_allclose(o['indirect_light'], np.exp(np.minimum(o['raw'][:, 9:12], 3.0)) * occ, rtol=1e-12)
    np.testing.assert_allclose(o['diffuse_light'], np.exp(np.minimum(o['raw'][:, 0:3], 3.0)), rtol=1e-12)


def test_refraction_cap_only_lowers_the_refraction_term(ops):
    p, cfg = parity_params(), oracle_cfg()
    a = SO.terms64(p, cfg, ops['shade_pts'], ops['shade_nrm'], ops['shade_view'], ops['shade_feats'])
    cap = float(np.median(a['raw'][:, 16:19]))            # (the seed-generated head sits near log 0.5, below SpecInner's -0.2)
    b = SO.terms64(p, cfg, ops['shade_pts'], ops['shade_nrm'], ops['shade_view'], ops['shade_feats'], refrac_exp_max=cap)
    assert np.array_equal(a['raw'], b['raw']) and np.array_equal(a['specular_color'], b['specular_color'])
    assert (b['refraction_light'] <= a['refraction_light']).all()
    assert (a['raw'][:, 16:19] > cap).any() and (a['raw'][:, 16:19] < cap).any() and not np.array_equal(a['rgb'], b['rgb'])


def test_shading_aov_names():
    from nu_nerf_amd import sdf_trace as S
    assert S.SHADING_AOVS == ('rgb', 'diffuse_color', 'specular_color', 'diffuse_light', 'specular_light', 'occ_prob', 'indirect_light',
                              'refraction_light', 'reflection_weight')
    assert S.ALL_AOVS == S.AOVS + S.SHADING_AOVS and len(set(S.ALL_AOVS)) == len(S.ALL_AOVS)
    assert len(S.AOVS) == 9 and not set(S.AOVS) & set(S.SHADING_AOVS)
    from nu_nerf_amd.surface_shade import TERMS
    assert set(TERMS) == set(S.SHADING_AOVS) - {'rgb'}
    assert {a for a in S.SHADING_AOVS if S._CHANNELS.get(a) == 3} == {'rgb'} | {k for k, c in TERMS.items() if c == 3}


def test_check_aovs_takes_the_new_names_and_refuses_unknown_ones():
    from nu_nerf_amd.sdf_trace import ALL_AOVS, _check_aovs
    assert _check_aovs('rgb') == ('rgb',)
    assert _check_aovs(('depth', 'rgb', 'occ_prob')) == ('depth', 'rgb', 'occ_prob')
    assert _check_aovs(ALL_AOVS) == ALL_AOVS
    for bad in ('color', 'rgba', 'human_light', ('rgb', 'specular'), ()):
        with pytest.raises(ValueError):
            _check_aovs(bad)


def test_command_parses_shading_aovs():
    from nu_nerf_amd import render_surface as R
    flags = R.parse_args(['--cfg', 'x.yaml', '--aovs', 'rgb'])
    assert flags.aovs == ('rgb',)
    flags = R.parse_args(['--cfg', 'x.yaml', '--aovs', 'rgb', 'depth', 'specular_light', 'rgb'])
    assert flags.aovs == ('rgb', 'depth', 'specular_light')
    assert R.frame_paths('out', 3, flags.aovs)['rgb'] == os.path.join('out', '3_rgb.png')
    with pytest.raises(SystemExit):
        R.parse_args(['--cfg', 'x.yaml', '--aovs', 'colour'])
    img = R.to_plain(np.asarray([[0.0, 0.5], [1.0, 7.0]], np.float32))
    assert img.dtype == np.uint8 and img.tolist() == [[0, 128], [255, 255]]


def test_header_declares_the_entry():
    from nu_nerf_amd import _lib as L
    sig = {name: args for name, _, args in L._signatures()}
    assert 'nu_surface_shade_fwd' in sig and len(sig['nu_surface_shade_fwd']) == 25
    assert L.NU_SHADE_LINEAR == 1
    with open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), 'csrc', 'surface_shade.hip')) as fh:
        assert 'extern "C" int nu_surface_shade_fwd(' in fh.read()
