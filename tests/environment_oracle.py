"""Float64 restatement of the learned-illumination query (TEST INFRASTRUCTURE -- not a test, not product code).

predict_specular_lights with reflective = d and no human light (network/field.py:636-667, :1399-1430), written from the formulas the
header of nu_nerf_amd/csrc/light_bake.hip cites; no code of the kernel or of nu_nerf_amd/environment.py is used.  The IDE, the
embedders and the sphere point are those of tests/encode_oracle.py (anchored on data recorded from the original project by
tests/test_encode_oracle_host.py); the predictors are written out here in numpy: four weight-normalised linear layers, ReLU x 3.
Everything takes and returns numpy arrays; the arithmetic is float64 throughout.

Also here, because the fixture generator (scripts/gen_environment_golden.py) and the tests must agree on them: the seed-generated rows
(`rows`), the directions every test includes (`special_dirs`) and the head overrides of the clamp test (`clamp_overrides`).
"""
import numpy as np
import torch

import encode_oracle as EO


def _t(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


def wn_weight64(params, name):
    """Legacy weight_norm (dim 0) of layer `name`: W = g v / |v|_row, in float64."""
    v = np.asarray(params[name + '.weight_v'], np.float64)
    g = np.asarray(params[name + '.weight_g'], np.float64).reshape(-1, 1)
    return v * (g / np.sqrt((v * v).sum(1, keepdims=True)))


def predictor64(params, prefix, x):
    """make_predictor (field.py:371-408) without its output activation: sequential indices 0, 2, 4, 6, ReLU after the first three."""
    h = np.asarray(x, np.float64)
    for j, idx in enumerate((0, 2, 4, 6)):
        h = h @ wn_weight64(params, f'{prefix}.{idx}').T + np.asarray(params[f'{prefix}.{idx}.bias'], np.float64)
        if j < 3:
            h = np.maximum(h, 0.0)
    return h


def encode64(dirs, rho, x, sphere, pos_freq=6):
    """The three input rows in float64: outer_light [N, 72 or 144], inner_light [N, pe + 72], inner_weight [N, pe + 39]."""
    d, k = _t(dirs), _t(rho).reshape(-1, 1)
    xs = _t(np.broadcast_to(np.zeros(3) if x is None else np.asarray(x, np.float64), d.shape))
    ide = EO.ide64(d, k)
    ol = torch.cat([ide, EO.ide64(EO.sphere_point64(xs, d), k)], -1) if sphere else ide
    pe = EO.embed64(xs, pos_freq)
    return ol.numpy(), torch.cat([pe, ide], -1).numpy(), torch.cat([pe, EO.embed64(d, 6)], -1).numpy()


def light64(params, dirs, rho, x=None, *, sphere=False, exp_max=3.0, pos_freq=6, probe=False, prefix='color_network'):
    """dict of float64 arrays: 'raw' [N,7] (direct 3, indirect 3, occlusion 1; the last four 0 without probe), 'direct', 'light' and,
    with probe, 'indirect' (times occ), 'occ' (clamped), 'occ_raw' (0.5 head + 0.5 before the clamp)."""
    dirs = np.asarray(dirs, np.float64)
    rho = np.broadcast_to(np.asarray(rho, np.float64), dirs.shape[:1])
    ol, il, iw = encode64(dirs, rho, x, sphere, pos_freq)
    raw = np.zeros((dirs.shape[0], 7))
    raw[:, :3] = predictor64(params, prefix + '.outer_light', ol)
    out = {'direct': np.exp(np.minimum(raw[:, :3], exp_max))}
    out['light'] = out['direct']
    if probe:
        raw[:, 3:6] = predictor64(params, prefix + '.inner_light', il)
        raw[:, 6:] = predictor64(params, prefix + '.inner_weight', iw)
        occ_raw = 0.5 * raw[:, 6] + 0.5
        occ = np.clip(occ_raw, 0.0, 1.0)
        ind = np.exp(np.minimum(raw[:, 3:6], exp_max)) * occ[:, None]
        out.update(indirect=ind, occ=occ, occ_raw=occ_raw, light=ind + out['direct'] * (1.0 - occ[:, None]))
    out['raw'] = raw
    return out


def special_dirs():
    """[14,3] float64: the poles +-z (where (x + i y)^m vanishes for m > 0), the other axes, and the eight diagonals."""
    ax = [(0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0)]
    dg = [(sx, sy, sz) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    d = np.asarray(ax + dg, np.float64)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def rows(n, seed, rim=16):
    """Seed-generated query rows: (dirs [n,3] float32 unit vectors starting with special_dirs, rho [n] float32 cycling through
    0, 0.03, 0.5, 1, points [n,3] float32 inside the unit ball of which the last `rim` have 0.999 < |x| < 1: the branch of
    offset_points_to_sphere)."""
    g = np.random.Generator(np.random.PCG64(seed))
    d = g.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    sp = special_dirs()
    d[:min(n, len(sp))] = sp[:n]
    rho = np.asarray([0.0, 0.03, 0.5, 1.0], np.float32)[np.arange(n) % 4]
    u = g.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = 0.95 * g.random((n, 1)) ** (1.0 / 3.0)
    rim = min(rim, n)
    if rim:
        r[n - rim:] = 0.9992 + 0.0006 * g.random((rim, 1))
    x = (u * r).astype(np.float32)
    if rim:
        assert (np.linalg.norm(x[n - rim:].astype(np.float64), axis=1) > 0.999).all() and (np.linalg.norm(x.astype(np.float64), axis=1) < 1.0).all()
    return d.astype(np.float32), rho, x


OCC_GAIN = 30.0


def head_gain_overrides(params, occ_gain=OCC_GAIN, prefix='color_network'):
    """The seed-generated occlusion head is almost constant over the rows and never reaches a clamp.  Its gain (weight_g) times
    `occ_gain`, as the material fixtures do it: the occlusion then sits at a clamp on a quarter of the rows.  The exp heads keep their
    gain: at rho = 0 the 16th-degree terms of the IDE carry fp32 rounding noise of 1e-3 (tests/encode_oracle.py IDE_KAPPA) in ANY fp32
    evaluation, the reference's included (2.9e-5 of the radiance as it is, 8.6e-5 at a gain of 3, 8.4e-4 at 30), and a head gain
    multiplies it into the radiance; the radiance varies by 15 % over the rows, a thousand times the tolerance of the tests."""
    return {f'{prefix}.inner_weight.6.weight_g': (np.asarray(params[f'{prefix}.inner_weight.6.weight_g'], np.float64) * occ_gain).astype(np.float32)}


def clamp_overrides(params, dirs, rho, x, *, sphere=False, exp_max=3.0, pos_freq=6, prefix='color_network'):
    """Head overrides that put the rows on both sides of every clamp, from the float64 oracle alone: the bias of each exp head is
    moved so that the median raw value of its channel over the given rows is exp_max; the occlusion head's gain (weight_g) and bias
    are set so that 0.5 raw + 0.5 has the 25 % quantile at 0 and the 75 % quantile at 1 -- about a quarter of the rows in each
    clamped regime and half in the interior.  Returns {parameter name: float32 array}."""
    o = light64(params, dirs, rho, x, sphere=sphere, exp_max=exp_max, pos_freq=pos_freq, probe=True, prefix=prefix)
    over = {}
    for name, cols in (('outer_light', slice(0, 3)), ('inner_light', slice(3, 6))):
        b = np.asarray(params[f'{prefix}.{name}.6.bias'], np.float64)
        over[f'{prefix}.{name}.6.bias'] = (b + exp_max - np.median(o['raw'][:, cols], axis=0)).astype(np.float32)
    b = float(np.asarray(params[f'{prefix}.inner_weight.6.bias'], np.float64).reshape(-1)[0])
    gq = np.asarray(params[f'{prefix}.inner_weight.6.weight_g'], np.float64)
    lin = o['raw'][:, 6] - b                                   # the head without its bias: scales with the gain
    q25, q75 = np.quantile(lin, 0.25), np.quantile(lin, 0.75)
    gain = 2.0 / (q75 - q25)                                   # raw = -1 at q25 (occ 0), raw = +1 at q75 (occ 1)
    over[f'{prefix}.inner_weight.6.weight_g'] = (gq * gain).astype(np.float32)
    over[f'{prefix}.inner_weight.6.bias'] = np.asarray([-1.0 - gain * q25], np.float32)
    return over


def shares(o, exp_max):
    """Fractions of the rows in each regime of the float64 result `o` of light64(probe=True): (direct above exp_max in any channel,
    direct below in any channel, indirect above, indirect below, occ = 0, occ interior, occ = 1)."""
    r = o['raw']
    f = lambda m: float(np.mean(m))      # noqa: E731
    return (f((r[:, :3] > exp_max).any(1)), f((r[:, :3] < exp_max).any(1)), f((r[:, 3:6] > exp_max).any(1)), f((r[:, 3:6] < exp_max).any(1)),
            f(o['occ_raw'] <= 0.0), f((o['occ_raw'] > 0.0) & (o['occ_raw'] < 1.0)), f(o['occ_raw'] >= 1.0))
