"""The float64 restatements of tests/encode_oracle.py against data recorded from the original project (tests/golden/ops.npz), the
stage-1 oracle and closed forms -- on the CPU, before tests/test_encode_ops_gpu.py compares a kernel with them."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encode_oracle as EO
from helpers import golden
from oracle import stage1_oracle as O


@pytest.fixture(scope="module")
def ops():
    return golden("ops.npz")


def test_ide64_reproduces_the_recorded_ide_and_the_stage1_oracle(ops, monkeypatch):
    d, k = torch.from_numpy(ops['ide_dirs']).double(), torch.from_numpy(ops['ide_kappa']).double()
    got = EO.ide64(d, k)
    assert got.shape == (64, 72) and got.dtype == torch.float64
    # the recorded vectors are fp32 results of the original (tests/test_oracle_golden.py::test_ide holds the fp32 oracle to the same)
    np.testing.assert_allclose(got.numpy(), ops['ide_out'], rtol=1e-4, atol=2e-6)
    # the oracle's formula (complex powers, z ** i) in float64 (its fp32 tables widened, the values unchanged): only the order of
    # operations differs
    monkeypatch.setattr(O, '_IDE_MAT', O._IDE_MAT.astype(np.float64))
    monkeypatch.setattr(O, '_IDE_ML', O._IDE_ML.astype(np.float64))
    ref = O.ide(d, k)
    assert ref.dtype == torch.float64
    scale = float(ref.abs().max())
    assert float((got - ref).abs().max()) <= 1e-12 * scale


def test_embed64_equals_the_stage1_oracle_embedding_and_the_recorded_one(ops):
    x = torch.from_numpy(ops['embed6_in']).double()
    got = EO.embed64(x, 6)
    assert got.shape == (64, 39)
    assert torch.equal(got, O.embed(x, 6))
    np.testing.assert_allclose(got.numpy(), ops['embed6_out'], rtol=0, atol=5e-6)
    x4 = torch.randn(9, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert torch.equal(EO.embed64(x4, 10), O.embed(x4, 10)) and EO.embed64(x4, 10).shape == (9, 84)


def test_embed_columns_describe_the_jacobian_of_embed64():
    for dim, n_freq in ((3, 6), (4, 10), (3, 4)):
        x = torch.randn(5, dim, dtype=torch.float64, generator=torch.Generator().manual_seed(dim)).requires_grad_(True)
        e = EO.embed64(x, n_freq)
        c, f, partner, sign = EO.embed_columns(dim, n_freq)
        for col in range(e.shape[1]):
            (g,) = torch.autograd.grad(e[:, col].sum(), x, retain_graph=True)
            want = torch.zeros_like(g)
            want[:, c[col]] = 1.0 if partner[col] < 0 else f[col] * sign[col] * e[:, partner[col]].detach()
            torch.testing.assert_close(g, want, rtol=1e-13, atol=1e-13)


def test_ide_of_a_unit_direction_at_kinv_0_has_the_analytic_l1_terms():
    d = F.normalize(torch.randn(33, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(2)), dim=-1)
    out = EO.ide64(d, torch.zeros(33, 1, dtype=torch.float64))
    # terms 0, 1 are (m, l) = (0, 1), (1, 1): Y_1^0 = sqrt(3 / 4 pi) z, Y_1^1 = -sqrt(3 / 8 pi) (x + i y)
    assert EO.IDE_M[:2].tolist() == [0, 1] and EO.IDE_L[:2].tolist() == [1.0, 1.0]
    a, b = math.sqrt(3.0 / (4.0 * math.pi)), -math.sqrt(3.0 / (8.0 * math.pi))
    # the table is stored in fp32: 2^-24 relative on each coefficient
    torch.testing.assert_close(out[:, 0], a * d[:, 2], rtol=1e-7, atol=0)
    assert float(out[:, 36].abs().max()) == 0.0
    torch.testing.assert_close(out[:, 1], b * d[:, 0], rtol=1e-7, atol=0)
    torch.testing.assert_close(out[:, 37], b * d[:, 1], rtol=1e-7, atol=0)
    # and kinv scales term i by exp(-l (l + 1) / 2 kinv)
    k = torch.rand(33, 1, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    att = torch.exp(-EO.IDE_SIGMA * k)
    torch.testing.assert_close(EO.ide64(d, k), out * torch.cat([att, att], -1), rtol=1e-14, atol=0)


def test_shade_dirs_sphere_point_and_nerf_inputs_against_the_stage1_oracle():
    g = torch.Generator().manual_seed(4)
    n, d = 1.7 * torch.randn(50, 3, dtype=torch.float64, generator=g), 0.6 * torch.randn(50, 3, dtype=torch.float64, generator=g)
    nh, vh, nov, r, inorm = EO.shade_dirs64(n, d)
    torch.testing.assert_close(nh, F.normalize(n, dim=-1), rtol=1e-14, atol=0)
    torch.testing.assert_close(vh, F.normalize(-d, dim=-1), rtol=1e-14, atol=0)
    torch.testing.assert_close(inorm[:, 0], 1.0 / n.norm(dim=-1), rtol=1e-14, atol=0)
    # r is the mirror image of v^ about n^: unit length, same cosine with n^
    torch.testing.assert_close(r.norm(dim=-1), torch.ones(50, dtype=torch.float64), rtol=1e-14, atol=0)
    torch.testing.assert_close((r * nh).sum(-1), nov[:, 0], rtol=1e-13, atol=1e-15)
    x = F.normalize(torch.randn(50, 3, dtype=torch.float64, generator=g), dim=-1) * torch.linspace(0.2, 1.2, 50, dtype=torch.float64)[:, None]
    s = EO.sphere_point64(x, r)
    sp = O.offset_points_to_sphere(x)
    want = F.normalize(sp + r * O.sphere_exit_distance(sp, r), dim=-1)
    torch.testing.assert_close(s, want, rtol=1e-13, atol=1e-15)
    assert int((x.norm(dim=-1) > 0.999).sum()) > 5 and int((x.norm(dim=-1) < 0.999).sum()) > 5
    xo = x * 6.0
    xh, inv = EO.nerf_inputs64(xo)
    torch.testing.assert_close(xh * xo.norm(dim=-1, keepdim=True), xo, rtol=1e-14, atol=0)
    torch.testing.assert_close(inv[:, 0] * xo.norm(dim=-1), torch.ones(50, dtype=torch.float64), rtol=1e-14, atol=0)


def test_shade_rows64_layout():
    g = torch.Generator().manual_seed(5)
    P = 7
    E = torch.randn(P, 39, dtype=torch.float64, generator=g)
    x = 0.5 * torch.randn(P, 3, dtype=torch.float64, generator=g)
    dirs = EO.shade_dirs64(torch.randn(P, 3, dtype=torch.float64, generator=g), torch.randn(P, 3, dtype=torch.float64, generator=g))
    nh, vh, nov, r, inorm = dirs
    rho = torch.rand(P, 1, dtype=torch.float64, generator=g)
    one, zero = torch.ones_like(rho), torch.zeros_like(rho)
    for sphere, rdim in ((0, 39), (1, 15)):
        rows = EO.shade_rows64(E, x, *dirs, rho, sphere, rdim)
        assert rows['OLin'].shape == (3 * P, 144 if sphere else 72) and rows['ILin'].shape == (2 * P, 111)
        assert rows['IWin'].shape == (P, 78) and rows['RLin'].shape == (P, 2 * rdim) and rows['SD'].shape == (P, 8)
        assert torch.equal(rows['OLin'][:P, :72], EO.ide64(nh, one)) and torch.equal(rows['OLin'][P:2 * P, :72], EO.ide64(r, rho))
        assert torch.equal(rows['OLin'][2 * P:, :72], EO.ide64(r, zero))
        if sphere:
            sr = EO.sphere_point64(x, r)
            assert torch.equal(rows['OLin'][:P, 72:], EO.ide64(EO.sphere_point64(x, nh), one))
            assert torch.equal(rows['OLin'][P:2 * P, 72:], EO.ide64(sr, rho)) and torch.equal(rows['OLin'][2 * P:, 72:], EO.ide64(sr, rho))
        assert torch.equal(rows['ILin'][:P, :39], E) and torch.equal(rows['ILin'][P:, :39], E)
        assert torch.equal(rows['ILin'][:P, 39:], rows['OLin'][P:2 * P, :72]) and torch.equal(rows['ILin'][P:, 39:], rows['OLin'][2 * P:, :72])
        assert torch.equal(rows['IWin'][:, 39:], O.embed(r, 6))
        assert torch.equal(rows['RLin'][:, :rdim], E[:, :rdim]) and torch.equal(rows['RLin'][:, rdim:], O.embed(vh, (rdim - 3) // 6))
        assert torch.equal(rows['SD'][:, :6], torch.cat([nh, nov, inorm, rho], -1)) and float(rows['SD'][:, 6:].abs().max()) == 0.0
