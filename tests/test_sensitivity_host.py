"""Sensitivity post-processing on the host (nekstab_amd/sensitivity.py): the numpy restatement of core/sensitivity.f against
the reference's own bf_sensitivity output, mode files at another polynomial order, delta_forcing, and ts_gmres's mode keyword."""
import inspect
import os

import numpy as np

from nekstab_amd import mesh, mesh3d, nekio, newton
from nekstab_amd import sensitivity as S
from nekstab_amd.capi import NSK_NEWTON

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _modes(lx1):
    m = np.load(os.path.join(GOLDEN, "cylinder_modes.npz"))
    return [S.interp_gll(m[k + "_u"].astype(np.float64), lx1) for k in ("dRe", "dIm", "aRe", "aIm")]


def _wl2(g, a, b):
    return np.sqrt(g.inner(a - b, a - b, g.bm1) / g.inner(b, b, g.bm1))


def test_numpy_bf_sensitivity_reproduces_reference_output():
    """Direct modes at lx1 = 6, adjoint modes stored at lx1 = 8 read at 6 (as load_fld does), biorthogonalised, gradm1 + dsavg:
    the reference's sr_ / si_ within 1e-2 (bm1-weighted relative L2; the rest is the adjoint's resolution)."""
    case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6)
    g = S.NpGeom(case)
    dRe, dIm, aRe, aIm, gamma, delta = S.np_biorthogonalize(g, *_modes(6))
    assert abs(gamma - (-0.0230524)) < 1e-6 and abs(delta - 0.0120317) < 1e-6, (gamma, delta)
    out = S.np_bf_sensitivity(g, dRe, dIm, aRe, aIm)
    ref = np.load(os.path.join(GOLDEN, "cylinder_bf_sensitivity.npz"))
    for k in ("sr", "si"):
        r = ref[k + "_u"].astype(np.float64)
        err = _wl2(g, out[k], r)
        scale = g.inner(out[k], r, g.bm1) / g.inner(out[k], out[k], g.bm1)
        print(f"{k}: weighted L2 {err:.2e}, least-squares scale {scale:.5f}")
        assert err <= 1e-2
        assert abs(scale - 1.0) < 5e-3
    np.testing.assert_allclose(out["sr"], out["tr"] + out["pr"], rtol=0, atol=0)
    # after biorthogonalisation <a, d> = 1 + 0i and ||d|| = 1
    assert abs(g.inner(aRe, dRe) + g.inner(aIm, dIm) - 1.0) < 1e-12
    assert abs(g.inner(aRe, dIm) - g.inner(aIm, dRe)) < 1e-12
    assert abs(g.inner(dRe, dRe) + g.inner(dIm, dIm) - 1.0) < 1e-12


def test_order_change_round_trips_polynomials(tmp_path):
    """GLL -> GLL interpolation 6 -> 8 -> 6 is exact on polynomials of degree 5, in 2-D and 3-D; a mode file written at lx1 = 8
    loads at lx1 = 6."""
    rng = np.random.default_rng(3)
    from nekstab_amd.quadrature import gauss_lobatto_legendre
    r = gauss_lobatto_legendre(6)[0]
    c = rng.standard_normal((7, 6, 6))
    f2 = np.einsum("eab,ja,ib->eji", c, np.vander(r, 6, increasing=True), np.vander(r, 6, increasing=True))
    back = S.interp_gll(S.interp_gll(f2, 8), 6)
    assert np.max(np.abs(back - f2)) <= 1e-13 * max(1.0, np.max(np.abs(f2)))
    c3 = rng.standard_normal((3, 6, 6, 6))
    V = np.vander(r, 6, increasing=True)
    f3 = np.einsum("eabc,ka,jb,ic->ekji", c3, V, V, V)
    back3 = S.interp_gll(S.interp_gll(f3, 8, ndim=3), 6, ndim=3)
    assert np.max(np.abs(back3 - f3)) <= 1e-13 * max(1.0, np.max(np.abs(f3)))
    # a file at lx1 = 8 (the reference's adjoint files) read at lx1 = 6
    u8 = np.array([S.interp_gll(f2, 8), S.interp_gll(2.0 * f2, 8)])
    p8 = S.interp_gll(f2, 8)
    path = str(tmp_path / "aRe1cyl0.f00002")
    nekio.write_fld(path, u=u8[:, :, None], p=p8[:, None])
    u6, p4 = S.load_mode(path, 6)
    assert u6.shape == (2, 7, 6, 6) and p4.shape == (7, 4, 4)
    assert np.max(np.abs(u6[0] - f2)) <= 1e-12 * np.max(np.abs(f2))
    assert np.max(np.abs(u6[1] - 2.0 * f2)) <= 1e-12 * np.max(np.abs(f2))


def test_numpy_3d_restatement_on_extruded_cylinder_is_the_2d_one():
    """The 3-D restatement (cofactor metrics, 3 x 3 gradients) on the z-extruded cylinder gives the 2-D fields on every plane."""
    case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6)
    c3 = mesh3d.extrude_case(case, 2, 1.0)
    g2, g3 = S.NpGeom(case), S.NpGeom(c3)
    m2 = _modes(6)
    o2 = S.np_bf_sensitivity(g2, *m2)
    m3 = [np.array([mesh3d.extrude_field(a[0], 2), mesh3d.extrude_field(a[1], 2), np.zeros((c3.nel, 6, 6, 6))]) for a in m2]
    o3 = S.np_bf_sensitivity(g3, *m3)
    for k in ("sr", "si", "tr", "pi"):
        a = o3[k].reshape(3, 2, case.nel, 6, 6, 6)
        s = np.max(np.abs(o2[k]))
        for kz in range(2):
            for lev in range(6):
                assert np.max(np.abs(a[:2, kz, :, lev] - o2[k])) <= 1e-11 * s
        assert np.max(np.abs(a[2])) <= 1e-11 * s


def test_delta_forcing_is_pointwise():
    rng = np.random.default_rng(5)
    ub, fr, fi = (rng.standard_normal((2, 4, 6, 6)) for _ in range(3))
    dl, dw = S.delta_forcing(ub, fr, fi, alpha=2.0)
    w = np.hypot(ub[0], ub[1])
    np.testing.assert_allclose(dl, -2.0 * w * (fr[0] * ub[0] + fr[1] * ub[1]), rtol=1e-14)
    np.testing.assert_allclose(dw, 2.0 * w * (fi[0] * ub[0] + fi[1] * ub[1]), rtol=1e-14)


def test_ts_gmres_default_mode_is_newton():
    """ts_gmres gained mode=; its default keeps the Newton-Krylov system (exp(LT) - I)."""
    assert inspect.signature(newton.ts_gmres).parameters["mode"].default == NSK_NEWTON


def test_file_names_follow_outpost():
    assert S.fld_name("sr_", "1cyl") == "sr_1cyl0.f00001"
    assert S.fld_name("fsr", "1cyl") == "fsr1cyl0.f00001"
