"""Vortex identification (lambda2, Q, Omega: vortex_core of nekStab_outpost's vox / omg files), host side: the filter matrix of
filter_s0 and the numpy restatement sensitivity.np_vortex_criteria against closed forms.  No GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

from nekstab_amd import mesh3d
from nekstab_amd import sensitivity as S
from nekstab_amd.quadrature import gauss_lobatto_legendre


def _phi_last(lx1, z):
    """phi_{lx1-1} = L_{lx1-1} - L_{lx1-3} at the points z"""
    c = np.zeros(lx1)
    c[lx1 - 1], c[lx1 - 3] = 1.0, -1.0
    return np.polynomial.legendre.legval(z, c)


@pytest.mark.parametrize("lx1", [6, 8, 10, 12])
def test_filter_matrix_keeps_low_degrees_and_damps_the_last_mode(lx1):
    z = gauss_lobatto_legendre(lx1)[0]
    for w in (0.5, 0.05, 1.0):
        F = S.gll_filter_matrix(lx1, w)
        assert F.shape == (lx1, lx1)
        for deg in range(lx1 - 1):                                                  # monomials up to degree lx1 - 2
            p = z ** deg
            assert np.linalg.norm(F @ p - p) <= 1e-12 * np.linalg.norm(p), (w, deg)
        ph = _phi_last(lx1, z)
        assert np.linalg.norm(F @ ph - (1.0 - w) * ph) <= 1e-12 * np.linalg.norm(ph), w
    assert np.array_equal(S.gll_filter_matrix(lx1, 0.0), np.eye(lx1))              # exactly
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            S.gll_filter_matrix(lx1, bad)


def _one_quad(lx1=6):
    """an undeformed single-element 2-D mesh, [0.5, 2.5] x [-1, 0.5], with what NpGeom reads"""
    z = gauss_lobatto_legendre(lx1)[0]
    x = np.broadcast_to(1.5 + z[None, :], (lx1, lx1))[None].copy()
    y = np.broadcast_to(-0.25 + 0.75 * z[:, None], (lx1, lx1))[None].copy()
    return SimpleNamespace(ndim=2, lx1=lx1, nel=1, x=x, y=y, gid=np.arange(lx1 * lx1).reshape(1, lx1, lx1), nglob=lx1 * lx1,
                           spng=np.zeros((1, lx1, lx1)))


def _one_hex(lx1=6):
    return mesh3d.box_case_3d(1, 1, 1, lx1, lengths=(2.0, 1.5, 0.8), origin=(0.5, -1.0, 0.2), warp=0.0)


def _fields(c, f2):
    """the velocity (f2(x, y) [, 0]) on the case c"""
    u = list(f2(c.x, c.y))
    if c.ndim == 3:
        u.append(np.zeros_like(c.x))
    return np.array(u)


@pytest.mark.parametrize("nd", [2, 3])
def test_solid_body_rotation(nd):
    """u = (-y, x [, 0]): S = 0, O O = -diag(1, 1 [, 0]); lambda2 = -1 in both dimensions (3-D: the middle of 0, -1, -1), Q = 2 in
    2-D (the reference's form) and 1 in 3-D, Omega = b / (b + 1e-5) with b = (||O||_F^2)^2 = 4."""
    c = _one_quad() if nd == 2 else _one_hex()
    lam, q, om = S.np_vortex_criteria(S.NpGeom(c), _fields(c, lambda x, y: (-y, x)), wght=0.0)
    assert lam.shape == q.shape == om.shape == c.x.shape
    assert np.max(np.abs(lam + 1.0)) <= 1e-12
    assert np.max(np.abs(q - (2.0 if nd == 2 else 1.0))) <= 1e-12
    assert np.max(np.abs(om - 4.0 / (4.0 + 1e-5))) <= 1e-12
    # constants pass the filter unchanged
    lam5, q5, om5 = S.np_vortex_criteria(S.NpGeom(c), _fields(c, lambda x, y: (-y, x)), wght=0.5)
    assert np.max(np.abs(lam5 + 1.0)) <= 1e-12 and np.max(np.abs(om5 - om)) <= 1e-12 and np.max(np.abs(q5 - q)) <= 1e-12


@pytest.mark.parametrize("nd", [2, 3])
def test_pure_strain(nd):
    """u = (x, -y [, 0]): O = 0, S S = diag(1, 1 [, 0]); lambda2 = 1 (2-D: the smaller of 1, 1; 3-D: the middle of 0, 1, 1),
    Omega = 0 exactly in the limit (b = 0), Q = 2 det g = -2 in 2-D and -1 in 3-D."""
    c = _one_quad() if nd == 2 else _one_hex()
    lam, q, om = S.np_vortex_criteria(S.NpGeom(c), _fields(c, lambda x, y: (x, -y)), wght=0.0)
    assert np.max(np.abs(lam - 1.0)) <= 1e-12
    assert np.all(q < 0.0) and np.max(np.abs(q - (-2.0 if nd == 2 else -1.0))) <= 1e-12
    assert np.max(np.abs(om)) <= 1e-20                                              # b = O(eps^4) over 1e-5


def test_eigenvalue_ordering_on_a_field_with_three_distinct_eigenvalues():
    """u = (2 x, -0.5 y, -1.5 z): O = 0, S S = diag(4, 0.25, 2.25): lambda2 is the middle one, 2.25; Q = -1 - 3 + 0.75."""
    c = _one_hex()
    u = np.array([2.0 * c.x, -0.5 * c.y, -1.5 * c.z])
    lam, q, om = S.np_vortex_criteria(S.NpGeom(c), u, wght=0.0)
    assert np.max(np.abs(lam - 2.25)) <= 1e-12
    assert np.max(np.abs(q - (2.0 * -0.5 + -0.5 * -1.5 + -1.5 * 2.0))) <= 1e-12


def test_the_3d_q_of_a_z_invariant_field_is_half_the_2d_q():
    """the same (non-polynomial) field on the quadrilateral and on the hexahedron over it: Q_3D = det g, Q_2D = 2 det g;
    lambda2 and Omega agree"""
    lx1 = 8
    c2 = _one_quad(lx1)
    c3 = mesh3d.box_case_3d(1, 1, 1, lx1, lengths=(2.0, 1.5, 0.8), origin=(0.5, -1.0, 0.2), warp=0.0)
    f = lambda x, y: (np.sin(0.7 * x) * np.cos(0.4 * y) + 0.3 * x * y, 0.5 * np.cos(0.6 * x + 0.2) * np.sin(0.9 * y) - 0.2 * x * x)
    for w in (0.0, 0.5):
        l2, q2, o2 = S.np_vortex_criteria(S.NpGeom(c2), _fields(c2, f), wght=w)
        l3, q3, o3 = S.np_vortex_criteria(S.NpGeom(c3), _fields(c3, f), wght=w)
        s = np.max(np.abs(q2))
        for k in range(lx1):                                                        # every z-level of the hexahedron
            assert np.max(np.abs(2.0 * q3[0, k] - q2[0])) <= 1e-12 * s, (w, k)
            assert np.max(np.abs(o3[0, k] - o2[0])) <= 1e-12, (w, k)
    # lambda2: A_3D = diag(A_2D, 0), so the middle of its three is the middle of A_2D's two eigenvalues and 0
    lam2, _, _= S.np_vortex_criteria(S.NpGeom(c2), _fields(c2, f), wght=0.0)
    lam3, _, _ = S.np_vortex_criteria(S.NpGeom(c3), _fields(c3, f), wght=0.0)
    g = S.NpGeom(c2)
    G = np.array([g.grad(a) for a in _fields(c2, f)])
    Sm, Om = 0.5 * (G + G.transpose(1, 0, 2, 3, 4)), 0.5 * (G - G.transpose(1, 0, 2, 3, 4))
    A = np.einsum("ikeyx,kjeyx->eyxij", Sm, Sm) + np.einsum("ikeyx,kjeyx->eyxij", Om, Om)
    ev = np.linalg.eigvalsh(A)                                                      # ascending pairs
    mid = np.sort(np.concatenate([ev, np.zeros(ev.shape[:-1] + (1,))], axis=-1), axis=-1)[..., 1]
    assert np.max(np.abs(lam2 - ev[..., 0])) <= 1e-13 * np.max(np.abs(ev))
    for k in range(lx1):
        assert np.max(np.abs(lam3[0, k] - mid[0])) <= 1e-12 * np.max(np.abs(ev)), k
