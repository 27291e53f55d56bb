"""Selective frequency damping, host side (nekstab_amd/fixedp.py): the two parameter rules of core/fixedp.f:137-152, the
Adams-Bashforth schedule of the filter, the residu.dat writer, the numpy restatement of the filter the device is tested
against, and the linear model of tests/test_sfd_gpu.py's damping test."""
import math
import os

import numpy as np
import pytest

from nekstab_amd import fixedp


def test_sfd_parameters_both_rules():
    w, chi = fixedp.sfd_parameters(0.12, 0.05)                 # Akervik 2006
    assert abs(w - 0.376991118430775) < 1e-14 and abs(chi - 0.1) < 1e-16
    w, chi = fixedp.sfd_parameters(-0.12, 0.05)                # Casacuberta 2018
    r = math.sqrt((2 * math.pi * 0.12) ** 2 + 0.05 ** 2)
    assert abs(w - 0.5 * (r - 0.05)) < 1e-15 and abs(chi - 0.5 * (r + 0.05)) < 1e-15
    assert abs(w - 0.352819) < 1e-6 and abs(chi - 0.402819) < 1e-6
    assert abs(chi - w - 0.05) < 1e-15 and abs(chi * w - (math.pi * 0.12) ** 2) < 1e-15
    # the sign of sigma is dropped, the sign of the Strouhal number selects the rule
    assert fixedp.sfd_parameters(0.12, -0.05) == fixedp.sfd_parameters(0.12, 0.05)


def test_ab_coefficient_schedule():
    assert fixedp.ab_coefficients(1) == (1.5, -0.5, 0.0) and fixedp.ab_coefficients(2) == (1.5, -0.5, 0.0)
    for j in (3, 4, 100):
        a, b, c = fixedp.ab_coefficients(j)
        assert (a, b, c) == (23.0 / 12.0, -16.0 / 12.0, 5.0 / 12.0) and abs(a + b + c - 1.0) < 1e-15
    with pytest.raises(ValueError):
        fixedp.ab_coefficients(0)


def test_numpy_filter_follows_the_call_order():
    """Three calls written out by hand: call j reads v^{j-1} (vxo), never v^j."""
    v = [np.array([1.0]), np.array([2.0]), np.array([4.0]), np.array([8.0])]
    w, dt = 0.5, 0.1
    q, res = fixedp.np_sfd_filter(v, np.array([0.0]), w, dt, volume=2.0, bm1=np.array([2.0]))
    u1 = 1.0 - 0.0
    q1 = 0.0 + w * dt * 1.5 * u1
    u2 = 2.0 - q1
    q2 = q1 + w * dt * (1.5 * u2 - 0.5 * u1)
    u3 = 4.0 - q2
    q3 = q2 + w * dt * (23.0 / 12.0 * u3 - 16.0 / 12.0 * u2 + 5.0 / 12.0 * u1)
    assert abs(q[0] - q3) < 1e-15
    assert np.allclose(res, [1.0, 2.0, 4.0], rtol=1e-15)
    # a steady input is a fixed point of the filter once qbar = v
    q, res = fixedp.np_sfd_filter([np.ones(3)] * 5, np.ones(3), w, dt, volume=1.0, bm1=np.ones(3))
    assert np.array_equal(q, np.ones(3)) and not res.any()


def test_residu_writer(tmp_path):
    line = fixedp.residu_line(0.01, 1.2345678e-5, -3.5e-4, 1e-8)
    assert line == "  0.1000000E-01  0.1234568E-04 -0.3500000E-03  0.1000000E-07" and len(line) == 60
    assert fixedp.residu_line(1.0, 0.0, 0.99999999, 123.456) == "  0.1000000E+01  0.0000000E+00  0.1000000E+01  0.1234560E+03"
    p = os.path.join(tmp_path, "residu.dat")
    fixedp.write_residu(p, [(0.1, 2.0, 20.0, 1e-6), (0.2, 1.0, -10.0, 1e-6)])
    rows = open(p).read().splitlines()
    assert len(rows) == 2 and all(len(r) == 60 for r in rows)
    assert np.array_equal(np.loadtxt(p), [[0.1, 2.0, 20.0, 1e-6], [0.2, 1.0, -10.0, 1e-6]])


def sfd_model_ratio(lam, chi, omega_c, T):
    """|a(T)| / |exp(lam T)| of a' = (lam - chi) a + chi b, b' = omega_c (a - b), a(0) = b(0) = 1: what SFD leaves of a mode
    with eigenvalue lam, relative to the undamped flow."""
    from scipy.linalg import expm
    M = np.array([[lam - chi, chi], [omega_c, -omega_c]], dtype=complex)
    a = (expm(M * T) @ np.ones(2))[0]
    return abs(a) / abs(np.exp(lam * T))


def test_linear_model_of_the_damping_test(spectre):
    """The ratios the issue quotes for the leading mode of the committed spectrum (0.0157 + 0.757 i)."""
    mu = complex(spectre["Hd"][0, 0], spectre["Hd"][0, 1])
    lam = np.log(mu) / 1.0
    assert abs(lam - complex(*spectre["NSd"][0, :2])) < 1e-6
    w, chi = fixedp.sfd_parameters(-0.12, 0.05)
    assert abs(sfd_model_ratio(lam, chi, w, 5.0) - 0.497) < 1e-3 and abs(sfd_model_ratio(lam, chi, w, 10.0) - 0.125) < 1e-3
    w, chi = fixedp.sfd_parameters(0.12, 0.05)
    assert abs(sfd_model_ratio(lam, chi, w, 5.0) - 0.749) < 1e-3 and abs(sfd_model_ratio(lam, chi, w, 10.0) - 0.492) < 1e-3
