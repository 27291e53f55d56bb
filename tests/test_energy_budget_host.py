"""The stability energy budget's numpy restatement (nekstab_amd/sensitivity.np_energy_budget, core/postproc.f:657-872) on the
host: closed-form production and dissipation on an undeformed box, and the budget of the committed cylinder mode."""
import os

import numpy as np

from nekstab_amd import mesh, mesh3d
from nekstab_amd import sensitivity as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_numpy_budget_matches_closed_form_on_undeformed_box():
    """Undeformed box at lx1 = 6, base flow and mode polynomials of degree <= 5 in each coordinate: gradm1 is exact and continuous,
    so dsavg changes nothing and the averaged Laplacian is exact.  Production and dissipation pointwise to 1e-10."""
    c = mesh3d.box_case_3d(2, 2, 2, 6, lengths=(2.0, 1.0, 0.8), origin=(-0.5, 0.2, 0.1))
    g = S.NpGeom(c)
    x, y, z = c.x, c.y, c.z
    ub = np.array([x * x * y + z, y * z * z - x, x * y * z])
    gU = [[2 * x * y, x * x, np.ones_like(x)],                       # d U_c / d x_j
          [-np.ones_like(x), z * z, 2 * y * z],
          [y * z, x * z, x * y]]
    dRe = np.array([x * y + 0.5, y * y * z, x - z ** 3])
    dIm = np.array([z * x * x, 1.0 + y ** 4, x * y * z])
    lapR = [np.zeros_like(x), 2 * z, -6 * z]
    lapI = [2 * z, 12 * y * y, np.zeros_like(x)]
    nu = 0.02
    out = S.np_energy_budget(g, ub, dRe, dIm, nu)
    a2 = g.inner(dRe, dRe) + g.inner(dIm, dIm)
    for ci in range(3):
        for j in range(3):
            ref = -0.5 * (dRe[ci] * dRe[j] + dIm[ci] * dIm[j]) * gU[ci][j] / a2
            assert np.max(np.abs(out["prod"][ci, j] - ref)) <= 1e-10 * np.max(np.abs(ref)), (ci, j)
            assert abs(out["integrals"][3 * ci + j] - np.sum(g.bm1 * ref)) <= 1e-10 * np.sum(g.bm1 * np.abs(ref))
    dref = 0.5 * nu * sum(dRe[j] * lapR[j] + dIm[j] * lapI[j] for j in range(3)) / a2
    assert np.max(np.abs(out["diss"] - dref)) <= 1e-10 * np.max(np.abs(dref))
    assert abs(out["integrals"][9] - np.sum(g.bm1 * dref)) <= 1e-10 * np.sum(g.bm1 * np.abs(dref))
    assert np.all(out["integrals"] != 0.0)


def test_numpy_budget_of_the_cylinder_mode():
    """The committed direct mode about the committed base flow (lx1 = 6, nu = 1/50): production P[1][2] feeds the instability,
    viscosity takes energy away, the budget's sum is positive (the mode grows); the third component's entries are 0 in 2-D;
    the budget does not depend on the mode's scale."""
    case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6)
    g = S.NpGeom(case)
    m = np.load(os.path.join(GOLDEN, "cylinder_modes.npz"))
    dRe, dIm = m["dRe_u"].astype(np.float64), m["dIm_u"].astype(np.float64)
    out = S.np_energy_budget(g, case.ub, dRe, dIm, 1.0 / case.re)
    I = out["integrals"]
    print("energy budget:", np.array2string(I, precision=4), "sum %.4e" % I.sum())
    assert np.all(I[[2, 5, 6, 7, 8]] == 0.0)
    assert I[1] > 0 and I[9] < 0 and I.sum() > 0
    assert abs(I[1] - 2.41e-2) < 5e-4 and abs(I[9] + 1.546e-2) < 5e-5 and abs(I.sum() - 1.04e-2) < 5e-4
    assert out["prod"].shape == (2, 2, case.nel, 6, 6) and out["diss"].shape == (case.nel, 6, 6)
    sc = S.np_energy_budget(g, case.ub, 3.0 * dRe, -3.0 * dIm, 1.0 / case.re)
    assert np.max(np.abs(sc["integrals"] - I)) <= 1e-13 * np.max(np.abs(I))


def test_kin_file_names_follow_outpost():
    assert [S.fld_name("KIN", "1cyl", c + 1) for c in range(3)] == ["KIN1cyl0.f00001", "KIN1cyl0.f00002", "KIN1cyl0.f00003"]
