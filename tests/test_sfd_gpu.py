"""Selective frequency damping on the device (nsk_sfd_map / nsk_group_sfd_map, nekstab_amd/fixedp.py; core/fixedp.f:114-242).

The algebra is pinned step by step: with chi = 0 against nsk_nonlinear_map (bits) and a numpy recursion of the filter; with
the force on against the CPU oracle, whose full-equation step takes a body force through its sponge term; then a fixed
point, the damping rate of the leading mode against the two-variable linear model, hexahedra and shards against the
quadrilateral single-rank map, the refusals and the driver.

BOUNDS of the hexahedral and the sharded comparison: not chosen, measured on the unforced 6-step nsk_nonlinear_map /
nsk_group_nonlinear_map (code this feature does not touch) at the same settings; the bound is ten times that difference
(the filter state on hexahedra has a bound of its own, from the maps of 1 .. 5 steps: see HEX_MEASURED).
`python -m tests.test_sfd_gpu` prints the tables the constants below were copied from, and the deviation of the damping
test from its model."""
import os

import numpy as np
import pytest

from tests import sym_box
from tests.conftest import GOLDEN, make_oracle

pytestmark = pytest.mark.gpu

CHI, OMEGA = 5.0, 20.0                 # large on purpose: omega_c dt ~ 0.2 on the cylinder fixture


# ---- the cylinder of tests/test_newton_gpu.py ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nosponge():
    from nekstab_amd import mesh
    from nekstab_amd.capi import NekStabHip
    case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6, spng_str=0.0)
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], tol_helm=1e-12, tol_pres=1e-3, tol_relative=1,
                   nproj=8, max_helm_iter=150, max_pres_iter=96)
    yield case, h
    h.close()


def _J12():
    from nekstab_amd.quadrature import gauss_legendre, gauss_lobatto_legendre, interp_matrix
    return interp_matrix(gauss_lobatto_legendre(6)[0], gauss_legendre(4)[0])


def _bf_state(case):
    J = _J12()
    return case.ub[0], case.ub[1], J @ case.meta["bf_p"] @ J.T


def _perturbed(case):
    q = _bf_state(case)
    return (q[0] * (1 + 0.05 * np.sin(case.y)), q[1] + 0.02 * np.cos(case.x) * case.mask, q[2])


_ORACLE = {}


def _oracle(case):
    """the test's OWN oracle instance (its sponge profile is set to 1 below: the channel of the body force)"""
    if "o" not in _ORACLE:
        o = make_oracle(case)
        o.set_baseflow(np.stack(_perturbed(case)[:2]))
        o.spng = np.ones_like(o.spng)
        _ORACLE["o"] = o
    return _ORACLE["o"]


def _sfd(h, q, qbar, chi, omega_c, nsteps):
    """one SFD map from host fields: (f, qbar at the end, residu)"""
    vq, vf, vb = h.alloc(3)
    h.upload(vq, *q)
    h.upload(vb, *qbar)
    h.set_nsteps(nsteps)
    res = h.sfd_map(vf, vq, vb, chi, omega_c)
    f, b = h.download(vf), h.download(vb)
    assert h.stats()["unconverged"] == 0
    h.free([vq, vf, vb])
    return f, b, res


def _plain(h, q, nsteps):
    vq, vf = h.alloc(2)
    h.upload(vq, *q)
    h.set_nsteps(nsteps)
    h.nonlinear_map(vf, vq)
    f = h.download(vf)
    h.free([vq, vf])
    return f


def _relw(a, b, w):
    return float(np.sqrt(sum(np.sum(w * (x - y) ** 2) for x, y in zip(a[:2], b[:2])) / sum(np.sum(w * y ** 2) for y in b[:2])))


def _start(case, h):
    """the perturbed start of test_nonlinear_steps_vs_oracle as the linearisation point, its tolerances"""
    q = _perturbed(case)
    vq, = h.alloc(1)
    h.upload(vq, *q)
    h.set_baseflow(vq)
    h.free([vq])
    h.set_tolerances(1e-13, 1e-8, 1)
    return q


def test_chi_zero_is_the_nonlinear_map_and_the_filter_is_the_numpy_recursion(nosponge):
    """A context of its own with "proj_reset" = 1: the pressure projection space of a quadrilateral context carries over from
    map to map, so two maps from one start return the same bits only when each starts from an empty space (or on fresh contexts
    with one history, as tests/test_sensitivity_gpu.py compares the forced map).  With it the first k steps of the 6-step map
    ARE the k-step map, and the recursion below sees the velocities the device's filter saw."""
    from nekstab_amd import fixedp
    from nekstab_amd.capi import NekStabHip
    case, _ = nosponge
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], tol_helm=1e-12, tol_pres=1e-3, tol_relative=1,
                   nproj=8, max_helm_iter=150, max_pres_iter=96)
    try:
        h.set_option("proj_reset", 1)
        q = _start(case, h)
        o = make_oracle(case, build_solvers=False)               # (for bm1 and the volume only)
        v = [q] + [_plain(h, q, k) for k in range(1, 7)]          # v^1 .. v^6 as maps of 1 .. 6 steps from the same start
        # the plain maps ran in the forms an SFD map does not take: convection fused into the right-hand side kernel, and (from
        # 3 steps on) captured graphs on per-step budgets or tails -- the bits below are equal across those forms
        st = h.stats()
        assert st["convfuse_steps"] > 0 and st["recaptures"] > 0
        f, qb, res = _sfd(h, q, q, 0.0, OMEGA, 6)
        assert h.stats()["convfuse_steps"] == st["convfuse_steps"] and h.stats()["recaptures"] == st["recaptures"]      # eager, unfused
        print("chi = 0 against nsk_nonlinear_map: max |difference|", [float(np.abs(a - b).max()) for a, b in zip(f, v[6])])
        assert np.abs(f[0]).max() > 0 and all(np.array_equal(a, b) for a, b in zip(f, v[6]))
        vel = [np.stack(x[:2]) for x in v]
        qref, rref = fixedp.np_sfd_filter(vel, vel[0], OMEGA, h.dt, volume=float(np.sum(o.bm1)), bm1=o.bm1[None])
        eq = np.abs(np.stack(qb[:2]) - qref).max() / np.abs(qref).max()
        er = np.abs(res / rref - 1.0).max()
        print("chi = 0: filter state %.2e, residu %.2e (relative)" % (eq, er), "residu", res)
        assert np.abs(qref - vel[0]).max() > 1e-3 * np.abs(qref).max()        # the filter moved
        assert eq <= 1e-13 and er <= 1e-13
        assert np.array_equal(qb[2], q[2])                        # the rest of qbar is not written
    finally:
        h.close()


def _oracle_sfd(o, q, qbar, splits, chi, omega_c):
    """SFD on the oracle by the reference's ordering: the maps of `splits` steps each restart the BDF / EXT ramp (new_state)
    and the filter's ramp, qbar is carried.  The force F = -chi (vxo - qbar) enters step_nonlinear as spng (vr - u) bm1 with
    spng = 1, vr = u + F.  Returns (u, v, p), qbar, residu."""
    vol = float(np.sum(o.bm1))
    qb = np.stack(qbar[:2]).copy()
    res = []
    for n in splits:
        st = o.new_state(q)
        vxo = np.stack([st["u"], st["v"]])                        # call 0
        ub = np.zeros_like(qb); uc = np.zeros_like(qb)
        F = -chi * (vxo - qb)
        for j in range(1, n + 1):
            st = o.step_nonlinear(st, j, 1.0, (st["u"] + F[0], st["v"] + F[1]))
            a, b, c = (1.5, -0.5, 0.0) if j <= 2 else (23.0 / 12.0, -16.0 / 12.0, 5.0 / 12.0)
            ua = vxo - qb                                         # call j: vxo is still v^{j-1}
            qb = qb + omega_c * o.dt * (a * ua + b * ub + c * uc)
            ub, uc = ua, ub
            F = -chi * (vxo - qb)
            vnew = np.stack([st["u"], st["v"]])
            res.append(np.sqrt(np.sum(o.bm1[None] * (vxo - vnew) ** 2) / vol))
            vxo = vnew
        q = (st["u"], st["v"], st["p"])
    return q, qb, np.array(res)


_ORACLE_RUNS = {}


def _oracle_run(case, splits):
    if splits not in _ORACLE_RUNS:
        q = _perturbed(case)
        _ORACLE_RUNS[splits] = _oracle_sfd(_oracle(case), q, q, splits, CHI, OMEGA)
    return _ORACLE_RUNS[splits]


@pytest.mark.parametrize("splits", [(8,), (5, 3)], ids=["one-map", "two-maps"])
def test_forced_steps_against_the_oracle(nosponge, splits):
    """f, qbar (bm1 norm) and every residu_j (relative to itself) within 1e-9 of the oracle.
    The solves are converged further than in test_nonlinear_steps_vs_oracle (1e-13 / 1e-8 there): residu is the norm of a
    velocity DIFFERENCE, 1.4e-4 of the velocity here, so 1e-9 of it is 1.5e-13 of the velocity -- below what a Helmholtz
    tolerance of 1e-13 leaves after 8 steps.  Measured on an MI355X, one map of 8 steps, (Helmholtz, pressure) tolerance ->
    f, qbar, worst residu_j:  (1e-13, 1e-8) 4.98e-13, 3.64e-13, 1.06e-9;  (1e-13, 1e-10) the same;  (1e-14, 1e-10) 6.6e-14,
    2.5e-14, 3.9e-12;  (1e-15, 1e-10) 8.8e-15, 2.4e-14, 4.9e-12.  The oracle solves directly."""
    case, h = nosponge
    try:
        q = _start(case, h)
        h.set_tolerances(1e-14, 1e-10, 1)
        o = _oracle(case)
        assert abs(h.dt - o.dt) < 1e-15
        ref, qref, rref = _oracle_run(case, splits)
        f, qb, res = q, q, []
        for n in splits:
            f, qb, r = _sfd(h, f, qb, CHI, OMEGA, n)
            res = np.concatenate([res, r])
        ev, eq = _relw(f, ref, o.bm1), _relw(qb, qref, o.bm1)
        er = np.abs(res / rref - 1.0).max()
        vn = np.sqrt(sum(np.sum(o.bm1 * y ** 2) for y in ref[:2]) / np.sum(o.bm1))
        print("SFD vs oracle, maps of", splits, "steps: f %.2e  qbar %.2e  residu %.2e (against the velocity's l2 norm: %.2e)"
              % (ev, eq, er, np.abs(res - rref).max() / vn))
        assert ev < 1e-9 and eq < 1e-9 and er < 1e-9
        # teeth, on the oracle alone: the force moves the result by more than a thousand bounds
        if "plain" not in _ORACLE_RUNS:
            _ORACLE_RUNS["plain"] = o.nonlinear_map(q, nsteps=8)
        teeth = _relw(ref, _ORACLE_RUNS["plain"], o.bm1)
        print("oracle, forced vs unforced: %.2e" % teeth)
        assert teeth > 1e-6
    finally:
        h.set_tolerances(1e-12, 1e-3, 1)


def _base(case, h):
    q = _bf_state(case)
    vq, = h.alloc(1)
    h.upload(vq, *q)
    h.set_baseflow(vq)
    return q, vq


def test_a_fixed_point_stays_one(nosponge):
    from nekstab_amd import fixedp
    case, h = nosponge
    q, vq = _base(case, h)
    assert h.nsteps == 100
    omega_c, chi = fixedp.sfd_parameters(0.12, 0.05)
    vf, vb = h.alloc(2)
    h.nonlinear_map(vf, vq, subtract_q=True)
    plain = h.norm(vf)
    h.copy(vb, vq)
    h.sfd_map(vf, vq, vb, chi, omega_c)
    h.axpy(vf, -1.0, vq)
    moved = h.norm(vf)
    T = 100 * h.dt
    print("|Phi_T(q) - q| = %.3e, |SFD_T(q) - q| = %.3e, factor allowed %.3f" % (plain, moved, 1 + chi * T))
    h.free([vq, vf, vb])
    assert moved <= (1 + chi * T) * plain


def _damping(case, h, modes, spectre, strouhal, T=5.0):
    """(A_plain / eps, A_sfd / eps, the model's ratio) of the leading direct mode over T time units"""
    from nekstab_amd import fixedp
    from tests.test_sfd_host import sfd_model_ratio
    omega_c, chi = fixedp.sfd_parameters(strouhal, 0.05)
    q, vq = _base(case, h)
    nst = int(round(T / h.dt))
    J = _J12()
    eps = 1e-3
    d = {k: (modes[k + "_u"][0].astype(np.float64), modes[k + "_u"][1].astype(np.float64), J @ modes[k + "_p"].astype(np.float64) @ J.T)
         for k in ("dRe", "dIm")}
    vd, vf, vb, v0 = h.alloc(4)
    nn = 0.0
    for k in d:
        h.upload(vd, *d[k])
        nn += h.norm(vd) ** 2
    s = eps / np.sqrt(nn)                                         # the MODE at unit norm: |Re|^2 + |Im|^2 = 1
    h.set_nsteps(nst)
    out = {}
    for kind in ("plain", "sfd"):
        res = {}
        for k in (None, "dRe", "dIm"):
            h.copy(v0, vq)
            if k:
                h.upload(vd, *d[k])
                h.axpy(v0, s, vd)
            if kind == "plain":
                h.nonlinear_map(vf, v0)
            else:
                h.copy(vb, v0)
                h.sfd_map(vf, v0, vb, chi, omega_c)
            res[k] = h.download(vf)
        a2 = 0.0
        for k in ("dRe", "dIm"):
            h.upload(vd, *[a - b for a, b in zip(res[k], res[None])])
            a2 += h.norm(vd) ** 2
        out[kind] = np.sqrt(a2) / eps
    h.free([vq, vd, vf, vb, v0])
    h.set_nsteps(100)
    lam = np.log(complex(spectre["Hd"][0, 0], spectre["Hd"][0, 1])) / 1.0
    return out["plain"], out["sfd"], sfd_model_ratio(lam, chi, omega_c, T)


def test_damping_of_the_leading_mode_follows_the_linear_model(nosponge, modes, spectre):
    """Casacuberta's parameters at St = 0.12, sigma = 0.05, T = 5: the model's ratio is 0.497.  Measured on an MI355X:
    A_plain = 1.0916, A_sfd = 0.5397, ratio 0.4944, 0.51 % below the model; Akervik's rule 0.7495 against 0.7495
    (DESIGN.md section 4.6)."""
    case, h = nosponge
    ap, asfd, model = _damping(case, h, modes, spectre, -0.12)
    print("A_plain / A_0 = %.4f, A_sfd / A_0 = %.4f, ratio %.4f, model %.4f (deviation %.2f %%)" % (ap, asfd, asfd / ap, model, 100 * (asfd / ap / model - 1)))
    assert abs(model - 0.497) < 1e-3
    assert ap > 1.0 and asfd < 1.0
    assert abs(asfd / ap / model - 1.0) <= 0.10


# ---- the channel of tests/sym_box.py: hexahedra and shards -----------------------------------------------------------------
KW = dict(tol_helm=1e-13, tol_pres=1e-11, tol_relative=1, schwarz_layers=2, max_helm_iter=200, max_pres_iter=144, nproj=8)
NCH = 6

# hexahedral vs quadrilateral nsk_nonlinear_map, z-invariant state, measured on an MI355X with `python -m tests.test_sfd_gpu`:
# (velocity in the bm1 norm after 6 steps, max |vz| / max |v| after 6 steps, the largest velocity difference over the maps of
# 1 .. 5 steps).  The bound of f, residu and vz is the issue's: 10 x the larger of the first two.  The filter state has a bound
# of its own: qbar^6 = qbar^0 + sum_j omega_c dt (a, b, c) . (v^{j-1} - qbar^{j-1}, ..) is a weighted sum of v^0 .. v^5 (weights of
# order omega_c dt each, of order one together) and never reads v^6; the two runs start from the same v^0, so its difference has
# the size of the largest difference among v^1 .. v^5 -- the third figure, which the first steps of this start (far from solenoidal) make
# ten times the 6-step one.  Bound of qbar: 10 x the third figure.
HEX_MEASURED = {
    6: (4.89e-13, 1.92e-13, 6.31e-12),     # per map length: 3.4e-12 6.3e-12 4.7e-12 2.9e-12 1.4e-12 4.9e-13; SFD: f 3.45e-12 vz 3.31e-12 qbar 7.94e-12 residu 4.44e-12
    8: (4.30e-13, 2.11e-13, 5.80e-12),     # per map length: 2.4e-12 5.4e-12 5.8e-12 3.0e-12 7.4e-13 4.3e-13; SFD: f 7.46e-13 vz 1.36e-12 qbar 2.65e-12 residu 3.72e-12
    10: (4.20e-13, 4.37e-13, 5.76e-12),    # per map length: 4.3e-12 4.1e-12 5.8e-12 2.5e-12 9.2e-13 4.2e-13; SFD: f 4.00e-13 vz 7.01e-13 qbar 1.07e-12 residu 1.38e-12
}
# nsk_group_nonlinear_map on R virtual ranks vs nsk_nonlinear_map after 6 steps: (ndim, lx1, R) -> velocity (quadrilaterals:
# bm1 norm; hexahedra: l2); the bound of f, qbar and residu is 10 x that
SHARD_MEASURED = {
    (2, 8, 2): 3.56e-14,         # SFD: f 7.07e-14 qbar 3.40e-14 residu 2.19e-14
    (2, 8, 3): 3.88e-14,         # SFD: f 7.23e-14 qbar 3.45e-14 residu 4.17e-14
    (3, 6, 2): 3.88e-14,         # SFD: f 1.61e-13 qbar 4.53e-14 residu 6.00e-15
    (3, 6, 3): 5.08e-14,         # SFD: f 1.58e-13 qbar 4.42e-14 residu 4.44e-15
}


def _bm1_2d(case):
    from tests.test_symmetry_gpu import _bm1
    return _bm1(case)


_CH = {}


def _channel(lx1, ndim):
    """(case, state, bm1, context) of the full channel; hexahedra: extruded over 2 periodic layers, z-invariant state"""
    from nekstab_amd import mesh3d
    from nekstab_amd.capi import NekStabHip
    c2, q2 = sym_box.case(lx1, False)
    w2 = _bm1_2d(c2)
    if ndim == 2:
        h = NekStabHip(c2, c2.meta["vert"], c2.meta["nvert"], **KW)
        # the classic GMRES iteration with a second Gram-Schmidt pass: at these tolerances, on a problem this small, the merged
        # iteration moves a quadrilateral map by 1e-2 between two tolerances (tests/test_symmetry_gpu.py)
        # "proj_reset": every map from an empty pressure projection space, as on hexahedra (the default there)
        for k, v in (("merged_iters", 0), ("gs2_from", 0), ("proj_reset", 1)):
            h.set_option(k, v)
        return c2, q2, w2, h
    c3 = mesh3d.extrude_case(c2, 2, 1.0, periodic=True)
    q3 = (mesh3d.extrude_field(q2[0], 2), mesh3d.extrude_field(q2[1], 2), np.zeros(c3.x.shape), mesh3d.extrude_pressure(q2[2], 2))
    return c3, q3, w2, NekStabHip(c3, c3.meta["vert"], c3.meta["nvert"], **KW)


def _run(be, q, ndim, sfd, nsteps=NCH):
    """`nsteps` steps from q: nonlinear map, or the SFD map with qbar = q; fields on the host (+ qbar, residu)"""
    up, down = (be.upload3, be.download3) if ndim == 3 else (be.upload, be.download)
    vq, vf, vb = be.alloc(3)
    up(vq, *q)
    be.set_nsteps(nsteps)
    if sfd:
        be.copy(vb, vq)
        res = be.sfd_map(vf, vq, vb, CHI, OMEGA)
        out = (down(vf), down(vb), res)
    else:
        be.nonlinear_map(vf, vq)
        out = (down(vf), None, None)
    be.free([vq, vf, vb])
    return out


def _quad(lx1, sfd, nsteps=NCH):
    key = ("quad", lx1, sfd, nsteps)
    if key not in _CH:
        c, q, w, h = _channel(lx1, 2)
        _CH[key] = _run(h, q, 2, sfd, nsteps) + (h.dt,)
        h.close()
    return _CH[key]


def _planes(f3, nel2):
    """the z planes of a hexahedral velocity field as quadrilateral fields: [(u, v), ..] over layers and GLL planes"""
    n = f3[0].shape[-1]
    return [(f3[0][l * nel2:(l + 1) * nel2, k], f3[1][l * nel2:(l + 1) * nel2, k]) for l in range(2) for k in range(n)]


def _hex_vs_quad(lx1, sfd, nsteps=NCH):
    """max over the z planes of |hex - quad| / |quad| (f; qbar), max |vz| / max |v|, max relative residu difference"""
    c3, q3, w2, h3 = _channel(lx1, 3)
    try:
        f2, b2, r2, dt2 = _quad(lx1, sfd, nsteps)
        assert h3.dt == dt2
        f3, b3, r3 = _run(h3, q3, 3, sfd, nsteps)
    finally:
        h3.close()
    nel2 = w2.shape[0]
    ev = max(_relw(p, f2, w2) for p in _planes(f3, nel2))
    vz = float(np.abs(f3[2]).max() / max(np.abs(f2[0]).max(), np.abs(f2[1]).max()))
    if not sfd:
        return ev, vz
    eb = max(_relw(p, b2, w2) for p in _planes(b3, nel2))
    bz = float(np.abs(b3[2]).max() / max(np.abs(b2[0]).max(), np.abs(b2[1]).max()))
    return ev, max(vz, bz), eb, float(np.abs(r3 / r2 - 1.0).max())


@pytest.mark.parametrize("lx1", [6, 8, 10])
def test_hexahedra_equal_quadrilaterals(lx1):
    bound, bound_q = 10.0 * max(HEX_MEASURED[lx1][:2]), 10.0 * HEX_MEASURED[lx1][2]
    ev, vz, eb, er = _hex_vs_quad(lx1, True)
    print("lx1 = %d, SFD hex vs quad: f %.2e  residu %.2e  vz %.2e  (bound %.2e)  qbar %.2e  (bound %.2e)" % (lx1, ev, er, vz, bound, eb, bound_q))
    assert ev <= bound and er <= bound and vz <= bound and eb <= bound_q


def _shards_vs_single(ndim, lx1, R, sfd, nsteps=NCH):
    from nekstab_amd.sharded import ShardGroup
    c, q, w2, h = _channel(lx1, ndim)
    try:
        one = _run(h, q, ndim, sfd, nsteps)
        g = ShardGroup(h, c, R)
        try:
            many = _run(g, q, ndim, sfd, nsteps)
            assert g.stats()["unconverged"] == 0
        finally:
            g.close()
    finally:
        h.close()
    nv = ndim
    rel = lambda a, b: float(np.sqrt(sum(np.sum((x - y) ** 2) for x, y in zip(a[:nv], b[:nv])) / sum(np.sum(y ** 2) for y in b[:nv])))
    if ndim == 2:
        rel = lambda a, b: _relw(a, b, w2)
    if not sfd:
        return rel(many[0], one[0])
    return rel(many[0], one[0]), rel(many[1], one[1]), float(np.abs(many[2] / one[2] - 1.0).max())


@pytest.mark.parametrize("key", sorted(SHARD_MEASURED), ids=lambda k: "%dd-lx%d-%dranks" % k)
def test_shards_equal_the_single_rank(key):
    """nsk_group_sfd_map returns ONE residu array, the sum over all ranks added in rank order: every rank receives it."""
    bound = 10.0 * SHARD_MEASURED[key]
    ev, eb, er = _shards_vs_single(*key, True)
    print(key, "SFD shards vs single rank: f %.2e  qbar %.2e  residu %.2e  (bound %.2e)" % (ev, eb, er, bound))
    assert ev <= bound and eb <= bound and er <= bound


def test_refusals():
    import ctypes as C
    from nekstab_amd.capi import NskError
    from nekstab_amd.sharded import ShardGroup
    case, _, _, h = _channel(6, 2)                               # (its own context: a lane and shards are cut from it)
    try:
        _refusals(h, case, C, NskError, ShardGroup)
    finally:
        h.close()


def _refusals(h, case, C, NskError, ShardGroup):
    h.set_nsteps(2)
    a, b, c = h.alloc(3)
    res = np.zeros(2)
    rp = res.ctypes.data_as(C.POINTER(C.c_double))
    lib = h.lib

    def refused(rc, who="nsk_sfd_map"):
        assert rc == -1 and who.encode() + b":" in lib.nsk_last_error(), (rc, lib.nsk_last_error())

    for f, q, qb in [(a, a, c), (a, b, a), (a, b, b), (None, b, c), (a, None, c), (a, b, None)]:
        refused(lib.nsk_sfd_map(h.ctx, f, q, qb, 1.0, 1.0, rp))
    refused(lib.nsk_sfd_map(None, a, b, c, 1.0, 1.0, rp))
    refused(lib.nsk_sfd_map(h.ctx, a, b, c, -1.0, 1.0, rp))
    refused(lib.nsk_sfd_map(h.ctx, a, b, c, 1.0, -1.0, rp))
    refused(lib.nsk_sfd_map(h.ctx, a, b, c, float("nan"), 1.0, rp))
    with pytest.raises(NskError) as e:
        h.sfd_map(a, a, c, 1.0, 1.0)
    assert e.value.code == -1 and "nsk_sfd_map" in str(e.value)
    # a lane
    h.add_lane()
    refused(lib.nsk_sfd_map(h._lanes[1], a, b, c, 1.0, 1.0, rp))
    # shards: the single-rank entry refuses them, the group entry refuses everything else
    g = ShardGroup(h, case, 2)
    try:
        x, y, z = g.alloc(3)
        refused(lib.nsk_sfd_map(g.ctx[0], x.parts[0], y.parts[0], z.parts[0], 1.0, 1.0, rp))
        one = lambda v: (C.c_void_p * 1)(v.value)
        refused(lib.nsk_group_sfd_map(one(h.ctx), 1, one(a), one(b), one(c), 1.0, 1.0, rp), "nsk_group_sfd_map")
        pr = g._per_rank
        refused(lib.nsk_group_sfd_map(g._arr, 2, pr(x), pr(x), pr(z), 1.0, 1.0, rp), "nsk_group_sfd_map")
        refused(lib.nsk_group_sfd_map(g._arr, 2, pr(x), pr(y), pr(x), 1.0, 1.0, rp), "nsk_group_sfd_map")
        refused(lib.nsk_group_sfd_map(g._arr, 2, pr(x), pr(y), pr(y), 1.0, 1.0, rp), "nsk_group_sfd_map")
        refused(lib.nsk_group_sfd_map(g._arr, 2, pr(x), pr(y), None, 1.0, 1.0, rp), "nsk_group_sfd_map")
        refused(lib.nsk_group_sfd_map(g._arr, 2, pr(x), pr(y), pr(z), -1.0, 1.0, rp), "nsk_group_sfd_map")
        refused(lib.nsk_group_sfd_map(g._arr, 2, pr(x), pr(y), pr(z), 1.0, -1.0, rp), "nsk_group_sfd_map")
        refused(lib.nsk_group_sfd_map(None, 2, pr(x), pr(y), pr(z), 1.0, 1.0, rp), "nsk_group_sfd_map")
        g.free([x, y, z])
    finally:
        g.close()
    h.free([a, b, c])


def test_rank_local_contexts_are_refused():
    import ctypes as C
    from nekstab_amd.sharded import local_parents
    c, _ = sym_box.case(6, False)
    parents, _ = local_parents(c, 2, **KW)
    try:
        p = parents[0]
        a, b, d = p.alloc(3)
        rc = p.lib.nsk_sfd_map(p.ctx, a, b, d, 1.0, 1.0, None)
        assert rc == -1 and b"nsk_sfd_map:" in p.lib.nsk_last_error()
    finally:
        for p in parents:
            p.close()


def test_driver_writes_the_reference_files(nosponge, tmp_path):
    from nekstab_amd import fixedp, nekio
    case, h = nosponge
    q, vq = _base(case, h)
    omega_c, chi = fixedp.sfd_parameters(0.12, 0.05)
    vf, vb, vw = h.alloc(3)
    h.copy(vb, vq)
    first = h.sfd_map(vf, vq, vb, chi, omega_c)
    tol = 2.0 * first.max()                                      # so that the `> 100 steps` rule is what decides
    out = str(tmp_path)
    ok, steps, hist = fixedp.sfd(h, vq, strouhal=0.12, sigma=0.05, tol=tol, max_time=50.0, outdir=out, ifvor=True)
    assert ok and steps == 101 and len(hist) == 101 and hist.max() < tol and h.nsteps == 100
    rows = open(os.path.join(out, "residu.dat")).read().splitlines()
    assert len(rows) == 101 and all(len(r) == 60 for r in rows)
    import re
    assert all(re.fullmatch(r"( [ -]0\.\d{7}E[+-]\d\d){4}", r) for r in rows)
    t = np.loadtxt(os.path.join(out, "residu.dat"))
    assert np.allclose(t[:, 1], hist, rtol=1e-6) and np.allclose(t[:, 0], h.dt * np.arange(1, 102), rtol=1e-6) and np.all(t[:, 3] == t[0, 3])
    prev = np.concatenate([[0.0], hist[:-1]])
    assert np.allclose(t[:, 2], (hist - prev) / h.dt, rtol=1e-5, atol=1e-7 * np.abs(hist).max() / h.dt)
    got = h.download(vq)
    bf = nekio.read_fld(os.path.join(out, "BF_1cyl0.f00001"))
    assert bf.wdsize == 8 and bf.istep == 101 and np.array_equal(bf.u[0, :, 0], got[0]) and np.array_equal(bf.u[1, :, 0], got[1])
    h.vorticity(vw, vq)
    w = h.download(vw)
    bfv = nekio.read_fld(os.path.join(out, "BFV1cyl0.f00001"))
    assert bfv.p is None and np.array_equal(bfv.u[0, :, 0], w[0].astype(np.float32).astype(np.float64)) and np.abs(w[0]).max() > 0
    h.free([vq, vf, vb, vw])


def test_driver_takes_a_shard_group(tmp_path):
    """fixedp.sfd on 2 virtual ranks of the channel (lx1 = 8) and on the single rank: `tol` above every residual, so both stop
    at step 101; the first map's first 6 residuals within the sharded bound (later steps are not bounded by a 6-step
    measurement), the files of the sharded run hold the sharded state and its vorticity."""
    from nekstab_amd import fixedp, nekio
    from nekstab_amd.sharded import ShardGroup
    c, q, w2, h = _channel(8, 2)
    try:
        runs = {}
        g = ShardGroup(h, c, 2)
        try:
            for name, be in (("one", h), ("two", g)):
                vq, vw = be.alloc(2)
                be.upload(vq, *q)
                out = os.path.join(str(tmp_path), name)
                ok, steps, hist = fixedp.sfd(be, vq, strouhal=0.12, sigma=0.05, tol=1e300, max_time=1e9, outdir=out, ifvor=True)
                be.vorticity(vw, vq)
                runs[name] = (ok, steps, hist, be.download(vq), be.download(vw), out)
                be.free([vq, vw])
        finally:
            g.close()
    finally:
        h.close()
    for ok, steps, hist, got, w, out in runs.values():
        assert ok and steps == 101 and len(hist) == 101 and len(open(os.path.join(out, "residu.dat")).read().splitlines()) == 101
        bf = nekio.read_fld(os.path.join(out, "BF_1cyl0.f00001"))
        assert bf.wdsize == 8 and np.array_equal(bf.u[0, :, 0], got[0]) and np.array_equal(bf.u[1, :, 0], got[1])
        bfv = nekio.read_fld(os.path.join(out, "BFV1cyl0.f00001"))
        assert np.array_equal(bfv.u[0, :, 0], w[0].astype(np.float32).astype(np.float64)) and np.abs(w[0]).max() > 0
    er = float(np.abs(runs["two"][2][:NCH] / runs["one"][2][:NCH] - 1.0).max())
    print("fixedp.sfd, 2 virtual ranks vs one: residu of steps 1 .. 6 %.2e (bound %.2e)" % (er, 10.0 * SHARD_MEASURED[(2, 8, 2)]))
    assert er <= 10.0 * SHARD_MEASURED[(2, 8, 2)]


def test_residu_is_identical_on_every_rank_of_two_processes():
    """Two ranks, one process each, sharing this GPU, sums over gloo on the host: the all-reduce branch of the residual sums."""
    import subprocess
    import sys
    from tests.conftest import ROOT
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29687", os.path.join(ROOT, "tests", "mp_sfd_worker.py")],
                         capture_output=True, text=True, timeout=600, env=env)
    print([l for l in out.stdout.splitlines() if "MPSFD" in l], out.stderr[-1500:] if out.returncode else "")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count("MPSFD rank") == 2


if __name__ == "__main__":      # the tables behind HEX_MEASURED / SHARD_MEASURED, and the figures of the damping test
    for lx1 in (6, 8, 10):
        m = [_hex_vs_quad(lx1, False, k) for k in range(1, NCH + 1)]
        print("    %d: (%.2e, %.2e, %.2e)," % (lx1, m[-1][0], m[-1][1], max(x[0] for x in m[:-1])), "   # per map length:", " ".join("%.1e" % x[0] for x in m),
              "; SFD: f %.2e vz %.2e qbar %.2e residu %.2e" % _hex_vs_quad(lx1, True), flush=True)
    for key in sorted(SHARD_MEASURED):
        m = [_shards_vs_single(*key, False, k) for k in range(1, NCH + 1)]
        print("    %r: %.2e," % (key, m[-1]), "   # per map length:", " ".join("%.1e" % x for x in m),
              "; SFD: f %.2e qbar %.2e residu %.2e" % _shards_vs_single(*key, True), flush=True)
    from nekstab_amd import mesh
    from nekstab_amd.capi import NekStabHip
    case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6, spng_str=0.0)
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], tol_helm=1e-12, tol_pres=1e-3, tol_relative=1, nproj=8, max_helm_iter=150, max_pres_iter=96)
    md, sp = np.load(os.path.join(GOLDEN, "cylinder_modes.npz")), np.load(os.path.join(GOLDEN, "cylinder_spectre.npz"))
    for st in (-0.12, 0.12):
        ap, asfd, model = _damping(case, h, md, sp, st)
        print("St = %+.2f: A_plain %.4f A_sfd %.4f ratio %.4f model %.4f deviation %.2f %%" % (st, ap, asfd, asfd / ap, model, 100 * (asfd / ap / model - 1)), flush=True)
    h.close()
