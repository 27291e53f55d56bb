"""Hexahedral kernels under axis relabelling and rigid rotation (helper: tests/axes3d.py).

The equations are covariant: relabelling every element's local axes (r, s, t) by a proper signed permutation and moving the frame
by an orthogonal matrix must return the same map, re-expressed.  Base geometry: axes3d.inplane_case, a z-extruded, in-plane curved
outflow case with a two-dimensional base flow and a sponge (3 x 2 elements in plane, 2 periodic layers; 2 x 2 x 2 at lx1 = 10).
Orientation (A, C): the spanwise direction lies on local axis A and on coordinate C.

What this closes: (1) the load-skipping of arrays that vanish on the whole mesh (Dev::zmask, Dev::bfmask) had run with two
zero patterns, both symmetric under a <-> c -- here every one of the nine (A, C) patterns runs, and a kernel that tests bit
c*3+a for a*3+c, or takes g5's bit for g6, fails; (2) the hexahedral kernels are tied to the quadrilateral kernels (which are
pinned to reference-held data) with the spanwise direction on each local axis in turn and obliquely, so the w equation, the z
rows of the metric tensor and the t direction of the Gauss-mesh operators are each held to a pinned term."""
import numpy as np
import pytest

from nekstab_amd import mesh3d
from tests import axes3d

pytestmark = pytest.mark.gpu

TOL = dict(tol_helm=1e-12, tol_pres=1e-8, tol_relative=1, max_helm_iter=200, max_pres_iter=48)          # tests/test_3d_gpu.py
PROD = dict(tol_helm=1e-11, tol_pres=1e-4, tol_relative=1, max_helm_iter=150, max_pres_iter=48, nproj=8)   # test_extruded_cylinder_matches_2d

_CYC = (1, 2, 0)
# named orientations: (local, Q)
ORIENT = {"A%dC%d" % (A, C): axes3d.orientation(A, C) for A in range(3) for C in range(3)}
ORIENT.update({
    "base": (axes3d.IDENTITY, np.eye(3)),
    # asymmetric, with flips: (b)
    "A0C1-flip": axes3d.orientation(0, 1, (1, -1, -1)),
    "A1C0-flip": axes3d.orientation(1, 0, (-1, 1, 1)),
    "oblique": ((_CYC, (1, 1, 1)), axes3d.oblique()),
    # one per A, with flips: (c)
    "A0C2-flip": axes3d.orientation(0, 2, (-1, 1, 1)),
    "A1C0-flip2": axes3d.orientation(1, 0, (1, 1, -1)),
    "A2C1-flip": axes3d.orientation(2, 1, (1, -1, 1)),
})


def expected_zero_bits(A, C):
    """The bits of stats()['zero_arrays'] with the spanwise direction on local axis A and coordinate C, from (A, C) alone.

    Metric term 3a + c = J d(xi_a)/d(x_c) vanishes iff exactly one of a, c is spanwise: (a == A) xor (c == C).
    G factors: bit 9 is (r, s), 10 is (r, t), 11 is (s, t); a cross term vanishes iff its pair contains A.
    Base-flow constants (k_baseflow, nsk3_kernels.hpp; bits 12 + q): q < 3 is the convecting component along local axis q,
    sum_c met[q][c] U_c, which vanishes iff q == A (row A of the metrics has its only entry in column C, and U_C = 0);
    q = 3 + 3 c + x is d U_c / d x_x, which vanishes iff c == C (no spanwise component) or x == C (no spanwise variation)."""
    metric = {3 * a + c for a in range(3) for c in range(3) if (a == A) != (c == C)}
    gfac = {bit for bit, pair in ((9, (0, 1)), (10, (0, 2)), (11, (1, 2))) if A in pair}
    bf = {12 + A} | {12 + 3 + 3 * c + x for c in range(3) for x in range(3) if c == C or x == C}
    return metric | gfac | bf


class _Pool:
    """cases, oracles and contexts, built once per (lx1, orientation[, settings]) and closed at teardown"""

    def __init__(self):
        self._case, self._hip, self._oracle = {}, {}, {}

    def case(self, lx1, key):
        if (lx1, key) not in self._case:
            base = axes3d.inplane_case(n=lx1, nz=2, nx=2 if lx1 >= 10 else 3)
            self._case[lx1, key] = base if key == "base" else axes3d.transform_case(base, *ORIENT[key])
        return self._case[lx1, key]

    def oracle(self, lx1, key, solvers=False):
        if (lx1, key, solvers) not in self._oracle:
            from oracle.linns3d import LinNS3D
            c = self.case(lx1, key)
            self._oracle[lx1, key, solvers] = LinNS3D(x=c.x, y=c.y, z=c.z, gid=c.gid, nglob=c.nglob, mask=c.mask, ub=c.ub, spng=c.spng,
                                                      re=c.re, endtime=c.endtime, has_outflow=c.has_outflow, build_solvers=solvers)
        return self._oracle[lx1, key, solvers]

    def hip(self, lx1, key, kind="tol"):
        if (lx1, key, kind) not in self._hip:
            from nekstab_amd.capi import NekStabHip
            if key == "plane":
                c = axes3d.plane_case(self.case(lx1, "base"))
            else:
                c = self.case(lx1, key)
            h = NekStabHip(c, c.meta["vert"], c.meta["nvert"], **(TOL if kind == "tol" else PROD))
            self._hip[lx1, key, kind] = h
            if kind == "prod":
                h.set_option("proj_reset", 1)                  # every map from an empty pressure projection space: maps repeat
        return self._hip[lx1, key, kind]

    def close(self):
        for h in self._hip.values():
            h.close()
        self._hip = {}


@pytest.fixture(scope="module")
def pool():
    p = _Pool()
    yield p
    p.close()


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


def _bits(mask):
    return {b for b in range(24) if mask >> b & 1}


def _forms(lx1):
    """the eapply_pipe forms that are kernels of their own at this order (nsk.hip launch_schwarz3 / launch_divgs3: at lx1 = 10
    forms 2 and 3 run form 0's kernels and 4 is 5; at lx1 <= 8 form 5 is 4)"""
    return (0, 1, 5) if lx1 >= 10 else (0, 1, 2, 3, 4)


def _E_apply(o, p):
    """E p = D (B^-1 M) D^T p with the oracle's operators: the product LinNS3D._build_pressure_solver assembles into `_Emat`
    (test_solves_do_not_depend_on_the_labelling checks the two against each other), without its factorisation"""
    g = o.opgradt(p)
    return o.opdiv([o.binvm1 * o.mask * o.dssum(gc) for gc in g])


_ZERO_CASES = [(6, A, C) for A in range(3) for C in range(3)] + [(lx1, A, (A + 1) % 3) for lx1 in (8, 10) for A in range(3)]


@pytest.mark.parametrize("lx1,A,C", _ZERO_CASES, ids=["lx%d-A%dC%d" % t for t in _ZERO_CASES])
def test_zero_array_patterns(pool, lx1, A, C):
    """Every pattern of arrays that vanish on the whole mesh (see `expected_zero_bits` for the rule): the set-up finds exactly
    the set that (A, C) predicts; with those loads skipped every element operator equals the oracle of the transformed case --
    axhelm, the weak divergence, D^T, the three convection terms on the thread-per-node and the matrix-core kernels at 1e-12,
    E = D B^-1 D^T at 1e-11 --; and with every array loaded again (option zero_metrics = 0) the same operators, a Helmholtz
    solve and a pressure solve under every Schwarz / divergence kernel form of this order (eapply_pipe, with divgs_c3 riding along
    with form 1 as in test_3d_gpu.test_schwarz_kernel_forms_agree; `t_eapply` itself always runs k_gradt + k_divgs, so the
    other forms are reached through the solve) return the same bits.  The forms' solutions agree with form 0's at that test's 1e-7."""
    # the parametrisation as a whole: every bit both set and clear somewhere, and a metric pattern that is not its own transpose
    sets = [expected_zero_bits(a, c) for (_, a, c) in _ZERO_CASES]
    for b in range(24):
        assert any(b in s for s in sets) and any(b not in s for s in sets), b
    transpose = lambda s: {3 * (q % 3) + q // 3 for q in s if q < 9}
    assert any({q for q in s if q < 9} != transpose(s) for s in sets)
    assert expected_zero_bits(2, 2) == {2, 5, 6, 7} | {10, 11} | {12 + 2, 12 + 5, 12 + 8, 12 + 9, 12 + 10, 12 + 11}      # test_3d_gpu.py

    key = "A%dC%d" % (A, C)
    c, o, h = pool.case(lx1, key), pool.oracle(lx1, key), pool.hip(lx1, key)
    want = expected_zero_bits(A, C)
    got = _bits(h.stats()["zero_arrays"])
    print("lx1 %d, spanwise on local axis %d, coordinate %d: zero arrays %s" % (lx1, A, C, sorted(got)))
    assert got == want, (sorted(got), sorted(want))
    assert h.nsteps == o.nsteps and abs(h.dt - o.dt) < 1e-15

    rng = np.random.default_rng(1)
    m = lx1 - 2
    u = rng.standard_normal((3,) + c.x.shape)
    p = rng.standard_normal((c.nel, m, m, m))
    r = rng.standard_normal((3,) + c.x.shape)
    U, sp = o.ub, o.spng * o.bm1
    adj = o.convect_adj(u, U)
    conv = {0: np.stack([-(sp * u[k] + o.convect(u, U[k]) + o.convect(U, u[k])) for k in range(3)]),
            1: np.stack([-(sp * u[k] + adj[k] - o.convect(U, u[k])) for k in range(3)]),
            2: np.stack([-o.convect(u, u[k]) for k in range(3)])}
    ops = [("axhelm", lambda: h.t_axhelm(u[0], 0.7, 1.3), o.axhelm(u[0], 0.7, 1.3), 1e-12),
           ("opdiv", lambda: h.t_op3(1, u), o.opdiv(u), 1e-12),
           ("opgradt", lambda: h.t_op3(2, p), np.stack(o.opgradt(p)), 1e-12),
           ("eapply", lambda: h.t_eapply(p), _E_apply(o, p), 1e-11)]
    for mode in (0, 1, 2):
        ops.append(("convect mode %d" % mode, lambda mode=mode: h.t_op3(3, u, mode), conv[mode], 1e-12))
        if lx1 in (8, 10) and (mode < 2 or lx1 == 10):
            ops.append(("convect mode %d, matrix cores" % mode, lambda mode=mode: h.t_op3(8, u, mode), conv[mode], 1e-12))
    try:
        worst = 0.0
        for name, run, ref, tol in ops:
            h.set_option("zero_metrics", 1)
            assert _bits(h.stats()["zero_arrays"]) == want
            masked = run()
            err = _rel(masked, ref)
            worst = max(worst, err / tol)
            print("  %-32s error %.2e" % (name, err))
            assert err < tol, (name, err)
            h.set_option("zero_metrics", 0)
            assert h.stats()["zero_arrays"] == 0
            assert np.array_equal(run(), masked), name
        print("  largest operator error / tolerance: %.3f" % worst)
        # the solves: same bits with the loads skipped and with every array loaded
        sol = {}
        for form in _forms(lx1):
            h.set_option("eapply_pipe", form)
            h.set_option("divgs_c3", 1 if form == 1 else 0)
            out = {}
            for zm in (1, 0):
                h.set_option("zero_metrics", zm)
                out[zm] = (h.t_pres_solve(p), h.t_op3(5, r, 3)) if form == _forms(lx1)[0] else (h.t_pres_solve(p), None)
            (x1, it1), (x0, it0) = out[1][0], out[0][0]
            assert it1 == it0 and 0 < it1 <= 48 and np.array_equal(x1, x0), (form, it1, it0)
            if out[1][1] is not None:
                (y1, jt1), (y0, jt0) = out[1][1], out[0][1]
                assert jt1 == jt0 and 0 < jt1 < 200 and np.array_equal(y1, y0), (jt1, jt0)
            sol[form] = (x1, it1)
        print("  GMRES iterations by kernel form:", {f: s[1] for f, s in sol.items()})
        for form in _forms(lx1)[1:]:
            assert _rel(sol[form][0], sol[0][0]) < 1e-7, form
            assert abs(sol[form][1] - sol[0][1]) <= 1, {f: s[1] for f, s in sol.items()}
    finally:
        h.set_option("zero_metrics", 1)
        h.set_option("eapply_pipe", 4)
        h.set_option("divgs_c3", -1)


def _map(h, q, mode, nst=5):
    """`nst` steps of the linearised (mode 0 direct, 1 adjoint) or the full ('nl') equations from the state q"""
    v0, v1 = h.alloc(2)
    try:
        if h.ndim == 3:
            h.upload3(v0, *q)
        else:
            h.upload(v0, *q)
        h.set_nsteps(nst)
        if mode == "nl":
            h.nonlinear_map(v1, v0)
        else:
            h.matvec(v1, v0, mode)
        out = h.download3(v1) if h.ndim == 3 else h.download(v1)
        assert h.stats()["unconverged"] == 0
        return out
    finally:
        h.free([v0, v1])


@pytest.mark.parametrize("lx1", [6, 8])
def test_map_is_covariant_and_matches_the_quadrilateral_path(pool, lx1):
    """Five steps in four frames -- the original one, two asymmetric orientations with flipped axes, one oblique rotation (no
    zero array there: every load is made, the general path) -- with the solver settings of
    test_3d_gpu.test_extruded_cylinder_matches_2d, at its 1e-7 of the largest |u|.
    A z-invariant in-plane state (solenoidal: see below), direct and adjoint: the transformed context's map carried back equals
    the untransformed hexahedral context's, and equals the quadrilateral context's map plane by plane; the spanwise component
    stays below tolerance.
    A fully three-dimensional state, direct, adjoint and the full equations: transformed against untransformed."""
    keys = ("base", "A0C1-flip", "A1C0-flip", "oblique")
    c = pool.case(lx1, "base")
    hs = {k: pool.hip(lx1, k, "prod") for k in keys}
    h2 = pool.hip(lx1, "plane", "prod")
    zeros = {k: _bits(hs[k].stats()["zero_arrays"]) for k in keys}
    print("lx1 %d zero arrays:" % lx1, {k: sorted(v) for k, v in zeros.items()})
    assert zeros["base"] == expected_zero_bits(2, 2) and zeros["A0C1-flip"] == expected_zero_bits(0, 1)
    assert zeros["A1C0-flip"] == expected_zero_bits(1, 0) and zeros["oblique"] == set()
    nz, nel2, n, m = 2, c.nel // 2, lx1, lx1 - 2
    for k in keys:
        assert hs[k].nsteps == h2.nsteps and abs(hs[k].dt - h2.dt) < 1e-15, k
    # --- z-invariant in-plane state.  tol_pres = 1e-4 is relative to the pressure right-hand side, and the quadrilateral and the
    # hexahedral iteration differ within it (other preconditioners; the hexahedral Schwarz solves are not z-invariant, so the
    # iterates leave the z-invariant subspace that only the converged solution lies in).  1e-7 of |u| therefore presumes a state
    # whose pressure increment per step is below 1e-3 of |u|: a solenoidal state past its start-up, as the eigenmode of
    # test_extruded_cylinder_matches_2d is, not an arbitrary field.  So the smooth field is first advanced ten steps by the 2-D CPU
    # oracle (direct solves: discretely solenoidal, with its pressure, past the three start-up steps of the BDF / extrapolation
    # orders).  Measured against the quadrilateral map at lx1 = 6 / 8, direct: the raw field 3.2e-5 / 2.7e-5, two steps of the
    # oracle 1.3e-6 / 1.2e-6, ten steps 2.4e-8 / 1.4e-8 (spanwise component 3e-9 / 5e-9); the frames among themselves agree to
    # 1e-14 (2e-11 oblique) whatever the state.
    from oracle.linns import LinNS2D
    c2 = axes3d.plane_case(c)
    o2 = LinNS2D(x=c2.x, y=c2.y, gid=c2.gid, nglob=c2.nglob, mask=c2.mask, ub=c2.ub, spng=c2.spng, re=c2.re, endtime=c2.endtime,
                 has_outflow=c2.has_outflow)
    assert o2.nsteps == h2.nsteps and abs(o2.dt - h2.dt) < 1e-15
    u2, v2, p2 = o2.matvec((np.sin(1.3 * c2.x) * np.cos(2.0 * c2.y) * c2.mask, np.cos(0.7 * c2.x + 0.2) * np.sin(3.0 * c2.y) * c2.mask,
                            np.zeros((nel2, m, m))), nsteps=10)
    q3 = [mesh3d.extrude_field(u2, nz), mesh3d.extrude_field(v2, nz), np.zeros_like(c.x), mesh3d.extrude_pressure(p2, nz)]
    bad = []
    for mode in (0, 1):
        r2 = _map(h2, (u2, v2, p2), mode)
        sc = max(np.abs(r2[0]).max(), np.abs(r2[1]).max())
        back = {}
        for k in keys:
            local, Q = ORIENT[k]
            vt, pt = axes3d.to_frame(q3[:3], q3[3], local, Q)
            out = _map(hs[k], (vt[0], vt[1], vt[2], pt), mode)
            back[k] = axes3d.from_frame(out[:3], out[3], local, Q)
            vel = back[k][0]
            e2d = max(np.abs(vel[comp].reshape(nz, nel2, n, n, n) - r2[comp][None, :, None]).max() for comp in (0, 1)) / sc
            e3 = np.abs(vel[2]).max() / sc
            e3d = max(np.abs(vel[comp] - back["base"][0][comp]).max() for comp in range(3)) / sc
            print("lx1 %d mode %d %-10s: against the quadrilateral map %.2e, spanwise component %.2e, against the untransformed map %.2e"
                  % (lx1, mode, k, e2d, e3, e3d))
            if not (e2d < 1e-7 and e3 < 1e-7 and e3d < 1e-7):
                bad.append((k, mode, e2d, e3, e3d))
    assert not bad, bad
    # --- fully three-dimensional state
    x, y, z = c.x, c.y, c.z
    kz = 2.0 * np.pi / 0.8
    q = [np.sin(1.3 * x + kz * z) * np.cos(2.0 * y) * c.mask, np.cos(0.7 * x + 0.2) * np.sin(3.0 * y - kz * z) * c.mask,
         np.sin(x + y) * np.cos(kz * z) * c.mask, np.zeros((c.nel, m, m, m))]
    for mode in (0, 1, "nl"):
        ref = _map(hs["base"], q, mode)
        sc = max(np.abs(ref[comp]).max() for comp in range(3))
        assert np.abs(ref[2]).max() > 1e-2 * sc                      # genuinely three-dimensional
        for k in keys[1:]:
            local, Q = ORIENT[k]
            vt, pt = axes3d.to_frame(q[:3], q[3], local, Q)
            out = _map(hs[k], (vt[0], vt[1], vt[2], pt), mode)
            vel, _ = axes3d.from_frame(out[:3], out[3], local, Q)
            err = max(np.abs(vel[comp] - ref[comp]).max() for comp in range(3)) / sc
            print("lx1 %d mode %s %-10s: three-dimensional state against the untransformed map %.2e" % (lx1, mode, k, err))
            if not err < 1e-7:
                bad.append((k, mode, err))
    assert not bad, bad


@pytest.mark.parametrize("lx1", [6, 8, 10])
def test_solves_do_not_depend_on_the_labelling(pool, lx1):
    """A Helmholtz solve (`t_op3(5, r, 3)`) and a pressure solve (`t_pres_solve`) from the same right-hand sides carried into
    the original frame and three orientations, one per spanwise local axis, each with a flipped axis.  The solutions equal the
    oracle's direct solves (of the untransformed case, carried into the frame: tests/test_oracle3d.py holds the oracle covariant
    to 1e-12) at the 1e-9 and 1e-6 of tests/test_3d_gpu.py.  Jacobi-CG and the Schwarz, fast-diagonalisation and coarse
    preconditioner treat r, s and t alike, so in exact arithmetic the iterates are identical in every frame: the iteration counts
    may differ by one (a stopping test that rounding pushes across its threshold) and no more."""
    keys = ("base", "A0C2-flip", "A1C0-flip2", "A2C1-flip")
    c, o = pool.case(lx1, "base"), pool.oracle(lx1, "base", True)
    m = lx1 - 2
    rng = np.random.default_rng(3)
    r = rng.standard_normal((3,) + c.x.shape)
    g = rng.standard_normal((c.nel, m, m, m))
    h2 = (11.0 / 6.0) / o.dt
    uref = [o.helm_solve(r[k], o.nu, h2) for k in range(3)]
    pref = o.E_solve(g)
    assert _rel(_E_apply(o, g).ravel(), o._Emat @ g.ravel()) < 1e-13            # (the matrix-free E of test_zero_array_patterns)
    hit, pit = {}, {}
    for k in keys:
        local, Q = ORIENT[k]
        h = pool.hip(lx1, k)
        rt, gt = axes3d.to_frame(r, g, local, Q)
        ut, pt = axes3d.to_frame(uref, pref, local, Q)
        out, hit[k] = h.t_op3(5, np.stack(rt), 3)
        eh = _rel(out, np.stack(ut))
        xs, pit[k] = h.t_pres_solve(gt)
        ep = _rel(xs, pt)
        print("lx1 %d %-10s: Helmholtz %d iterations, error %.2e; pressure %d iterations, error %.2e" % (lx1, k, hit[k], eh, pit[k], ep))
        assert eh < 1e-9 and ep < 1e-6, (k, eh, ep)
        assert 0 < hit[k] < 200 and 0 < pit[k] <= 48
    print("lx1 %d iteration counts: Helmholtz %s, pressure %s" % (lx1, hit, pit))
    assert max(hit.values()) - min(hit.values()) <= 1, hit
    assert max(pit.values()) - min(pit.values()) <= 1, pit
