"""Quadrilateral kernels on irregular topology: fans of k elements around one vertex with a second ring (tests/fan_mesh.py;
centre of valence k = 3, 5, 6, 8, ring-0 corners of valence 3) against the oracle.  Valence 5 takes the CSR walk of the gather
inside the two-launch pressure iteration, valence 6 and 8 switch the context to the three-launch form, valence 8 fills the
vertex table (CVT), valence 9 is refused.  Bounds: the operators' of tests/test_kernels_other_orders_gpu.py::test_operators, the
solves' and maps' of tests/test_3d_gpu.py::test_steps_match_oracle at the same settings (tests/test_irregular_host.py: a gather
that drops one copy at the centre is 1000 bounds away)."""
import numpy as np
import pytest

from tests import fan_mesh

pytestmark = pytest.mark.gpu

TOL = dict(tol_helm=1e-12, tol_pres=1e-8, tol_relative=1, max_helm_iter=200, max_pres_iter=48)
NSTEPS = 5
OPERATOR_CASES = [(5, 6), (5, 8), (5, 10), (5, 12), (8, 6), (8, 8), (8, 10), (8, 12), (3, 8), (6, 8)]
SOLVE_CASES = [(5, 6), (5, 8), (8, 6), (8, 8), (5, 10), (5, 12)]

_SETUP, _REF = {}, {}


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# The pressure iteration of these contexts: the merged iteration as it is by default (two launches per iteration where every
# vertex has at most five elements, three otherwise) for the first 24 iterations of a solve, and a second Gram-Schmidt pass in
# every classic iteration after them.  With the default single pass (gs2_from = 48) a solve to 1e-8 on a mesh of 15 - 24 elements
# reports convergence with a true residual of 0.07 - 3 |g| (measured; also on the regular 30-element channel of tests/sym_box.py,
# so this is no matter of topology): the norm of a new basis vector is taken as sqrt(|w|^2 - sum h_k^2) from one pass of dots
# (k_gmres_update, uc_rotate), the basis loses its orthogonality once that difference cancels, and the Givens residual then
# underestimates the true one.  DESIGN.md section 3 records this limit of tiny meshes at tolerances far below production's;
# tests/test_symmetry_gpu.py avoids it in the same way.
SOLVER_OPTIONS = (("gs2_from", 0),)


def _hip(c, **kw):
    from nekstab_amd.capi import NekStabHip
    a = dict(TOL); a.update(kw)
    h = NekStabHip(c, c.meta["vert"], c.meta["nvert"], **a)
    for name, val in SOLVER_OPTIONS:
        h.set_option(name, val)
    return h


def _setup(k, lx1):
    """(case, oracle, context) on fan(k, 2), made once; the oracle has its factorisations where a solve needs them"""
    if (k, lx1) not in _SETUP:
        from tests.conftest import make_oracle
        c = fan_mesh.case2(k, 2, lx1)
        _SETUP[k, lx1] = (c, make_oracle(c, build_solvers=(k, lx1) in SOLVE_CASES), _hip(c))
    return _SETUP[k, lx1]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for _, _, h in _SETUP.values():
        h.close()
    _SETUP.clear(); _REF.clear()


def _state(c):
    m = c.lx1 - 2
    return (np.sin(1.3 * c.x + 0.2) * np.cos(0.9 * c.y) * c.mask, np.cos(0.7 * c.x) * np.sin(1.1 * c.y + 0.3) * c.mask, np.zeros((c.nel, m, m)))


def _reference_map(k, lx1, mode):
    """the oracle's five steps of `_state`, computed once per case and direction"""
    if (k, lx1, mode) not in _REF:
        c, o, _ = _setup(k, lx1)
        _REF[k, lx1, mode] = o.matvec(_state(c), adjoint=bool(mode), nsteps=NSTEPS)
    return _REF[k, lx1, mode]


def _map_errors(h, c, ref, mode):
    """(velocity error / velocity scale, relative pressure error) of the context's five-step map against `ref`"""
    a, b = h.alloc(2)
    h.upload(a, *_state(c))
    keep = h.nsteps
    h.set_nsteps(NSTEPS)
    h.matvec(b, a, mode)
    h.set_nsteps(keep)
    out = h.download(b)
    st = h.stats()
    h.free([a, b])
    sc = max(np.abs(ref[0]).max(), np.abs(ref[1]).max())
    return max(np.abs(out[0] - ref[0]).max(), np.abs(out[1] - ref[1]).max()) / sc, rel(out[2], ref[2]), st


@pytest.mark.parametrize("k,lx1", OPERATOR_CASES)
def test_operators(k, lx1):
    c, o, h = _setup(k, lx1)
    assert (h.nsteps, abs(h.dt - o.dt) < 1e-15) == (o.nsteps, True)
    rng = np.random.default_rng(100 * k + lx1)
    u, v = rng.standard_normal(c.x.shape), rng.standard_normal(c.x.shape)
    p = rng.standard_normal((c.nel, lx1 - 2, lx1 - 2))
    err = {}
    err["axhelm"] = rel(h.t_axhelm(u, 0.02, 300.0), o.axhelm(u, 0.02, 300.0))
    err["dssum"] = rel(h.t_dssum(u), o.dssum(u))
    err["opdiv"] = rel(h.t_opdiv(u, v), o.opdiv(u, v))
    gx, gy = h.t_opgradt(p); ox, oy = o.opgradt(p)
    err["opgradt"] = max(rel(gx, ox), rel(gy, oy))
    U, V = o.ub
    bx = -o.spng * u * o.bm1 - (o.convect(u, v, U) + o.convect(U, V, u))
    by = -o.spng * v * o.bm1 - (o.convect(u, v, V) + o.convect(U, V, v))
    cx, cy = h.t_convect(u, v, False)
    err["convect"] = max(rel(cx, bx), rel(cy, by))
    ax, ay = o.convect_adj(u, v, U, V)
    bx = -o.spng * u * o.bm1 - ax + o.convect(U, V, u)
    by = -o.spng * v * o.bm1 - ay + o.convect(U, V, v)
    cx, cy = h.t_convect(u, v, True)
    err["convect_adj"] = max(rel(cx, bx), rel(cy, by))
    wx, wy = o.opgradt(p)
    fac = o.binvm1 * o.mask
    err["eapply"] = rel(h.t_eapply(p), o.opdiv(fac * o.dssum(wx * o.mask), fac * o.dssum(wy * o.mask)))
    print("fan(%d, 2) lx1 %d:" % (k, lx1), " ".join("%s %.2e" % kv for kv in err.items()))
    for name, e in err.items():
        assert e < (1e-13 if name == "dssum" else 1e-12), (name, e)


@pytest.mark.parametrize("k,lx1", SOLVE_CASES)
def test_solves(k, lx1):
    c, o, h = _setup(k, lx1)
    rng = np.random.default_rng(7 * k + lx1)
    rx, ry = rng.standard_normal(c.x.shape) * o.bm1, rng.standard_normal(c.x.shape) * o.bm1
    h1, h2 = o.nu, (11.0 / 6.0) / o.dt
    ox, oy, it = h.t_helm_solve(rx, ry, 3)
    ex, ey = o.helm_solve(rx, h1, h2), o.helm_solve(ry, h1, h2)
    sc = max(np.abs(ex).max(), np.abs(ey).max())
    ev = max(np.abs(ox - ex).max(), np.abs(oy - ey).max()) / sc
    g = rng.standard_normal((c.nel, lx1 - 2, lx1 - 2))
    x, itp = h.t_pres_solve(g)
    ep = rel(x, o.E_solve(g))
    print("fan(%d, 2) lx1 %d: velocity solve %.2e (%d iterations), pressure solve %.2e (%d iterations), unconverged %d"
          % (k, lx1, ev, it, ep, itp, h.stats()["unconverged"]))
    assert 0 < it < 200 and 0 < itp <= 48
    assert ev < 1e-7 and ep < 1e-4


@pytest.mark.parametrize("mode", [0, 1], ids=["direct", "adjoint"])
@pytest.mark.parametrize("k,lx1", SOLVE_CASES)
def test_steps_match_oracle(k, lx1, mode):
    c, o, h = _setup(k, lx1)
    ev, ep, st = _map_errors(h, c, _reference_map(k, lx1, mode), mode)
    print("fan(%d, 2) lx1 %d mode %d: velocity %.2e, pressure %.2e, iterations %d / %d" % (k, lx1, mode, ev, ep, st["helm_iters"], st["pres_iters"]))
    assert st["unconverged"] == 0
    assert ev < 1e-7 and ep < 1e-4


FORMS = [[], [("fuse2", 0)], [("helm_pack", 0)], [("conv_fuse", 0)], [("tail", 1), ("tail_off_h", -3), ("tail_off_p", -1)], [("tail", 0)], [("use_graph", 0)]]


@pytest.mark.parametrize("options", FORMS, ids=lambda o: "-".join("%s=%s" % kv for kv in o) or "default")
def test_launch_forms_against_the_oracle(options):
    """fan(8, 2) at lx1 = 8 with a projection space (nproj = 8, what the deferred projection update needs): every launch-form
    option the suite toggles on the cylinder.  The same map twice -- the second with the launch budgets the first has left and the
    projection space it has filled -- each against the oracle"""
    c, o, _ = _setup(8, 8)
    h = _hip(c, nproj=8)
    try:
        for name, val in options:
            h.set_option(name, val)
        ev, ep = 0.0, 0.0
        for rep in range(2):
            e1, e2, st = _map_errors(h, c, _reference_map(8, 8, 0), 0)
            assert st["unconverged"] == 0, rep
            ev, ep = max(ev, e1), max(ep, e2)
    finally:
        h.close()
    # absorb_maps counts the maps whose solves started inside the two-launch iteration (tests/test_step_form_gpu.py)
    print("options %s: pressure iteration in %s launches; convfuse_steps %d helmpack_steps %d tail_maps %d; velocity %.2e pressure %.2e"
          % (options, "two" if st["absorb_maps"] > 0 else "three (or two without the deferred update)", st["convfuse_steps"], st["helmpack_steps"],
             st["tail_maps"], ev, ep))
    assert st["unconverged"] == 0
    assert ev < 1e-7 and ep < 1e-4


def test_valence_nine_is_refused_and_the_library_goes_on():
    from nekstab_amd.capi import NskError, load_library
    c9 = fan_mesh.case2(9, 1, 6)
    with pytest.raises(NskError) as e:
        _hip(c9)
    assert e.value.code == -1 and "vertex valence outside 1..8" in str(e.value)
    assert b"vertex valence outside 1..8" in load_library().nsk_last_error()
    c, o, _ = _setup(5, 6)
    h = _hip(c)
    try:
        u = np.random.default_rng(0).standard_normal(c.x.shape)
        assert rel(h.t_dssum(u), o.dssum(u)) < 1e-13
    finally:
        h.close()


@pytest.mark.parametrize("k", [24, 128])
def test_basis_gemm_tail_rows(k):
    """nsk_basis_gemm on fan(5, 1) at lx1 = 6: the state length 2 * 5 * 36 + 5 * 16 = 440 is no multiple of 16 (the row tail of the
    matrix-core kernel), k = 24 and 128 are its column tiles of 2 and 8 (128: the benchmark's Krylov dimension).  Every column
    against a long-double sum."""
    c = fan_mesh.case2(5, 1, 6)
    h = _hip(c)
    try:
        assert h.nstate == 440 and h.nstate % 16 != 0
        rng = np.random.default_rng(k)
        vs = [(rng.standard_normal(c.x.shape), rng.standard_normal(c.x.shape), rng.standard_normal((c.nel, 4, 4))) for _ in range(k)]
        dv = h.alloc(k)
        for d, v in zip(dv, vs):
            h.upload(d, *v)
        Z = rng.standard_normal((k, k))
        h.basis_gemm(dv, Z)
        V = np.stack([np.concatenate([a.ravel() for a in v]) for v in vs]).astype(np.longdouble)      # (k, 440)
        ref = np.zeros((k, V.shape[1]), dtype=np.longdouble)
        for q in range(k):
            ref += Z[q, :, None].astype(np.longdouble) * V[q][None, :]
        worst = 0.0
        for j in range(k):
            got = np.concatenate([a.ravel() for a in h.download(dv[j])])
            worst = max(worst, float(np.abs(got - ref[j]).max()))
        print("basis_gemm k = %d on 440 rows: worst |difference| %.2e (bound %.2e)" % (k, worst, 1e-11 * np.sqrt(k)))
        assert worst < 1e-11 * np.sqrt(k)
        h.free(dv)
    finally:
        h.close()
