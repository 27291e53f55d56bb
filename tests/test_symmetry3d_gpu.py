"""Symmetry boundaries on hexahedra on the device (nsk_init_masks with ndim = 3: k_helm, k_helm_p, k_divgs, k_divgs_c3 and
k_vel_update_proj of namespace k3 in their <.., CM = true> forms, k_helm_first_cm).  The reference is the project's own full-domain path, by
mirror symmetry (tests/sym_box3d.py): the 60-element channel is mirror-symmetric about y = 0 and about z = 0, base flow and
state have the parities of the subspace symmetric about both planes, and the y-half, the z-half and the quarter domain with
'SYM' on the cut planes are Galerkin restrictions to that subspace -- they differ from the full domain by solver tolerance and
rounding only.  One full-domain map per (lx1, kind) serves the three of them; the x-half has the transposed channel's.

BOUNDS: not chosen, measured on the full-domain context alone (code that the component masks do not touch), at the tolerances
TIGHT of tests/test_symmetry_gpu.py: its own symmetry defect |f - mirror(f)| / |f| about each of the two planes and the change of
f when both tolerances are tightened tenfold; the bound of a case is ten times the largest of the three (half and full run
different iteration histories), for the velocity (bm1 norm) and for the pressure (l2 over the Gauss nodes, means removed where
there is no outflow) separately.  `python -m tests.test_symmetry3d_gpu` prints the tables the constants below were copied from."""
from dataclasses import replace

import numpy as np
import pytest

from tests import sym_box, sym_box3d
from tests.test_symmetry_gpu import SOLVER_OPTIONS, TIGHT

pytestmark = pytest.mark.gpu

NSTEPS = 5
# (lx1, kind of map, sub-domain)
CASES = [(6, "direct", "quarter"), (8, "direct", "quarter"), (10, "direct", "quarter"),
         (6, "adjoint", "quarter"), (8, "adjoint", "quarter"), (10, "adjoint", "quarter"),
         (8, "direct", "yhalf"), (8, "direct", "zhalf"), (8, "direct", "xhalf"),
         (8, "nonlinear", "quarter"), (8, "newton", "quarter")]

# full-domain map (lx1, kind, transposed): (velocity, pressure) of its symmetry defect about the in-plane symmetry plane, about
# z = 0, and of its change under tenfold tighter tolerances -- measured on an MI355X with `python -m tests.test_symmetry3d_gpu`
MEASURED = {
    (6, 'adjoint', False): ((3.35e-14, 1.28e-13), (3.08e-14, 1.15e-13), (6.78e-13, 5.68e-11)),      # quarter 9.36e-13 / 1.03e-10
    (6, 'direct', False): ((2.92e-14, 7.45e-14), (2.66e-14, 6.24e-14), (5.36e-13, 9.53e-11)),      # quarter 7.73e-13 / 1.12e-10
    (8, 'adjoint', False): ((5.18e-14, 2.58e-13), (4.33e-14, 2.15e-13), (5.56e-13, 1.73e-10)),      # quarter 7.97e-13 / 2.24e-10
    (8, 'direct', False): ((4.97e-14, 2.26e-13), (4.60e-14, 2.22e-13), (5.24e-13, 1.92e-10)),      # quarter 7.91e-13 / 2.78e-10; yhalf 7.04e-13 / 2.11e-10; zhalf 6.56e-13 / 1.85e-10
    (8, 'direct', True): ((6.16e-14, 1.56e-13), (5.77e-14, 1.38e-13), (6.40e-13, 8.19e-11)),      # xhalf 8.50e-13 / 1.02e-10
    (8, 'newton', False): ((2.11e-14, 2.26e-13), (1.96e-14, 2.22e-13), (2.23e-13, 1.92e-10)),      # quarter 3.36e-13 / 2.78e-10
    (8, 'nonlinear', False): ((5.09e-14, 4.60e-13), (4.83e-14, 4.16e-13), (4.37e-13, 1.36e-10)),      # quarter 6.47e-13 / 4.23e-10
    (10, 'adjoint', False): ((7.35e-14, 5.34e-13), (6.04e-14, 4.40e-13), (6.09e-13, 4.03e-10)),      # quarter 8.31e-13 / 3.68e-10
    (10, 'direct', False): ((7.26e-14, 5.47e-13), (6.50e-14, 4.81e-13), (5.01e-13, 2.46e-10)),      # quarter 7.63e-13 / 3.32e-10
}
# the same run, (8, direct) quarter: walls in place of 'SYM' 2.9e-01 / 1.2e+00, the code of y = 0 left out 1.8e+00 / 8.6e-01
# (1000 bounds: 5.2e-09 / 1.9e-06)
# 2-D half channel against its periodic extrusion: the same comparison for the FULL channel (shared mask on both sides, no code
# of the component masks), lx1 -> (velocity incl. w, pressure); the bound of the half channel is ten times that
MEASURED_2D = {
    6: (9.93e-13, 2.77e-10),   # half channel: 1.05e-12, 1.61e-10
    8: (9.66e-13, 2.02e-10),   # half channel: 1.10e-12, 1.97e-10
}


def _fkey(key):
    lx1, kind, dom = key
    return lx1, kind, dom == "xhalf"


def bound(fkey):
    m = MEASURED[fkey]
    return 10.0 * max(x[0] for x in m), 10.0 * max(x[1] for x in m)


def _ctx(case, tighten=1.0, options=None, **over):
    from nekstab_amd.capi import NekStabHip
    kw = dict(TIGHT)
    kw["tol_helm"] *= tighten
    kw["tol_pres"] *= tighten
    kw.update(over)
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **kw)
    for k, v in (SOLVER_OPTIONS if options is None else options):
        h.set_option(k, v)
    return h


def _map(h, q, kind, nsteps=NSTEPS):
    h.set_nsteps(nsteps)
    a, b = h.alloc(2)
    h.upload3(a, *q)
    if kind == "nonlinear":
        h.nonlinear_map(b, a)
    else:
        h.matvec(b, a, {"direct": 0, "adjoint": 1, "newton": 3}[kind])
    f = h.download3(b)
    assert h.stats()["unconverged"] == 0
    h.free([a, b])
    return f


def _rel(a, b, w, nullspace=False):
    """(velocity in the bm1 norm, pressure in l2): |a - b| / |b|; nullspace: both pressures without their means"""
    v = np.sqrt(sum(np.sum(w * (x - y) ** 2) for x, y in zip(a[:3], b[:3])) / sum(np.sum(w * y ** 2) for y in b[:3]))
    pa, pb = (a[3] - a[3].mean(), b[3] - b[3].mean()) if nullspace else (a[3], b[3])
    return float(v), float(np.sqrt(np.sum((pa - pb) ** 2) / np.sum(pb ** 2)))


_FULL = {}


def _full_case(fkey):
    lx1, kind, tr = fkey
    return sym_box3d.case(lx1, "full", adjoint=(kind == "adjoint"), transpose=tr)


def _full_map(fkey):
    """the full-domain map at the tight tolerances, computed once and left unchanged: (fields, dt)"""
    if fkey not in _FULL:
        full, qf = _full_case(fkey)
        h = _ctx(full)
        _FULL[fkey] = (_map(h, qf, fkey[1]), h.dt)
        h.close()
    return _FULL[fkey]


def _sub_vs_full(key, code="SYM"):
    lx1, kind, dom = key
    ff, dt = _full_map(_fkey(key))
    sub, qs = sym_box3d.case(lx1, dom, code, adjoint=(kind == "adjoint"))
    h = _ctx(sub)
    assert h.dt == dt                                   # the same time step on both domains
    fs = _map(h, qs, kind)
    h.close()
    el = sym_box3d.elements(dom)
    return _rel(fs, [f[el] for f in ff], sym_box3d.bm1(sub), not sub.has_outflow), fs, sub


def measure(fkey):
    """the full-domain map: symmetry defect about both planes and change under tenfold tighter tolerances, (velocity, pressure) each"""
    lx1, kind, tr = fkey
    full, qf = _full_case(fkey)
    ff, _ = _full_map(fkey)
    w = sym_box3d.bm1(full)
    ns = not full.has_outflow
    iy = 0 if tr else 1                                 # the component normal to the in-plane symmetry plane
    sy = [1.0, 1.0, 1.0, 1.0]; sy[iy] = -1.0
    dy = _rel([sym_box3d.mirror(f, "y", s, tr) for f, s in zip(ff, sy)], ff, w, ns)
    dz = _rel([sym_box3d.mirror(f, "z", s, tr) for f, s in zip(ff, (1.0, 1.0, -1.0, 1.0))], ff, w, ns)
    h = _ctx(full, tighten=0.1)
    ft = _map(h, qf, kind)
    h.close()
    return dy, dz, _rel(ff, ft, w, ns)


@pytest.mark.parametrize("key", CASES, ids=lambda k: "%d-%s-%s" % k)
def test_sub_domain_equals_full(key):
    """Quarter against full at lx1 = 6, 8, 10, direct and adjoint; y-half, z-half and x-half at lx1 = 8; the nonlinear and the
    Newton-mode map on the quarter at lx1 = 8."""
    (ev, ep), _, _ = _sub_vs_full(key)
    bv, bp = bound(_fkey(key))
    print("sub-domain vs full", key, "velocity %.3e (bound %.3e)  pressure %.3e (bound %.3e)" % (ev, bv, ep, bp))
    assert ev <= bv and ep <= bp


@pytest.mark.parametrize("code", ["W", ""])
def test_the_comparison_has_teeth(code):
    """The quarter with walls in place of 'SYM', and with the code of the side y = 0 left out (a stress-free open boundary), is at
    least 1000 bounds away from the full-domain result."""
    key = (8, "direct", "quarter")
    (ev, ep), _, _ = _sub_vs_full(key, code)
    bv, bp = bound(_fkey(key))
    print("code %r: velocity %.3e pressure %.3e, 1000 x bound %.3e / %.3e" % (code, ev, ep, 1e3 * bv, 1e3 * bp))
    assert ev >= 1e3 * bv and ep >= 1e3 * bp


def test_invariants_on_the_symmetry_planes_and_the_seed():
    from nekstab_amd import seed
    _, fq, quarter = _sub_vs_full((8, "direct", "quarter"))
    for plane, normal in ((np.isclose(quarter.y, 0.0, atol=1e-13), 1), (quarter.z == 0.0, 2)):
        assert plane.sum() > 0 and np.all(fq[normal][plane] == 0.0)
        for k in range(3):
            if k != normal:
                assert np.abs(fq[k][plane]).max() > 1e-3 * np.abs(fq[k]).max()
    h = _ctx(quarter)
    v, = h.alloc(1)
    h.seed_noise(v)
    d = h.download3(v)
    h.close()
    q = seed.add_noise(quarter)
    assert all(np.array_equal(d[k], q[k]) for k in range(3)) and not d[3].any() and np.abs(d[0]).max() > 0


def _ubf(x, y, z):
    return np.stack([np.sin(np.pi * y) * np.cos(z), 0.3 * np.cos(x) * np.sin(np.pi * z), 0.2 * np.sin(x + y)])


def test_equal_component_masks_give_the_bits_of_nsk_init():
    """three copies of the shared mask through nsk_init_masks: the context of nsk_init, the same kernels, the same bits"""
    from nekstab_amd import mesh3d, seed
    c = mesh3d.box_case_3d(2, 2, 2, 6, re=40.0, endtime=0.05, ub_func=_ubf, warp=0.05)
    q = seed.add_noise(c) + (np.zeros((c.nel, 4, 4, 4)),)
    out = []
    for case in (c, replace(c, cmask=np.stack([c.mask, c.mask, c.mask]))):
        h = _ctx(case, options=[], tol_helm=1e-11, tol_pres=1e-6)
        out.append(_map(h, q, "direct", 3))
        h.close()
    assert np.abs(out[0][0]).max() > 0 and all(np.array_equal(a, b) for a, b in zip(*out))


@pytest.mark.parametrize("lx1", [8, 10])
def test_divergence_kernel_forms_agree(lx1):
    """k_divgs<N, true> (divgs_c3 = 0) against k_divgs_c3<N, true> (1) on the quarter: the same arithmetic up to the order of the
    sums inside the matrix-core passes -- the tolerances of tests/test_3d_gpu.py::test_schwarz_kernel_forms_agree."""
    quarter, q = sym_box3d.case(lx1, "quarter")
    rng = np.random.default_rng(5)
    g = rng.standard_normal((quarter.nel,) + (lx1 - 2,) * 3)
    sol, its, maps = {}, {}, {}
    for form in (0, 1):
        h = _ctx(quarter, options=[], tol_helm=1e-12, tol_pres=1e-8, max_pres_iter=96)
        try:
            h.set_option("divgs_c3", form)
            sol[form], its[form] = h.t_pres_solve(g)
            maps[form] = _map(h, q, "adjoint")
        finally:
            h.close()
    sc = max(np.abs(maps[0][k]).max() for k in range(3))
    assert np.abs(sol[1] - sol[0]).max() / np.abs(sol[0]).max() < 1e-7 and abs(its[1] - its[0]) <= 1
    for k in range(3):
        assert np.abs(maps[1][k] - maps[0][k]).max() < 1e-9 * sc


def test_resident_velocity_iteration_is_bit_identical_lx1_10():
    """k_helm_p<10, true> (helm_pf = 1, the default at lx1 = 10) with eight resident workgroups -- 15 elements: uneven walks --
    against one workgroup per element, k_helm<10, true> (helm_pf = 0): the same arithmetic in the same order, a five-step direct
    map and the iteration counts are equal bit for bit, as test_resident_helmholtz_iteration_is_bit_identical_lx1_10 asserts for
    the shared mask."""
    quarter, q = sym_box3d.case(10, "quarter")
    out, its = [], []
    for pf in (1, 0):
        h = _ctx(quarter, options=[], tol_helm=1e-12, tol_pres=1e-8)
        try:
            h.set_option("helm_pf", pf)
            if pf:
                h.set_option("helm_pf_grid", 8)
            out.append(_map(h, q, "direct"))
            st = h.stats()
            its.append((st["total_helm_iters"], st["total_pres_iters"], h.step_iters()))
        finally:
            h.close()
    assert np.abs(out[0][0]).max() > 0 and its[0][0] > 0
    assert all(np.array_equal(a, b) for a, b in zip(*out))
    assert its[0][:2] == its[1][:2] and all(np.array_equal(a, b) for a, b in zip(its[0][2], its[1][2]))


def test_refusals():
    """What has no component-mask form on hexahedra says so."""
    import ctypes as C
    from nekstab_amd.capi import NskError
    quarter, q = sym_box3d.case(10, "quarter")
    h = _ctx(quarter)
    try:
        for name, val in [("helm_fdm", 1), ("eapply_pipe", 3)]:
            with pytest.raises(NskError) as e:
                h.set_option(name, val)
            assert e.value.code == -1 and "nsk_init_masks" in str(e.value)
        h.set_option("eapply_pipe", 4)
        part = (C.c_int * quarter.nel)(*([0] * 8 + [1] * 7))
        out = C.c_void_p()
        assert h.lib.nsk_shard_create(h.ctx, part, 0, 2, C.byref(out)) == -1 and b"nsk_init_masks" in h.lib.nsk_last_error()
        with pytest.raises(NskError) as e:
            h.bench_kernel("helm", 2)
        assert e.value.code == -1 and "nsk_init_masks" in str(e.value)
        assert np.abs(_map(h, q, "direct", 2)[2]).max() > 0            # the context still works
    finally:
        h.close()
    bad = replace(quarter, cmask=np.stack([quarter.cmask[0], quarter.cmask[1], 0.5 * quarter.cmask[2]]))
    with pytest.raises(NskError) as e:
        _ctx(bad)
    assert e.value.code == -1 and "0.0 and 1.0" in str(e.value)


def _planes(lx1, half):
    """the 2-D channel (half: 'SYM' on y = 0, the merged component-mask path of quadrilaterals) against its periodic extrusion
    with a z-invariant state and w = 0, plane by plane: (velocity incl. w relative to |(u, v)|, pressure), max over the planes"""
    from nekstab_amd import mesh3d
    from tests.test_symmetry_gpu import _bm1, _map as _map2
    c2, q2 = sym_box.case(lx1, half)
    h = _ctx(c2)
    f2 = _map2(h, q2, "direct", NSTEPS)
    dt = h.dt
    h.close()
    c3 = mesh3d.extrude_case(c2, 2, 1.0)
    h = _ctx(c3)
    assert abs(h.dt - dt) <= 1e-14 * dt
    f3 = _map(h, (mesh3d.extrude_field(q2[0], 2), mesh3d.extrude_field(q2[1], 2), np.zeros(c3.x.shape), mesh3d.extrude_pressure(q2[2], 2)), "direct")
    h.close()
    w, n, nel2 = _bm1(c2), lx1, c2.nel
    nv = sum(np.sum(w * y ** 2) for y in f2[:2])
    ev = ep = 0.0
    for kz in range(2):
        sl = slice(kz * nel2, (kz + 1) * nel2)
        for k in range(n):
            dv = sum(np.sum(w * (f3[c][sl, k] - f2[c]) ** 2) for c in range(2)) + np.sum(w * f3[2][sl, k] ** 2)
            ev = max(ev, float(np.sqrt(dv / nv)))
        for k in range(n - 2):
            ep = max(ep, float(np.sqrt(np.sum((f3[3][sl, k] - f2[2]) ** 2) / np.sum(f2[2] ** 2))))
    return ev, ep


@pytest.mark.parametrize("lx1", [6, 8])
def test_extruded_half_channel_equals_the_quadrilateral_path(lx1):
    ev, ep = _planes(lx1, True)
    bv, bp = (10.0 * x for x in MEASURED_2D[lx1])
    print("2-D half channel vs periodic extrusion, lx1 = %d: velocity %.3e (bound %.3e) pressure %.3e (bound %.3e)" % (lx1, ev, bv, ep, bp))
    assert ev <= bv and ep <= bp


if __name__ == "__main__":      # the tables behind MEASURED and MEASURED_2D, and every figure the tests assert on
    for fkey in sorted({_fkey(k) for k in CASES}):
        m = measure(fkey)
        print("    %r: (%s)," % (fkey, ", ".join("(%.2e, %.2e)" % x for x in m)), flush=True)
    for key in CASES:
        try:
            (ev, ep), _, _ = _sub_vs_full(key)
            print("# sub-domain vs full %r: %.2e, %.2e" % (key, ev, ep), flush=True)
        except AssertionError as err:       # (a time step or a convergence count that differs is a finding of its own: the table goes on)
            print("# sub-domain vs full %r: assertion failed: %r" % (key, err), flush=True)
    for code in ("W", ""):
        (ev, ep), _, _ = _sub_vs_full((8, "direct", "quarter"), code)
        print("# teeth, code %r: %.3e %.3e" % (code, ev, ep), flush=True)
    for lx1 in (6, 8):
        print("    %d: (%.2e, %.2e),   # half channel: %s" % ((lx1,) + _planes(lx1, False) + ("%.2e, %.2e" % _planes(lx1, True),)), flush=True)
