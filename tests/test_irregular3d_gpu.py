"""Hexahedral kernels on irregular topology: the fan of k quadrilaterals extruded in z (tests/fan_mesh.py) against the 3-D oracle.
On the fan's axis the gather takes every branch that a box never takes: element corners with 5, 6 and 8 copies (corner lists
partly and exactly full), corners with 10, 12 and 16 copies (beyond their list: the CSR walk), and edge nodes -- no corners --
with 5, 6 and 8 copies (the wide CSR forms).  tests/test_irregular_host.py asserts that census and that a gather which drops one
copy there is 1000 bounds away.  Bounds: those of tests/test_3d_gpu.py (operators 1e-12 / 1e-13 / 1e-11, Helmholtz solve 1e-9,
pressure solve 1e-6, five-step maps 1e-7 of the velocity scale and 1e-4 of the pressure) and of tests/test_sharded_gpu.py."""
from dataclasses import replace

import numpy as np
import pytest

from tests import fan_mesh

pytestmark = pytest.mark.gpu

TOL = dict(tol_helm=1e-12, tol_pres=1e-8, tol_relative=1, max_helm_iter=200, max_pres_iter=48)
NSTEPS = 5
# name -> (k, layers, periodic)
FIXTURES = {"k5x2-walls": (5, 2, False), "k8x2-periodic": (8, 2, True), "k8x1": (8, 1, False), "k6x1": (6, 1, False), "k5x1": (5, 1, False)}
OPERATOR_CASES = [(f, n) for f in ("k5x2-walls", "k8x2-periodic", "k8x1") for n in (6, 8, 10)]
STEP_CASES = [("k5x2-walls", 6), ("k5x2-walls", 8), ("k8x2-periodic", 6), ("k6x1", 8), ("k5x1", 10)]

_CASE, _ORACLE, _CTX, _REF = {}, {}, {}, {}


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()


def _case(name, lx1):
    if (name, lx1) not in _CASE:
        k, nz, per = FIXTURES[name]
        _CASE[name, lx1] = fan_mesh.fan3(k, nz, lx1, per)
    return _CASE[name, lx1]


def _oracle(name, lx1, solvers=False):
    """the 3-D oracle of a fixture, made once; with its pressure factorisation only where asked for"""
    from oracle.linns3d import LinNS3D
    key = (name, lx1)
    if key not in _ORACLE:
        c = _case(name, lx1)
        _ORACLE[key] = LinNS3D(x=c.x, y=c.y, z=c.z, gid=c.gid, nglob=c.nglob, mask=c.mask, ub=c.ub, spng=c.spng, re=c.re,
                               endtime=c.endtime, has_outflow=c.has_outflow, build_solvers=False)
    if solvers and _ORACLE[key]._E is None:
        _ORACLE[key]._build_pressure_solver()
    return _ORACLE[key]


def _hip(c, **kw):
    from nekstab_amd.capi import NekStabHip
    a = dict(TOL); a.update(kw)
    return NekStabHip(c, c.meta["vert"], c.meta["nvert"], **a)


def _ctx(name, lx1):
    """the default context of a fixture, shared by the tests that set no option on it"""
    if (name, lx1) not in _CTX:
        _CTX[name, lx1] = _hip(_case(name, lx1))
    return _CTX[name, lx1]


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for h in _CTX.values():
        h.close()
    for d in (_CASE, _ORACLE, _CTX, _REF):
        d.clear()


def _state(c):
    x, y, z = c.x, c.y, c.z
    m = c.lx1 - 2
    return [np.sin(1.3 * x + z) * np.cos(2.0 * y) * c.mask, np.cos(0.7 * x + 0.2) * np.sin(3.0 * y - z) * c.mask,
            np.sin(x + y) * np.cos(2.0 * z) * c.mask, np.zeros((c.nel, m, m, m))]


def _reference_map(name, lx1, mode):
    if (name, lx1, mode) not in _REF:
        _REF[name, lx1, mode] = _oracle(name, lx1, True).matvec(_state(_case(name, lx1)), adjoint=bool(mode), nsteps=NSTEPS)
    return _REF[name, lx1, mode]


def _map(h, c, mode):
    a, b = h.alloc(2)
    h.upload3(a, *_state(c))
    keep = h.nsteps
    h.set_nsteps(NSTEPS)
    h.matvec(b, a, mode)
    h.set_nsteps(keep)
    out = h.download3(b)
    st = h.stats()
    h.free([a, b])
    return out, st


def _map_errors(out, ref):
    sc = max(np.abs(ref[k]).max() for k in range(3))
    return max(np.abs(out[k] - ref[k]).max() for k in range(3)) / sc, _rel(out[3], ref[3])


def _chain(o, p, masks=None):
    """E p through opgradt -> mask, dssum -> binvm1 mask -> opdiv of the oracle (masks: one per component)"""
    masks = masks or [o.mask] * 3
    w = o.opgradt(p)
    return o.opdiv([o.binvm1 * masks[c] * o.dssum(w[c] * masks[c]) for c in range(3)])


# ---------------------------------------------------------------------------------------------------------------- operators
@pytest.mark.parametrize("name,lx1", OPERATOR_CASES)
def test_element_operators(name, lx1):
    c, o, h = _case(name, lx1), _oracle(name, lx1), _ctx(name, lx1)
    assert h.nsteps == o.nsteps and abs(h.dt - o.dt) < 1e-15
    rng = np.random.default_rng(1)
    u = rng.standard_normal((3,) + c.x.shape)
    p = rng.standard_normal((c.nel,) + (lx1 - 2,) * 3)
    err = dict(axhelm=_rel(h.t_axhelm(u[0], 0.7, 1.3), o.axhelm(u[0], 0.7, 1.3)), dssum=_rel(h.t_dssum(u[1]), o.dssum(u[1])),
               opdiv=_rel(h.t_op3(1, u), o.opdiv(u)), opgradt=_rel(h.t_op3(2, p), np.stack(o.opgradt(p))), eapply=_rel(h.t_eapply(p), _chain(o, p)))
    print(name, lx1, " ".join("%s %.2e" % kv for kv in err.items()))
    assert err["axhelm"] < 1e-12 and err["dssum"] < 1e-13 and err["opdiv"] < 1e-12 and err["opgradt"] < 1e-12 and err["eapply"] < 1e-11


@pytest.mark.parametrize("name,lx1", OPERATOR_CASES)
def test_convection_terms(name, lx1):
    c, o, h = _case(name, lx1), _oracle(name, lx1), _ctx(name, lx1)
    rng = np.random.default_rng(2)
    u = rng.standard_normal((3,) + c.x.shape)
    U = o.ub
    sp = o.spng * o.bm1
    direct = np.stack([-(sp * u[k] + o.convect(u, U[k]) + o.convect(U, u[k])) for k in range(3)])
    a = o.convect_adj(u, U)
    adj = np.stack([-(sp * u[k] + a[k] - o.convect(U, u[k])) for k in range(3)])
    nl = np.stack([-o.convect(u, u[k]) for k in range(3)])
    assert _rel(h.t_op3(3, u, 0), direct) < 1e-12
    assert _rel(h.t_op3(3, u, 1), adj) < 1e-12
    assert _rel(h.t_op3(3, u, 2), nl) < 1e-12
    if lx1 in (8, 10):
        assert _rel(h.t_op3(8, u, 0), direct) < 1e-12
        assert _rel(h.t_op3(8, u, 1), adj) < 1e-12
        assert _rel(h.t_op3(8, u, 0), h.t_op3(3, u, 0)) < 1e-13
    if lx1 == 10:
        assert _rel(h.t_op3(8, u, 2), nl) < 1e-12
        assert _rel(h.t_op3(8, u, 2), h.t_op3(3, u, 2)) < 1e-13


@pytest.mark.parametrize("name,lx1", OPERATOR_CASES)
def test_helmholtz_solve(name, lx1):
    """k_helm<N> with every branch of its fused gather; at lx1 = 10 the resident k_helm_p<10> (helm_pf = 1, the default: eight
    resident workgroups, so that on 10 and 16 elements a workgroup walks more than one) and k_helm<10> (helm_pf = 0)"""
    c, o, h = _case(name, lx1), _oracle(name, lx1), _ctx(name, lx1)
    rng = np.random.default_rng(3)
    r = rng.standard_normal((3,) + c.x.shape)
    ref = np.stack([o.helm_solve(r[k], o.nu, (11.0 / 6.0) / o.dt) for k in range(3)])
    forms = [None] if lx1 != 10 else [1, 0]
    try:
        for pf in forms:
            if pf is not None:
                h.set_option("helm_pf", pf)
                h.set_option("helm_pf_grid", 8)
            out, iters = h.t_op3(5, r, 3)
            print(name, lx1, "helm_pf", pf, "error %.2e, %d iterations" % (_rel(out, ref), iters))
            assert _rel(out, ref) < 1e-9, pf
            assert 0 < iters < 200
    finally:
        if lx1 == 10:
            h.set_option("helm_pf", 1)


# ---------------------------------------------------------------------------------------------------- pressure solve, maps
@pytest.mark.parametrize("name,lx1", STEP_CASES)
def test_pressure_solve(name, lx1):
    c, o, h = _case(name, lx1), _oracle(name, lx1, True), _ctx(name, lx1)
    g = np.random.default_rng(4).standard_normal((c.nel,) + (lx1 - 2,) * 3)
    x, iters = h.t_pres_solve(g)
    err = _rel(x, o.E_solve(g))
    print(name, lx1, "pressure solve %.2e, %d iterations" % (err, iters))
    assert err < 1e-6, iters
    assert 0 < iters <= 48


@pytest.mark.parametrize("mode", [0, 1], ids=["direct", "adjoint"])
@pytest.mark.parametrize("name,lx1", STEP_CASES)
def test_steps_match_oracle(name, lx1, mode):
    c, h = _case(name, lx1), _ctx(name, lx1)
    out, st = _map(h, c, mode)
    ev, ep = _map_errors(out, _reference_map(name, lx1, mode))
    print(name, lx1, "mode", mode, "velocity %.2e pressure %.2e, iterations %d / %d" % (ev, ep, st["helm_iters"], st["pres_iters"]))
    assert st["unconverged"] == 0
    assert ev < 1e-7 and ep < 1e-4


# ------------------------------------------------------------------------------------------------------------ kernel forms
FORM_OPTIONS = ([[("eapply_pipe", f), ("divgs_c3", 1 if f == 1 else 0)] for f in range(6)]      # (divgs_c3 rides along with form 1, as in test_3d_gpu)
                + [[("flat_proj", f)] for f in (0, 1)] + [[("gs_lag", f)] for f in (0, 1, 2)])


@pytest.mark.parametrize("options", FORM_OPTIONS, ids=lambda o: "%s=%d" % o[0])
@pytest.mark.parametrize("name,lx1", [("k5x2-walls", 8), ("k8x2-periodic", 6)])
def test_kernel_forms_against_the_oracle(name, lx1, options):
    """Every form of the pressure iteration's kernels (a form that an order does not build leaves the order's default in place),
    the streaming projection kernels and the lagged Gram-Schmidt passes: each five-step map, direct and adjoint, against the oracle"""
    c = _case(name, lx1)
    h = _hip(c, nproj=4 if options[0][0] == "flat_proj" else 0)
    try:
        for k, v in options:
            h.set_option(k, v)
        for mode in (0, 1):
            out, st = _map(h, c, mode)
            ev, ep = _map_errors(out, _reference_map(name, lx1, mode))
            print(name, lx1, options, "mode", mode, "velocity %.2e pressure %.2e, iterations %d / %d" % (ev, ep, st["helm_iters"], st["pres_iters"]))
            assert st["unconverged"] == 0
            assert ev < 1e-7 and ep < 1e-4
    finally:
        h.close()


@pytest.mark.parametrize("options", [[("divgs_c3", 0)], [("divgs_c3", 1)], [("helm_pf", 0)], [("helm_pf", 1)]], ids=lambda o: "%s=%d" % o[0])
def test_kernel_forms_lx1_10(options):
    c = _case("k5x1", 10)
    h = _hip(c)
    try:
        for k, v in options:
            h.set_option(k, v)
        for mode in (0, 1):
            out, st = _map(h, c, mode)
            ev, ep = _map_errors(out, _reference_map("k5x1", 10, mode))
            print("k5x1 10", options, "mode", mode, "velocity %.2e pressure %.2e" % (ev, ep))
            assert st["unconverged"] == 0
            assert ev < 1e-7 and ep < 1e-4
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------------------- component masks
@pytest.mark.parametrize("lx1", [8, 10])
def test_equal_component_masks_give_the_bits_of_nsk_init(lx1):
    c = _case("k5x2-walls", lx1)
    res = []
    for case in (c, replace(c, cmask=np.stack([c.mask, c.mask, c.mask]))):
        h = _hip(case)
        try:
            out, st = _map(h, c, 0)
            res.append((out, (st["helm_iters"], st["pres_iters"]), h.step_iters()))
        finally:
            h.close()
    assert np.abs(res[0][0][0]).max() > 0 and res[0][1][0] > 0
    assert all(np.array_equal(a, b) for a, b in zip(res[0][0], res[1][0]))
    assert res[0][1] == res[1][1] and all(np.array_equal(a, b) for a, b in zip(res[0][2], res[1][2]))


@pytest.mark.parametrize("lx1", [8, 10])
def test_component_mask_forms_on_the_axis(lx1):
    """Three equal masks take the shared-mask kernels (nsk_init_masks hands them to nsk_init), so the <.., CM = true> forms of the
    gather need masks that differ: the fan between two symmetry planes ('SYM' at both ends: w fixed there, u and v free -- the axis'
    end vertices with their corner lists of five are then free in two components).  Velocity solve and E against the oracle's
    operators with one mask per component; same bounds as for the shared mask."""
    from nekstab_amd import mesh3d
    from oracle.linns3d import LinNS3D
    c = mesh3d.extrude_case(fan_mesh.case2(5, 1, lx1), 2, fan_mesh.LZ, periodic=False, zcodes=("SYM", "SYM"))
    c.ub = fan_mesh.baseflow3(c.x, c.y, c.z)
    assert c.cmask is not None and not np.array_equal(c.cmask[0], c.cmask[2])
    axis = np.bincount(c.gid.ravel())[c.gid] >= 5
    assert (c.cmask[0][axis] == 1.0).any() and (c.cmask[2][axis] == 0.0).any()
    os_ = [LinNS3D(x=c.x, y=c.y, z=c.z, gid=c.gid, nglob=c.nglob, mask=c.cmask[k], ub=c.ub, spng=c.spng, re=c.re, endtime=c.endtime,
                   has_outflow=c.has_outflow, build_solvers=False) for k in range(3)]
    h = _hip(c)
    try:
        rng = np.random.default_rng(6)
        r = rng.standard_normal((3,) + c.x.shape)
        p = rng.standard_normal((c.nel,) + (lx1 - 2,) * 3)
        ref = np.stack([os_[k].helm_solve(r[k], os_[k].nu, (11.0 / 6.0) / os_[k].dt) for k in range(3)])
        for pf in ([None] if lx1 != 10 else [1, 0]):
            if pf is not None:
                h.set_option("helm_pf", pf)
                h.set_option("helm_pf_grid", 8)
            out, iters = h.t_op3(5, r, 3)
            print("lx1", lx1, "helm_pf", pf, "velocity solve with component masks %.2e, %d iterations" % (_rel(out, ref), iters))
            assert _rel(out, ref) < 1e-9 and 0 < iters < 200
        e = _rel(h.t_eapply(p), _chain(os_[0], p, [c.cmask[k] for k in range(3)]))
        print("lx1", lx1, "E with component masks %.2e" % e)
        assert e < 1e-11
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------------------------- shards
def _partition(kind, k, nranks, layers=1):
    """elements of the fan's sector i go to rank i * nranks // k: every rank holds a sector, the axis is shared by all ranks.
    kind 'fan3': k elements per layer; 'fan2': k inner elements, then the 2k of the second ring (ring element j lies on sector j // 2)"""
    sector = np.arange(k) * nranks // k
    if kind == "fan3":
        return np.tile(sector, layers).astype(np.int32)
    return np.concatenate([sector, np.repeat(sector, 2)]).astype(np.int32)


@pytest.mark.parametrize("nranks", [2, 3])
def test_sharded_hexahedra(nranks):
    from nekstab_amd.sharded import ShardGroup
    name, lx1 = "k5x2-walls", 6
    c, o = _case(name, lx1), _oracle(name, lx1)
    part = _partition("fan3", 5, nranks, 2)
    centre = fan_mesh.centre_node(c)
    assert sorted(np.unique(part[np.any(c.gid.reshape(c.nel, -1) == centre, axis=1)])) == list(range(nranks))
    h = _hip(c, tol_pres=1e-7)
    try:
        g = ShardGroup(h, c, nranks, part)
        rng = np.random.default_rng(0)
        u = rng.standard_normal(c.x.shape)
        p = rng.standard_normal((c.nel, 4, 4, 4))
        assert np.abs(g.group_test(0, u) - o.dssum(u)).max() < 1e-12 * np.abs(u).max() * 8
        er = _chain(o, p)
        assert np.abs(g.group_test(1, p) - er).max() < 1e-12 * np.abs(er).max()
        ref, _ = _map(h, c, 0)
        g.set_nsteps(NSTEPS)
        sq, sf = g.alloc(2)
        g.upload3(sq, *_state(c))
        g.matvec(sf, sq, 0)
        got = g.download3(sf)
        sc = max(np.abs(ref[k]).max() for k in range(3))
        ev = max(np.abs(got[k] - ref[k]).max() for k in range(3)) / sc
        print("%d ranks around the axis, hexahedra: velocity %.2e pressure %.2e against the single rank" % (nranks, ev, _rel(got[3], ref[3])))
        assert ev < 1e-8 and _rel(got[3], ref[3]) < 1e-4
        g.free([sq, sf]); g.close()
    finally:
        h.close()


@pytest.mark.parametrize("nranks", [2, 3])
def test_sharded_quadrilaterals(nranks):
    from nekstab_amd.sharded import ShardGroup
    from tests.conftest import make_oracle
    c = fan_mesh.case2(8, 2, 8)
    o = make_oracle(c, build_solvers=False)
    part = _partition("fan2", 8, nranks)
    centre = fan_mesh.centre_node(c)
    assert sorted(np.unique(part[np.any(c.gid.reshape(c.nel, -1) == centre, axis=1)])) == list(range(nranks))
    h = _hip(c, tol_pres=1e-6)
    try:
        g = ShardGroup(h, c, nranks, part)
        rng = np.random.default_rng(0)
        u = rng.standard_normal(c.x.shape)
        p = rng.standard_normal((c.nel, 6, 6))
        assert np.abs(g.group_test(0, u) - o.dssum(u)).max() < 1e-12 * np.abs(u).max() * 8
        wx, wy = o.opgradt(p)
        fac = o.binvm1 * o.mask
        er = o.opdiv(fac * o.dssum(wx * o.mask), fac * o.dssum(wy * o.mask))
        assert np.abs(g.group_test(1, p) - er).max() < 1e-12 * np.abs(er).max()
        q = (np.sin(1.3 * c.x + 0.2) * np.cos(0.9 * c.y) * c.mask, np.cos(0.7 * c.x) * np.sin(1.1 * c.y + 0.3) * c.mask, np.zeros((c.nel, 6, 6)))
        h.set_nsteps(NSTEPS)
        vq, vf = h.alloc(2)
        h.upload(vq, *q)
        h.matvec(vf, vq, 0)
        ref = h.download(vf)
        g.set_nsteps(NSTEPS)
        sq, sf = g.alloc(2)
        g.upload(sq, *q)
        g.matvec(sf, sq, 0)
        got = g.download(sf)
        num = np.sqrt(sum(np.sum(o.bm1 * (a - b) ** 2) for a, b in zip(got[:2], ref[:2])))
        den = np.sqrt(sum(np.sum(o.bm1 * b ** 2) for b in ref[:2]))
        print("%d ranks around the centre, quadrilaterals: velocity %.2e pressure %.2e against the single rank" % (nranks, num / den, _rel(got[2], ref[2])))
        assert num / den < 1e-9
        assert np.abs(got[2] - ref[2]).max() < 1e-5 * np.abs(ref[2]).max()
        g.free([sq, sf]); g.close()
    finally:
        h.close()
