"""The fixtures of irregular topology (tests/fan_mesh.py) on the CPU: each holds the copy counts it is there for, the oracle is
sane on them whatever a kernel does, and the comparisons of tests/test_irregular_gpu.py / test_irregular3d_gpu.py have teeth: a
gather that drops one copy at the centre node moves the reference by at least 1000 times every bound used there."""
import numpy as np
import pytest

from tests import fan_mesh

# bounds of the GPU files: relative on operators, on the velocity scale / relative on the pressure for solves and maps
BOUND_OPERATOR, BOUND_DSSUM, BOUND_VELOCITY, BOUND_PRESSURE = 1e-12, 1e-13, 1e-7, 1e-4


def _oracle2(c, **kw):
    from tests.conftest import make_oracle
    return make_oracle(c, **kw)


def _oracle3(c, solvers=False):
    from oracle.linns3d import LinNS3D
    return LinNS3D(x=c.x, y=c.y, z=c.z, gid=c.gid, nglob=c.nglob, mask=c.mask, ub=c.ub, spng=c.spng, re=c.re,
                   endtime=c.endtime, has_outflow=c.has_outflow, build_solvers=solvers)


# ---- census: (k, nz, periodic) -> {copies: (corner nodes, other nodes)} on the axis, n = lx1
CENSUS3 = {
    (5, 2, False): lambda n: {5: (2, 2 * (n - 2)), 10: (1, 0)},          # corner lists of 5, a corner beyond its list, wide edge nodes
    (8, 2, True): lambda n: {8: (0, 2 * (n - 2)), 16: (2, 0)},           # every axis vertex beyond its list, edge nodes of 8
    (8, 1, False): lambda n: {8: (2, n - 2)},                            # corner lists exactly full, edge nodes of 8
    (6, 2, False): lambda n: {6: (2, 2 * (n - 2)), 12: (1, 0)},
    (3, 1, False): lambda n: {3: (2, n - 2)},                            # fits the 4-wide table
}


@pytest.mark.parametrize("key", list(CENSUS3), ids=lambda k: "k%d-nz%d-%s" % (k[0], k[1], "periodic" if k[2] else "walls"))
@pytest.mark.parametrize("lx1", [6, 10])
def test_census_hexahedra(key, lx1):
    k, nz, per = key
    c = fan_mesh.fan3(k, nz, lx1, per)
    assert c.nel == k * nz
    got = fan_mesh.census(c.gid, 3)
    for copies, (corner, other) in CENSUS3[key](lx1).items():
        assert got.get(copies) == (corner, other), (copies, got)
    assert max(got) == max(CENSUS3[key](lx1))                       # nothing wider than the axis
    # every other node of the mesh fits the 4-wide table
    assert all(cp <= 4 for cp in got if cp not in CENSUS3[key](lx1))


@pytest.mark.parametrize("k", [3, 5, 6, 8, 9])
def test_census_quadrilaterals(k):
    for rings in (1, 2):
        c = fan_mesh.case2(k, rings, 6)
        assert c.nel == k * (1 if rings == 1 else 3) and c.has_outflow
        got = fan_mesh.census(c.gid, 2)
        want = {k: (1, 0)}
        if rings == 2:
            want[3] = (k + (1 if k == 3 else 0), 0)
            want[4] = (k, 0)
            if k == 3:
                want = {3: (4, 0), 4: (3, 0)}
        for copies, cn in want.items():
            assert got.get(copies) == cn, (rings, copies, got)
        assert all(cn[1] == 0 for cp, cn in got.items() if cp > 2)   # only vertices have more than two copies in 2-D


# ---- the oracle on these meshes, no kernel involved
@pytest.mark.parametrize("k,rings", [(3, 2), (5, 2), (6, 2), (8, 2), (5, 1), (9, 1)])
def test_mass_matrix_sums_to_the_area(k, rings):
    m, _ = fan_mesh.fan(k, rings)
    a = fan_mesh.area(m)
    x, y = m.xc, m.yc                                                # every element convex and counter-clockwise
    for i in range(4):
        j, l = (i + 1) % 4, (i + 2) % 4
        assert np.all((x[:, j] - x[:, i]) * (y[:, l] - y[:, j]) - (y[:, j] - y[:, i]) * (x[:, l] - x[:, j]) > 0)
    for lx1 in (6, 8, 10, 12):
        o = _oracle2(fan_mesh.case2(k, rings, lx1), build_solvers=False)
        assert abs(o.bm1.sum() - a) < 1e-13 * a, (lx1, o.bm1.sum(), a)
    if (k, rings) == (5, 2):
        assert abs(a - 10.0373206910322) < 1e-12


@pytest.mark.parametrize("key", list(CENSUS3), ids=lambda k: "k%d-nz%d-%s" % (k[0], k[1], "periodic" if k[2] else "walls"))
def test_volume_and_divergence_hexahedra(key):
    k, nz, per = key
    vol = fan_mesh.area(fan_mesh.fan(k, 1)[0]) * fan_mesh.LZ
    for lx1 in (6, 8):
        c = fan_mesh.fan3(k, nz, lx1, per)
        o = _oracle3(c)
        assert abs(o.bm1.sum() - vol) < 1e-13 * vol
        d = o.opdiv([c.x, -c.y, np.zeros_like(c.x)])
        assert np.abs(d).max() < 1e-14 * np.abs(o.opdiv([c.x, c.y, c.z])).max()


@pytest.mark.parametrize("k,rings,lx1", [(5, 2, 6), (8, 2, 8), (3, 2, 8), (6, 2, 10)])
def test_divergence_and_E_quadrilaterals(k, rings, lx1):
    c = fan_mesh.case2(k, rings, lx1)
    o = _oracle2(c, factorize_pressure=False)
    assert np.abs(o.opdiv(c.x, -c.y)).max() < 1e-14 * np.abs(o.opdiv(c.x, c.y)).max()
    p = np.random.default_rng(0).standard_normal((c.nel, lx1 - 2, lx1 - 2))
    wx, wy = o.opgradt(p)
    fac = o.binvm1 * o.mask
    chain = o.opdiv(fac * o.dssum(wx * o.mask), fac * o.dssum(wy * o.mask))
    ref = (o._Emat @ p.ravel()).reshape(p.shape)
    assert np.abs(chain - ref).max() < 1e-13 * np.abs(ref).max()     # two orders of summation of the same O(100)-term sums


@pytest.mark.parametrize("key", [(5, 2, False), (8, 2, True)], ids=["k5-walls", "k8-periodic"])
def test_E_chain_hexahedra(key):
    k, nz, per = key
    c = fan_mesh.fan3(k, nz, 6, per)
    o = _oracle3(c, solvers=True)
    p = np.random.default_rng(0).standard_normal((c.nel, 4, 4, 4))
    ref = (o._Emat @ p.ravel()).reshape(p.shape)
    assert np.abs(chain3(o, p) - ref).max() < 1e-13 * np.abs(ref).max()


def chain3(o, p):
    """E p through the operator chain opgradt -> mask, dssum -> binvm1 mask -> opdiv of the 3-D oracle"""
    w = o.opgradt(p)
    fac = o.binvm1 * o.mask
    return o.opdiv([fac * o.dssum(w[c] * o.mask) for c in range(3)])


# ---- teeth
def _drop_one_copy(o, c, free=False):
    """o.dssum without the last local copy of the node with the most copies (free: of the free node with the most copies)"""
    cnt = np.bincount(c.gid.ravel(), minlength=c.nglob)
    if free:
        g = np.ones(c.nglob)
        np.minimum.at(g, c.gid.ravel(), c.mask.ravel())
        cnt = cnt * (g > 0)
    node = int(np.argmax(cnt))
    drop = np.flatnonzero(c.gid.ravel() == node)[-1]
    clean = o.dssum

    def broken(f):
        g = np.array(f, dtype=np.float64).ravel()
        g[drop] = 0.0
        return clean(g.reshape(np.shape(f)))
    return broken, int(cnt[node])


def test_teeth_quadrilaterals():
    """fan(5, 2) at lx1 = 6: the reference with one of the centre's five copies dropped from its gather"""
    c = fan_mesh.case2(5, 2, 6)
    o = _oracle2(c)
    rng = np.random.default_rng(1)
    u = rng.standard_normal(c.x.shape)
    p = rng.standard_normal((c.nel, 4, 4))
    q = (np.sin(1.3 * c.x + 0.2) * np.cos(0.9 * c.y) * c.mask, np.cos(0.7 * c.x) * np.sin(1.1 * c.y + 0.3) * c.mask, np.zeros((c.nel, 4, 4)))

    def observe():
        wx, wy = o.opgradt(p)
        fac = o.binvm1 * o.mask
        return o.dssum(u), o.opdiv(fac * o.dssum(wx * o.mask), fac * o.dssum(wy * o.mask)), o.matvec(q, nsteps=5)
    d0, e0, f0 = observe()
    o.dssum, copies = _drop_one_copy(o, c)
    assert copies == 5
    d1, e1, f1 = observe()
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    sc = max(np.abs(f0[0]).max(), np.abs(f0[1]).max())
    dv = max(np.abs(f1[0] - f0[0]).max(), np.abs(f1[1] - f0[1]).max()) / sc
    print("one copy dropped: dssum %.2e, E %.2e, 5-step map velocity %.2e, pressure %.2e" % (rel(d1, d0), rel(e1, e0), dv, rel(f1[2], f0[2])))
    assert rel(d1, d0) >= 1e3 * BOUND_DSSUM and rel(e1, e0) >= 1e3 * BOUND_OPERATOR
    assert dv >= 1e3 * BOUND_VELOCITY and rel(f1[2], f0[2]) >= 1e3 * BOUND_PRESSURE


def test_teeth_hexahedra():
    """fan3(8, 2, periodic) at lx1 = 6: one of sixteen copies of an axis vertex dropped"""
    c = fan_mesh.fan3(8, 2, 6, True)
    o = _oracle3(c, solvers=True)
    rng = np.random.default_rng(1)
    u = rng.standard_normal(c.x.shape)
    p = rng.standard_normal((c.nel, 4, 4, 4))
    x, y, z = c.x, c.y, c.z
    q = [np.sin(1.3 * x + z) * np.cos(2.0 * y) * c.mask, np.cos(0.7 * x + 0.2) * np.sin(3.0 * y - z) * c.mask,
         np.sin(x + y) * np.cos(2.0 * z) * c.mask, np.zeros((c.nel, 4, 4, 4))]
    observe = lambda: (o.dssum(u), chain3(o, p), o.matvec(q, nsteps=5))
    d0, e0, f0 = observe()
    o.dssum, copies = _drop_one_copy(o, c, free=True)
    assert copies == 16
    d1, e1, f1 = observe()
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    sc = max(np.abs(f0[k]).max() for k in range(3))
    dv = max(np.abs(f1[k] - f0[k]).max() for k in range(3)) / sc
    print("one copy dropped: dssum %.2e, E %.2e, 5-step map velocity %.2e, pressure %.2e" % (rel(d1, d0), rel(e1, e0), dv, rel(f1[3], f0[3])))
    assert rel(d1, d0) >= 1e3 * BOUND_DSSUM and rel(e1, e0) >= 1e3 * BOUND_OPERATOR
    assert dv >= 1e3 * BOUND_VELOCITY and rel(f1[3], f0[3]) >= 1e3 * BOUND_PRESSURE
