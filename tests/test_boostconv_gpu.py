"""BoostConv on the device (nsk_boostconv_* / nsk_group_boostconv_*, nekstab_amd/fixedp.py; core/fixedp.f:282-468).

The algebra of nsk_boostconv_core against np_boostconv_core, the numpy restatement of the reference (modified Gram-Schmidt and
all); the map with no call against nsk_nonlinear_map (bits); the map against the CPU oracle with np_boostconv_core behind the
selected steps; hexahedra and shards against the quadrilateral single-rank map; the refusals and the driver.

BOUNDS are not chosen.  Algebra: ten times the difference, measured here on the CPU, between the restatement and a numpy model
of the device's solve (Gram matrix, diagonal scaling, pivoted Cholesky) on the same inputs.  Maps: ten times S times the
device-oracle (hexahedra-quadrilaterals, shards-single rank) difference of the UNFORCED map recorded in tests/test_sfd_gpu.py,
S the factor by which the oracle's BoostConv chain amplifies a 1e-12 perturbation of every post-step velocity (printed)."""
import os
import re

import numpy as np
import pytest

from tests.conftest import GOLDEN, make_oracle
from tests.test_boostconv_np import linear_problem
from tests.test_sfd_gpu import HEX_MEASURED, SHARD_MEASURED, _channel, _perturbed, _planes, _relw, _start

pytestmark = pytest.mark.gpu

ORACLE_UNFORCED = 6.6e-14          # device vs oracle, unforced map at 1e-14 / 1e-10 (tests/test_sfd_gpu.py, test_forced_steps_against_the_oracle)
EPS = 1e-12


def _context(case):
    from nekstab_amd.capi import NekStabHip
    return NekStabHip(case, case.meta["vert"], case.meta["nvert"], tol_helm=1e-12, tol_pres=1e-3, tol_relative=1,
                      nproj=8, max_helm_iter=150, max_pres_iter=96)


@pytest.fixture(scope="module")
def cyl():
    from nekstab_amd import mesh
    case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6, spng_str=0.0)
    h = _context(case)
    yield case, h
    h.close()


# ---- 1. the algebra ------------------------------------------------------------------------------------------------------------
def np_gram_core(state, r, bm1, snp):
    """The device's form of boostconv_core in numpy: the Gram matrix of Y, scaled by its diagonal, columns with D_jj < 1e-60
    dropped, Cholesky with diagonal pivoting, a pivot below snp 2^-52 ends it.  For the bound of the algebra test only."""
    r = np.array(r, dtype=np.float64)
    ip = lambda a, b: sum(float(np.sum(a[k] * bm1 * b[k])) for k in range(a.shape[0]))
    if not state:
        X, Y = np.zeros((snp,) + r.shape), np.zeros((snp,) + r.shape)
        X[0], Y[0] = r, r
        state.update(X=X, Y=Y, rot=1)
        return r.copy()
    X, Y, rot = state["X"], state["Y"], state["rot"]
    Y[rot - 1] -= r
    X[rot - 1] -= Y[rot - 1]
    D = np.array([[ip(Y[i], Y[j]) for j in range(snp)] for i in range(snp)])
    g = np.array([ip(Y[j], r) for j in range(snp)])
    idx = [j for j in range(snp) if D[j, j] >= 1e-60]
    s = np.array([1.0 / np.sqrt(D[j, j]) for j in idx])
    W = D[np.ix_(idx, idx)] * s[:, None] * s[None, :]
    w = g[idx] * s
    m = len(idx)
    perm, L, rank = list(range(m)), np.zeros((m, m)), m
    for k in range(m):
        q = k + int(np.argmax([W[perm[t], perm[t]] - L[perm[t], :k] @ L[perm[t], :k] for t in range(k, m)]))
        piv = W[perm[q], perm[q]] - L[perm[q], :k] @ L[perm[q], :k]
        if not piv >= snp * 2.0 ** -52:
            rank = k
            break
        perm[k], perm[q] = perm[q], perm[k]
        L[perm[k], k] = np.sqrt(piv)
        for t in range(k + 1, m):
            L[perm[t], k] = (W[perm[t], perm[k]] - L[perm[t], :k] @ L[perm[k], :k]) / L[perm[k], k]
    P = perm[:rank]
    c = np.zeros(snp)
    if rank:
        Lr = L[P, :rank]
        z = np.linalg.solve(Lr.T, np.linalg.solve(Lr, w[P]))
        for t, pt in enumerate(P):
            c[idx[pt]] = z[t] * s[pt]
    rot = rot % snp + 1
    Y[rot - 1] = r
    xi = r.copy()
    for j in range(snp):
        xi += X[j] * c[j]
    X[rot - 1] = xi
    state["rot"] = rot
    return xi.copy()


def _residual_fields(case, ncalls=8):
    """smooth masked fields of decreasing size, as the residuals of a converging run: products of sines of x and y"""
    x, y, m = case.x, case.y, case.mask
    return [np.stack([0.6 ** k * np.sin(0.11 * (k + 1) * x + 0.3 * k) * np.cos(0.23 * (k + 2) * y) * m,
                      0.6 ** k * np.cos(0.07 * (k + 2) * x) * np.sin(0.31 * (k + 1) * y + 0.2 * k) * m]) for k in range(ncalls)]


def _core(h, r):
    v, = h.alloc(1)
    p = np.full((r.shape[1], 4, 4), 0.25)
    h.upload(v, r[0], r[1], p)
    h.boostconv_core(v)
    out = h.download(v)
    h.free([v])
    assert np.array_equal(out[2], p)                               # the pressure is not touched
    return np.stack(out[:2])


@pytest.mark.parametrize("snp", [3, 1])
def test_core_is_the_numpy_restatement(cyl, snp):
    from nekstab_amd import fixedp
    case, h = cyl
    bm1 = make_oracle(case, build_solvers=False).bm1
    rel = lambda a, b: float(np.sqrt(np.sum(bm1 * (a - b) ** 2) / np.sum(bm1 * b ** 2)))
    rs = _residual_fields(case)
    sa, sb = {}, {}
    ref = [fixedp.np_boostconv_core(sa, r, bm1, snp) for r in rs]
    fig = max(rel(np_gram_core(sb, r, bm1, snp), x) for r, x in zip(rs, ref))
    print("snp = %d: Gram + pivoted Cholesky vs Gram-Schmidt in numpy, xi of 8 calls: %.2e" % (snp, fig))
    assert fig <= 1e-10
    bound = 10.0 * max(fig, 2.0 ** -52)
    h.boostconv_init(snp)
    err = [rel(_core(h, r), x) for r, x in zip(rs, ref)]
    print("snp = %d: device vs restatement, xi per call:" % snp, " ".join("%.1e" % e for e in err), "(bound %.2e)" % bound)
    assert all(rel(x, r) > 1e-3 for x, r in zip(ref[1:], rs[1:]))       # teeth: xi is not r after the first call
    assert max(err) <= bound


def test_core_solves_the_linear_problem_and_holds(cyl):
    """The rank-3 problem of tests/test_boostconv_np.py, r evaluated on the host from downloaded fields: at the fifth call the
    residual is at rounding level, and the three calls after it -- stored differences that are rounding noise, the case the
    safeguarded solve is there for -- keep it."""
    case, h = cyl
    bm1 = make_oracle(case, build_solvers=False).bm1
    shape = (2,) + case.x.shape
    resid, norm = linear_problem(shape, bm1, 3)
    h.boostconv_init(3)
    v, hist = np.zeros(shape), []
    for _ in range(8):
        r = resid(v)
        hist.append(norm(r))
        v = v + _core(h, r)
    print("linear problem on the device, |r| per call:", " ".join("%.2e" % x for x in hist))
    assert hist[3] > 1e-3 and all(x <= 1e-11 for x in hist[4:]) and np.all(np.isfinite(v))


def test_init_resets_the_state(cyl):
    case, h = cyl
    rs = _residual_fields(case, 3)
    h.boostconv_init(3)
    a = [_core(h, r) for r in rs]
    h.boostconv_init(3)
    b = [_core(h, r) for r in rs]
    assert np.array_equal(a[0], rs[0]) and not np.array_equal(a[2], rs[2])      # a first call returns r, a later one does not
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    h.boostconv_init(2)                                                       # another size: reallocated
    assert np.array_equal(_core(h, rs[0]), rs[0])


# ---- 2. no call, no change -----------------------------------------------------------------------------------------------------
def test_a_map_without_a_call_is_the_nonlinear_map(cyl):
    case, _ = cyl
    h = _context(case)
    try:
        h.set_option("proj_reset", 1)
        q = _start(case, h)
        vq, vf, vg = h.alloc(3)
        h.upload(vq, *q)
        h.set_nsteps(6)
        h.nonlinear_map(vf, vq)
        h.boostconv_init(3)
        res = h.boostconv_map(vg, vq, 8, 1)                       # global steps 2 .. 7: no multiple of 8
        f, g = h.download(vf), h.download(vg)
        assert len(res) == 0 and np.abs(f[0]).max() > 0 and all(np.array_equal(a, b) for a, b in zip(f, g))
        res = h.boostconv_map(vg, vq, 8, 0)                       # step0 = 0: the call at step 0 is a first call, xi = r = v^0
        g = h.download(vg)
        assert len(res) == 1 and all(np.array_equal(a, b) for a, b in zip(f, g))
        bm1 = make_oracle(case, build_solvers=False).bm1
        assert abs(res[0] / np.sqrt(sum(np.sum(bm1 * x ** 2) for x in q[:2]) / np.sum(bm1)) - 1.0) <= 1e-13
        h.free([vq, vf, vg])
    finally:
        h.close()


# ---- 3. against the CPU oracle -------------------------------------------------------------------------------------------------
def _smooth(o_or_case):
    c = o_or_case
    return np.stack([np.sin(0.9 * c.x + 0.3) * np.cos(1.1 * c.y), np.cos(0.7 * c.x) * np.sin(1.3 * c.y + 0.1)]) * c.mask


def _oracle_bcv(o, case, q, splits, snp, skip, eps=0.0):
    """BoostConv on the oracle by the reference's ordering: maps of `splits` steps (new_state: the BDF / EXT ramp restarts), the
    global step count and the BoostConv state carried.  eps: every post-step velocity moved by eps |v| x a smooth masked field.
    Returns (u, v, p), residu per call."""
    from nekstab_amd import fixedp
    vol = float(np.sum(o.bm1))
    state, res, step0 = {}, [], 0
    g = _smooth(case)
    for n in splits:
        st = o.new_state(q)
        for j in range(0, n + 1):
            if j > 0:
                st = o.step_nonlinear(st, j)
                if eps:
                    sc = eps * max(np.abs(st["u"]).max(), np.abs(st["v"]).max())
                    st["u"], st["v"] = st["u"] + sc * g[0], st["v"] + sc * g[1]
            if (j == 0 and step0 == 0) or (j > 0 and (step0 + j) % skip == 0):
                vel = np.stack([st["u"], st["v"]])
                lag = np.stack(st["ulag"][0]) if j > 0 else np.zeros_like(vel)
                r = vel - lag
                res.append(np.sqrt(np.sum(o.bm1[None] * r ** 2) / vol))
                xi = fixedp.np_boostconv_core(state, r, o.bm1, snp)
                st["u"], st["v"] = lag[0] + xi[0], lag[1] + xi[1]
        q = (st["u"], st["v"], st["p"])
        step0 += n
    return q, np.array(res)


def _device_bcv(be, q, splits, snp, skip, ndim=2):
    up, down = (be.upload3, be.download3) if ndim == 3 else (be.upload, be.download)
    vq, vf = be.alloc(2)
    up(vq, *q)
    be.boostconv_init(snp)
    res, step0 = [], 0
    for n in splits:
        be.set_nsteps(n)
        res = np.concatenate([res, be.boostconv_map(vf, vq, skip, step0)])
        assert be.stats()["unconverged"] == 0
        be.copy(vq, vf)
        step0 += n
    f = down(vf)
    be.free([vq, vf])
    return f, res


_ORUNS = {}


def _oracle_cyl(case, splits):
    """(reference run, residu, S) of the cylinder chain; the oracle is test_sfd_gpu's construction without the sponge channel"""
    if "o" not in _ORUNS:
        o = make_oracle(case)
        o.set_baseflow(np.stack(_perturbed(case)[:2]))
        _ORUNS["o"] = o
    o = _ORUNS["o"]
    if splits not in _ORUNS:
        q = _perturbed(case)
        ref, rref = _oracle_bcv(o, case, q, splits, 3, 2)
        per, rper = _oracle_bcv(o, case, q, splits, 3, 2, EPS)
        vn = float(np.sqrt(sum(np.sum(o.bm1 * y ** 2) for y in ref[:2]) / np.sum(o.bm1)))
        _ORUNS[splits] = (ref, rref, _relw(per, ref, o.bm1) / EPS, float(np.abs(rper - rref).max()) / vn / EPS, vn)
    return (o,) + _ORUNS[splits]


@pytest.mark.parametrize("splits", [(9,), (5, 4)], ids=["one-map", "two-maps"])
def test_map_against_the_oracle(cyl, splits):
    """snp = 3, skip = 2: calls at the global steps 0, 2, 4, 6, 8 -- the rotation wraps at the fifth; in the (5, 4) split the
    second map's calls fall on its odd steps (step0 = 5 carried).  A call on a map's last step: the channel tests below.
    The bound is a relative size of the VELOCITY: S is measured on f in the velocity's bm1 norm, 6.6e-14 is a velocity difference.
    f is compared in that norm, and every residu -- the l2 norm of a velocity DIFFERENCE, 1.4e-4 to 4e-5 of the velocity here --
    by its error against the velocity's l2 norm: a velocity error of relative size d moves r = v - v_before by d |v|, i.e.
    residu by up to d |v|, which is d |v| / residu = 2e4 d of residu itself.  The perturbed oracle run gives the same
    picture: the residu's own amplification, in units of the velocity, is printed as S_r and stays below S.
    Measured on an MI355X: (9,): S = 1.31, f 7.2e-14, residu 3.5e-14 of the velocity (6.5e-10 of itself);
    (5, 4): S = 5.23, f 7.7e-13, residu 3.5e-14 (9.2e-12 of itself); S_r = 2e-3, 1e-3."""
    case, h = cyl
    try:
        q = _start(case, h)
        h.set_tolerances(1e-14, 1e-10, 1)
        o, ref, rref, S, Sr, vn = _oracle_cyl(case, splits)
        assert abs(h.dt - o.dt) < 1e-15
        bound = 10.0 * S * ORACLE_UNFORCED
        f, res = _device_bcv(h, q, splits, 3, 2)
        assert len(res) == len(rref) == 5
        ev, er = _relw(f, ref, o.bm1), float(np.abs(res - rref).max()) / vn
        print("BoostConv vs oracle, maps of", splits, "steps: S = %.3g (residu: S_r = %.3g), bound %.2e: f %.2e  residu %.2e of the velocity, %.2e of itself"
              % (S, Sr, bound, ev, er, float(np.abs(res / rref - 1.0).max())), "residu", res)
        assert S <= 1e4
        assert ev <= bound and er <= bound
        # teeth, on the oracle alone: the accelerated run and the plain 9-step map differ by more than a thousand bounds
        if "plain" not in _ORUNS:
            _ORUNS["plain"] = o.nonlinear_map(q, nsteps=9)
        if splits == (9,):
            teeth = _relw(ref, _ORUNS["plain"], o.bm1)
            print("oracle, BoostConv vs plain map: %.2e" % teeth)
            assert teeth > 1e3 * bound
    finally:
        h.set_tolerances(1e-12, 1e-3, 1)


# ---- 4. hexahedra and shards on the channel of tests/sym_box.py ----------------------------------------------------------------
NCH, SNP, SKIP = 6, 3, 2               # calls at the steps 0, 2, 4, 6
_CH = {}


def _channel_S(lx1):
    """S of the channel chain, from the CPU oracle of the quadrilateral case"""
    if ("S", lx1) not in _CH:
        from tests import sym_box
        c, q = sym_box.case(lx1, False)
        o = make_oracle(c)
        ref, _ = _oracle_bcv(o, c, q, (NCH,), SNP, SKIP)
        per, _ = _oracle_bcv(o, c, q, (NCH,), SNP, SKIP, EPS)
        _CH[("S", lx1)] = _relw(per, ref, o.bm1) / EPS
    return _CH[("S", lx1)]


def _quad(lx1):
    if ("quad", lx1) not in _CH:
        c, q, w, h = _channel(lx1, 2)
        try:
            _CH[("quad", lx1)] = _device_bcv(h, q, (NCH,), SNP, SKIP) + (h.dt,)
        finally:
            h.close()
    return _CH[("quad", lx1)]


@pytest.mark.parametrize("lx1", [6, 8])
def test_hexahedra_equal_quadrilaterals(lx1):
    S = _channel_S(lx1)
    bound = 10.0 * S * max(HEX_MEASURED[lx1][:2])
    f2, r2, dt2 = _quad(lx1)
    c3, q3, w2, h3 = _channel(lx1, 3)
    try:
        assert h3.dt == dt2
        f3, r3 = _device_bcv(h3, q3, (NCH,), SNP, SKIP, 3)
    finally:
        h3.close()
    ev = max(_relw(p, f2, w2) for p in _planes(f3, w2.shape[0]))
    vz = float(np.abs(f3[2]).max() / max(np.abs(f2[0]).max(), np.abs(f2[1]).max()))
    er = float(np.abs(r3 / r2 - 1.0).max())
    print("lx1 = %d, BoostConv hex vs quad: S = %.3g, bound %.2e: f %.2e  vz %.2e  residu %.2e" % (lx1, S, bound, ev, vz, er))
    assert len(r3) == 4 and ev <= bound and vz <= bound and er <= bound


@pytest.mark.parametrize("key", [(2, 8, 2), (2, 8, 3), (3, 6, 2)], ids=lambda k: "%dd-lx%d-%dranks" % k)
def test_shards_equal_the_single_rank(key):
    """nsk_group_boostconv_map: the sums of a call run over all ranks, one residu array for all of them."""
    from nekstab_amd.sharded import ShardGroup
    ndim, lx1, R = key
    S = _channel_S(lx1)
    bound = 10.0 * S * SHARD_MEASURED[key]
    c, q, w2, h = _channel(lx1, ndim)
    try:
        one = _device_bcv(h, q, (NCH,), SNP, SKIP, ndim)
        g = ShardGroup(h, c, R)
        try:
            many = _device_bcv(g, q, (NCH,), SNP, SKIP, ndim)
        finally:
            g.close()
    finally:
        h.close()
    if ndim == 2:
        ev = _relw(many[0], one[0], w2)
    else:
        ev = float(np.sqrt(sum(np.sum((x - y) ** 2) for x, y in zip(many[0][:3], one[0][:3])) / sum(np.sum(y ** 2) for y in one[0][:3])))
    er = float(np.abs(many[1] / one[1] - 1.0).max())
    print(key, "BoostConv shards vs single rank: S = %.3g, bound %.2e: f %.2e  residu %.2e" % (S, bound, ev, er))
    assert len(many[1]) == 4 and ev <= bound and er <= bound


# ---- 5. residu (and with it c) identical on every rank of two processes ---------------------------------------------------------
def test_residu_is_identical_on_every_rank_of_two_processes():
    """Two ranks, one process each, sharing this GPU, sums over gloo on the host: the all-reduce branch of the sums of a call."""
    import subprocess
    import sys
    from tests.conftest import ROOT
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29688", os.path.join(ROOT, "tests", "mp_boostconv_worker.py")],
                         capture_output=True, text=True, timeout=600, env=env)
    print([l for l in out.stdout.splitlines() if "MPBCV" in l], out.stderr[-1500:] if out.returncode else "")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count("MPBCV rank") == 2


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    import ctypes as C
    from nekstab_amd.capi import NskError
    from nekstab_amd.sharded import ShardGroup
    case, _, _, h = _channel(6, 2)                               # (its own context: a lane and shards are cut from it)
    try:
        h.set_nsteps(2)
        a, b = h.alloc(2)
        res, nc = np.zeros(4), C.c_int(0)
        rp, lib = res.ctypes.data_as(C.POINTER(C.c_double)), h.lib

        def refused(rc, who):
            assert rc == -1 and who.encode() + b":" in lib.nsk_last_error(), (rc, lib.nsk_last_error())

        # no prior init
        refused(lib.nsk_boostconv_core(h.ctx, a), "nsk_boostconv_core")
        refused(lib.nsk_boostconv_map(h.ctx, a, b, 1, 0, rp, C.byref(nc)), "nsk_boostconv_map")
        refused(lib.nsk_boostconv_rewind(h.ctx), "nsk_boostconv_rewind")
        for snp in (0, 17, -1):
            refused(lib.nsk_boostconv_init(h.ctx, snp), "nsk_boostconv_init")
        refused(lib.nsk_boostconv_init(None, 3), "nsk_boostconv_init")
        h.boostconv_init(3)
        refused(lib.nsk_boostconv_rewind(h.ctx), "nsk_boostconv_rewind")            # no map yet
        refused(lib.nsk_boostconv_core(h.ctx, None), "nsk_boostconv_core")
        for f, q, skip, step0 in [(a, a, 1, 0), (None, b, 1, 0), (a, None, 1, 0), (a, b, 0, 0), (a, b, -2, 0), (a, b, 1, -1)]:
            refused(lib.nsk_boostconv_map(h.ctx, f, q, skip, step0, rp, C.byref(nc)), "nsk_boostconv_map")
        refused(lib.nsk_boostconv_map(None, a, b, 1, 0, rp, C.byref(nc)), "nsk_boostconv_map")
        with pytest.raises(NskError) as e:
            h.boostconv_map(a, a, 1, 0)
        assert e.value.code == -1 and "nsk_boostconv_map" in str(e.value)
        # a lane
        h.add_lane()
        refused(lib.nsk_boostconv_init(h._lanes[1], 3), "nsk_boostconv_init")
        refused(lib.nsk_boostconv_core(h._lanes[1], a), "nsk_boostconv_core")
        refused(lib.nsk_boostconv_map(h._lanes[1], a, b, 1, 0, rp, C.byref(nc)), "nsk_boostconv_map")
        # shards: the single-rank entries refuse them, the group entries refuse everything else
        g = ShardGroup(h, case, 2)
        try:
            x, y = g.alloc(2)
            refused(lib.nsk_boostconv_init(g.ctx[0], 3), "nsk_boostconv_init")
            refused(lib.nsk_boostconv_core(g.ctx[0], x.parts[0]), "nsk_boostconv_core")
            refused(lib.nsk_boostconv_map(g.ctx[0], x.parts[0], y.parts[0], 1, 0, rp, C.byref(nc)), "nsk_boostconv_map")
            one = lambda v: (C.c_void_p * 1)(v.value)
            refused(lib.nsk_group_boostconv_init(one(h.ctx), 1, 3), "nsk_group_boostconv_init")
            refused(lib.nsk_group_boostconv_map(one(h.ctx), 1, one(a), one(b), 1, 0, rp, C.byref(nc)), "nsk_group_boostconv_map")
            pr = g._per_rank
            refused(lib.nsk_group_boostconv_map(g._arr, 2, pr(x), pr(y), 1, 0, rp, C.byref(nc)), "nsk_group_boostconv_map")      # no init
            refused(lib.nsk_group_boostconv_init(g._arr, 2, 17), "nsk_group_boostconv_init")
            g.boostconv_init(2)
            refused(lib.nsk_group_boostconv_map(g._arr, 2, pr(x), pr(x), 1, 0, rp, C.byref(nc)), "nsk_group_boostconv_map")
            refused(lib.nsk_group_boostconv_map(g._arr, 2, pr(x), None, 1, 0, rp, C.byref(nc)), "nsk_group_boostconv_map")
            refused(lib.nsk_group_boostconv_map(g._arr, 2, pr(x), pr(y), 0, 0, rp, C.byref(nc)), "nsk_group_boostconv_map")
            refused(lib.nsk_group_boostconv_map(g._arr, 2, pr(x), pr(y), 1, -1, rp, C.byref(nc)), "nsk_group_boostconv_map")
            refused(lib.nsk_group_boostconv_core(g._arr, 2, None), "nsk_group_boostconv_core")
            refused(lib.nsk_group_boostconv_map(None, 2, pr(x), pr(y), 1, 0, rp, C.byref(nc)), "nsk_group_boostconv_map")
            g.free([x, y])
        finally:
            g.close()
        h.free([a, b])
    finally:
        h.close()


def test_rank_local_contexts_are_refused():
    from nekstab_amd.sharded import local_parents
    from tests import sym_box
    from tests.test_sfd_gpu import KW
    c, _ = sym_box.case(6, False)
    parents, _ = local_parents(c, 2, **KW)
    try:
        p = parents[0]
        rc = p.lib.nsk_boostconv_init(p.ctx, 3)
        assert rc == -1 and b"nsk_boostconv_init:" in p.lib.nsk_last_error()
    finally:
        for p in parents:
            p.close()


# ---- 7. the driver -------------------------------------------------------------------------------------------------------------
def test_driver_writes_the_reference_files(cyl, tmp_path):
    """A run from the perturbed start with snp = 3, skip = 10, stopped by a tolerance put between the smallest and the second
    smallest residual of the first map's calls: the driver finds that call, cuts the map there and writes the files."""
    from nekstab_amd import fixedp, nekio
    case, _ = cyl
    h = _context(case)
    try:
        h.set_option("proj_reset", 1)       # (so that the driver's maps repeat the first map of this test to the bit)
        _driver(h, case, str(tmp_path), fixedp, nekio)
    finally:
        h.close()


def _driver(h, case, out, fixedp, nekio):
    q = _perturbed(case)
    vq, vf, vw = h.alloc(3)
    h.upload(vq, *q)
    h.set_baseflow(vq)
    n = h.nsteps
    h.boostconv_init(3)
    first = h.boostconv_map(vf, vq, 10, 0)
    at = [0] + list(range(10, n + 1, 10))
    assert len(first) == len(at)
    order = np.argsort(first[1:])
    k, k2 = 1 + order[0], 1 + order[1]
    print("first map: nsteps %d, residu" % n, first, "-> stop at call", k, "step", at[k])
    assert first[k2] / first[k] > 1.05
    tol = float(np.sqrt(first[k] * first[k2]))
    ok, steps, hist = fixedp.boostconv(h, vq, snp=3, skip=10, tol=tol, max_time=50.0, outdir=out, ifvor=True)
    assert ok and steps == at[k] and len(hist) == k + 1 and hist[-1] < tol and np.all(hist[1:-1] >= tol) and h.nsteps == n
    assert np.allclose(hist, first[:k + 1], rtol=1e-12)
    rows = open(os.path.join(out, "residu.dat")).read().splitlines()
    assert len(rows) == k + 1 and all(re.fullmatch(r"( [ -]0\.\d{7}E[+-]\d\d){3}", r) for r in rows)
    t = np.loadtxt(os.path.join(out, "residu.dat"))
    assert np.allclose(t[:, 1], hist, rtol=1e-6) and np.allclose(t[:, 0], h.dt * np.array(at[:k + 1]), rtol=1e-6, atol=1e-12)
    prev = np.concatenate([[0.0], hist[:-1]])
    assert np.allclose(t[:, 2], (hist - prev) / h.dt, rtol=1e-5, atol=1e-7 * np.abs(hist).max() / h.dt)
    got = h.download(vq)
    bf = nekio.read_fld(os.path.join(out, "BF_1cyl0.f00001"))
    assert bf.wdsize == 8 and bf.istep == steps and np.array_equal(bf.u[0, :, 0], got[0]) and np.array_equal(bf.u[1, :, 0], got[1])
    h.vorticity(vw, vq)
    w = h.download(vw)
    bfv = nekio.read_fld(os.path.join(out, "BFV1cyl0.f00001"))
    assert bfv.p is None and np.array_equal(bfv.u[0, :, 0], w[0].astype(np.float32).astype(np.float64)) and np.abs(w[0]).max() > 0
    h.free([vq, vf, vw])


def test_driver_takes_a_shard_group(tmp_path):
    """fixedp.boostconv on 2 virtual ranks of the channel (lx1 = 8) and on the single rank with `tol` above every residual:
    both stop at the first call behind a step, step `skip` = 2, where the map is cut; residu within the sharded bound."""
    from nekstab_amd import fixedp, nekio
    from nekstab_amd.sharded import ShardGroup
    c, q, w2, h = _channel(8, 2)
    try:
        runs = {}
        g = ShardGroup(h, c, 2)
        try:
            for name, be in (("one", h), ("two", g)):
                vq, = be.alloc(1)
                be.upload(vq, *q)
                out = os.path.join(str(tmp_path), name)
                ok, steps, hist = fixedp.boostconv(be, vq, snp=SNP, skip=SKIP, tol=1e300, max_time=1e9, outdir=out)
                runs[name] = (ok, steps, hist, be.download(vq), out)
                be.free([vq])
        finally:
            g.close()
    finally:
        h.close()
    for ok, steps, hist, got, out in runs.values():
        assert ok and steps == SKIP and len(hist) == 2 and len(open(os.path.join(out, "residu.dat")).read().splitlines()) == 2
        bf = nekio.read_fld(os.path.join(out, "BF_1cyl0.f00001"))
        assert bf.wdsize == 8 and np.array_equal(bf.u[0, :, 0], got[0]) and np.array_equal(bf.u[1, :, 0], got[1])
    bound = 10.0 * _channel_S(8) * SHARD_MEASURED[(2, 8, 2)]
    er = float(np.abs(runs["two"][2] / runs["one"][2] - 1.0).max())
    print("fixedp.boostconv, 2 virtual ranks vs one: residu %.2e (bound %.2e)" % (er, bound))
    assert er <= bound
