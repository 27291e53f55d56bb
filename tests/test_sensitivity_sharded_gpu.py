"""Eigenmode post-processing on element shards (nsk_group_biorthogonalize, nsk_group_wavemaker, nsk_group_bf_sensitivity,
nsk_group_energy_budget, nsk_group_forced_map; uparam(1) = 4.x under the element decomposition) against the numpy restatement
on the WHOLE mesh (nekstab_amd/sensitivity.py), the reference the single-rank tests use, at their bounds: relative L2 error
<= 1e-12 per field, integrals within 1e-12 of their largest magnitude, gamma and delta to 1e-12 relative.  Sharding changes
only the order in which the at most valence-many copies of a node are added inside a dsavg (local partial sum + the peers'
partial sums), far inside those bounds; a wrong ghost slot, stride or multiplicity is far outside them.

Full-mesh contexts and references are built once per module and shared; the groups are cut per test (cheap)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from nekstab_amd import mesh, mesh3d, nekio
from nekstab_amd import sensitivity as S
from nekstab_amd.capi import NSK_ADJOINT, NSK_DIRECT, NekStabHip, NskError
from nekstab_amd.sharded import ShardGroup, local_parents, partition_rcb, shard_halo_counts
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
# the tolerances of tests/test_sharded_gpu.py::test_sharded_matvec_equals_single_rank (the post-processing does not read them).
# Its iteration caps (120 / 48) are doubled: under the committed force the SINGLE-RANK forced map, the yardstick of the forced
# sharded maps, ends one solve at the cap of 48 and returns NSK_ENOCONV; the caps bound work, not accuracy.
KW = dict(tol_helm=1e-12, tol_pres=1e-6, tol_relative=1, schwarz_layers=2, max_helm_iter=240, max_pres_iter=96)
KW3 = dict(tol_helm=1e-12, tol_pres=1e-7, tol_relative=1, max_helm_iter=200, max_pres_iter=48)
UBF = lambda x, y, z: np.stack([1.0 - 0.3 * y * y + 0.1 * np.sin(x + z), 0.2 * np.cos(x) * y + 0.1 * z, 0.15 * np.sin(y + 0.5 * z)])
# the budget's base flow: the one of tests/test_energy_budget_gpu.py::test_hexahedra_genuinely_3d_field_matches_numpy (every
# derivative non-zero: with UBF, d U_z / d x = 0 and P[3][1] would be compared against rounding noise)
UBF_BUDGET = lambda x, y, z: np.stack([1.0 - 0.3 * y * y + 0.1 * np.sin(x + z), 0.2 * np.cos(x) * y + 0.1 * z,
                                       0.15 * np.sin(y + 0.5 * z + 0.4 * x)])
_CACHE = {}


def _rel(a, b):
    return np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b))


def _smooth_modes(c):
    """the analytic modes of tests/test_sensitivity_gpu.py::test_hexahedra_genuinely_3d_field_matches_numpy"""
    x, y, z = c.x, c.y, c.z
    f = lambda a, b, cc, d: np.sin(a * x + 0.3) * np.cos(b * y - 0.2) * np.exp(cc * z) + d * x * y * z
    return [np.array([f(1.1, 0.7, 0.3, 0.2), f(0.5, 1.3, -0.4, 0.1), f(0.9, 0.4, 0.8, -0.3)]),
            np.array([f(0.6, 1.0, 0.5, 0.0), f(1.4, 0.2, 0.1, 0.4), f(0.3, 0.9, -0.6, 0.2)]),
            np.array([f(0.8, 0.5, -0.2, 0.3), f(0.2, 1.1, 0.7, -0.1), f(1.2, 0.6, 0.4, 0.0)]),
            np.array([f(1.3, 0.3, 0.6, -0.2), f(0.7, 0.8, -0.5, 0.3), f(0.4, 1.2, 0.2, 0.1)])]


class Setup:
    """One case: its full-mesh context, the raw modes, the base flow and the numpy references (computed once, read only)."""

    def __init__(self, name):
        if name.startswith("cyl"):
            lx1 = int(name[3:])
            self.case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), lx1)
            m = np.load(os.path.join(GOLDEN, "cylinder_modes.npz"))
            self.raw = [S.interp_gll(m[k + "_u"].astype(np.float64), lx1) for k in ("dRe", "dIm", "aRe", "aIm")]
            self.ub = np.asarray(self.case.ub, dtype=np.float64)
            self.h = NekStabHip(self.case, self.case.meta["vert"], self.case.meta["nvert"], **KW)
        else:
            shape = (4, 3, 2, 6, 0.05) if name == "box6" else (2, 2, 2, 10, 0.06)
            self.case = mesh3d.box_case_3d(*shape[:4], lengths=(2.0, 1.0, 0.8), outflow_xmax=True, re=40.0, endtime=0.05, ub_func=UBF,
                                           warp=shape[4])
            self.raw = _smooth_modes(self.case)
            self.ub = UBF_BUDGET(self.case.x, self.case.y, self.case.z)
            self.h = NekStabHip(self.case, self.case.meta["vert"], self.case.meta["nvert"], **KW3)
        self.geom = S.NpGeom(self.case)
        self._ref = {}

    def ref(self, what):
        g = self.geom
        if what not in self._ref:
            if what == "bio":
                self._ref[what] = S.np_biorthogonalize(g, *self.raw)
            elif what == "sens":
                self._ref[what] = S.np_bf_sensitivity(g, *self.ref("bio")[:4])
            elif what == "budget":
                self._ref[what] = S.np_energy_budget(g, self.ub, self.raw[0], self.raw[1], 1.0 / self.case.re)
        return self._ref[what]


@pytest.fixture(scope="module")
def setups():
    def get(name):
        if name not in _CACHE:
            _CACHE[name] = Setup(name)
        return _CACHE[name]
    yield get
    for s in _CACHE.values():
        s.h.close()
    _CACHE.clear()


def _upload(h, fields):
    vecs = h.alloc(len(fields))
    for v, u in zip(vecs, fields):
        S.upload_velocity(h, v, u)
    return vecs


def _all(h, v):
    return h.download3(v) if h.ndim == 3 else h.download(v)


def _check_sens(g, st, parts=True):
    """bf_sensitivity of the biorthogonalised modes on the group g against numpy; returns the downloaded fields."""
    ref = st.ref("sens")
    v = _upload(g, st.ref("bio")[:4])
    outs = g.alloc(6)
    try:
        g.bf_sensitivity(*v, outs[0], outs[1], parts=outs[2:] if parts else None)
        got = {k: S.download_velocity(g, o) for k, o in zip(("sr", "si", "tr", "ti", "pr", "pi"), outs[:6 if parts else 2])}
        for k in got:
            err = _rel(got[k], ref[k])
            print(f"{k}: relative L2 error against numpy {err:.2e}")
            assert err <= 1e-12, k
        assert not np.any(_all(g, outs[0])[g.ndim]) and not np.any(_all(g, outs[1])[g.ndim])      # pressure of the outputs: 0
    finally:
        g.free(v + outs)
    return got


def _check_budget(g, st):
    """energy_budget with every output on the group g against numpy; inputs keep their bits; returns (integrals, prod, diss)."""
    ref, nd = st.ref("budget"), g.ndim
    v = _upload(g, (st.ub, st.raw[0], st.raw[1]))
    outs = g.alloc(nd + 1)
    try:
        before = [_all(g, a) for a in v]
        I = g.energy_budget(*v, prod=outs[:nd], diss=outs[nd])
        for x0, x1 in zip(before, [_all(g, a) for a in v]):
            for a0, a1 in zip(x0, x1):
                assert np.array_equal(a0, a1)
        prod = np.array([S.download_velocity(g, o) for o in outs[:nd]])
        dv = _all(g, outs[nd])
        rest = [np.asarray(a) for a in dv[1:]] + [_all(g, o)[nd] for o in outs[:nd]]
        for c in range(nd):
            for j in range(nd):
                assert _rel(prod[c, j], ref["prod"][c, j]) <= 1e-12, (c, j)
        err = _rel(dv[0], ref["diss"])
        dI = np.max(np.abs(I - ref["integrals"])) / np.max(np.abs(ref["integrals"]))
        print(f"dissipation field: relative L2 error {err:.2e}; integrals: {dI:.2e} of the largest")
        assert err <= 1e-12
        assert dI <= 1e-12, (I, ref["integrals"])
        assert all(not np.any(a) for a in rest)                                     # pressure and unused components: 0
        np.testing.assert_array_equal(g.energy_budget(*v), I)                       # no field outputs: the same sums
    finally:
        g.free(v + outs)
    return I, prod, np.asarray(dv[0])


# ---- 1. cylinder fixture ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lx1,nranks", [(6, 2), (6, 4), (8, 2)])
def test_cylinder_postprocessing_matches_numpy(setups, lx1, nranks):
    st = setups("cyl%d" % lx1)
    case = st.case
    part = partition_rcb(case, nranks)
    g = ShardGroup(st.h, case, nranks, part)
    try:
        halo = [shard_halo_counts(g.lib, c, nranks)[0] for c in g.ctx]
        assert all(h.sum() > 0 for h in halo), halo                                 # every rank exchanges a velocity halo
        if nranks == 4:                                                             # ... and one node lives on three ranks
            gid = np.asarray(case.gid).reshape(case.nel, -1)
            own = np.zeros((int(case.nglob), nranks), dtype=bool)
            for r in range(nranks):
                own[np.unique(gid[part == r]), r] = True
            assert np.sum(own.sum(axis=1) >= 3) >= 1
        # biorthogonalize: gamma, delta and the four modes
        ref = st.ref("bio")
        v = _upload(g, st.raw)
        wm = g.alloc(1)[0]
        try:
            gamma, delta = g.biorthogonalize(*v)
            assert abs(gamma - ref[4]) <= 1e-12 * abs(ref[4]) and abs(delta - ref[5]) <= 1e-12 * abs(ref[5]), (gamma, delta, ref[4:])
            for k, vec in enumerate(v):
                assert _rel(S.download_velocity(g, vec), ref[k]) <= 1e-12, k
            dRe, dIm, aRe, aIm = v
            assert abs(g.dot(aRe, dRe) + g.dot(aIm, dIm) - 1.0) <= 1e-12 and abs(g.dot(aRe, dIm) - g.dot(aIm, dRe)) <= 1e-12
            g.wavemaker(*v, wm)
            w = _all(g, wm)
            assert _rel(w[0], S.np_wavemaker(*ref[:4])) <= 1e-12 and not np.any(w[1]) and not np.any(w[2])
        finally:
            g.free(v + [wm])
        got = _check_sens(g, st, parts=True)
        assert np.array_equal(got["sr"], got["tr"] + got["pr"]) and np.array_equal(got["si"], got["ti"] + got["pi"])
        got2 = _check_sens(g, st, parts=False)
        assert _rel(got2["sr"], got["sr"]) <= 1e-13 and _rel(got2["si"], got["si"]) <= 1e-13
        I, _, _ = _check_budget(g, st)
        assert np.all(I[[2, 5, 6, 7, 8]] == 0.0)
    finally:
        g.close()


# ---- 2. / 3. hexahedra -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nranks", [2, 3])
def test_deformed_box_matches_numpy(setups, nranks):
    """3 ranks: 12 nodes on three ranks and 6 interface nodes of valence > 4 (the CSR branch of the gather)."""
    st = setups("box6")
    g = ShardGroup(st.h, st.case, nranks)
    try:
        halo = [shard_halo_counts(g.lib, c, nranks)[0] for c in g.ctx]
        assert all(h.sum() > 0 for h in halo), halo
        _check_sens(g, st)
        I, _, _ = _check_budget(g, st)
        assert np.min(np.abs(I)) > 0.0
    finally:
        g.close()


def test_box_lx10_budget_matches_numpy(setups):
    """the <10, 3> instantiations (launch shape of their own)"""
    st = setups("box10")
    g = ShardGroup(st.h, st.case, 2)
    try:
        _check_budget(g, st)
    finally:
        g.close()


# ---- 4. rank-local parents, released parents -------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["local", "released"])
def test_local_and_released_parents(setups, how):
    st = setups("cyl6")
    case = st.case
    if how == "local":
        parents, part = local_parents(case, 2, **KW)
        g = ShardGroup(parents, case, 2, part)
    else:
        parents = [NekStabHip(case, case.meta["vert"], case.meta["nvert"], **KW)]
        g = ShardGroup(parents[0], case, 2)
        g.release_parent()
    try:
        _check_sens(g, st)
        I1, p1, d1 = _check_budget(g, st)
        I2, p2, d2 = _check_budget(g, st)
        np.testing.assert_array_equal(I1, I2)                                       # two calls: the same bits
        assert np.array_equal(p1, p2) and np.array_equal(d1, d2)
    finally:
        g.close()
        for p in parents:
            p.close()


# ---- 5. forced maps --------------------------------------------------------------------------------------------------

def _force6():
    return np.load(os.path.join(GOLDEN, "cylinder_bf_sensitivity.npz"))["sr_u"].astype(np.float64)


def _flat(g, v):
    return np.concatenate([np.ravel(a) for a in _all(g, v)])


def test_forced_map_with_zero_force_is_the_eager_map(setups):
    """Three fresh groups with the same history: eager matvec, forced map with force = 0, graph-replayed matvec; direct then adjoint."""
    st = setups("cyl6")
    q = st.raw[0] * st.case.mask
    res = {}
    for kind in ("eager", "forced", "graph"):
        g = ShardGroup(st.h, st.case, 2)
        try:
            g.set_nsteps(4)
            if kind == "eager":
                g.set_option("shard_graph", 0)
            a, b, z = g.alloc(3)
            S.upload_velocity(g, a, q)
            g.zero(z)
            out = []
            for mode in (NSK_DIRECT, NSK_ADJOINT):
                if kind == "forced":
                    g.forced_map(b, a, z, mode)
                else:
                    g.matvec(b, a, mode)
                out.append(_flat(g, b))
            res[kind] = out
        finally:
            g.close()
    for k in range(2):
        assert np.array_equal(res["eager"][k], res["forced"][k]), k
        assert np.array_equal(res["graph"][k], res["forced"][k]), k


def test_forced_map_equals_single_rank_and_leaves_the_graphs(setups):
    st = setups("cyl6")
    h, case = st.h, st.case
    q, f = st.raw[0] * case.mask, _force6()
    w = st.geom.bm1
    nsteps = h.nsteps
    h.set_nsteps(4)
    g = ShardGroup(h, case, 2)
    hv = _upload(h, (q, f)) + h.alloc(2)
    gv = _upload(g, (q, f)) + g.alloc(3)
    try:
        g.set_nsteps(4)
        g.zero(gv[3])
        g.matvec(gv[4], gv[0], NSK_DIRECT)
        plain = _flat(g, gv[4])
        st0 = g.stats()
        for mode in (NSK_DIRECT, NSK_ADJOINT):
            h.forced_map(hv[2], hv[0], hv[1], mode)
            g.forced_map(gv[2], gv[0], gv[1], mode)
            ref, got = h.download(hv[2]), g.download(gv[2])
            num = np.sqrt(sum(np.sum(w * (a - b) ** 2) for a, b in zip(got[:2], ref[:2])))
            den = np.sqrt(sum(np.sum(w * b ** 2) for b in ref[:2]))
            perr = np.abs(got[2] - ref[2]).max() / np.abs(ref[2]).max()
            print(f"mode {mode}: forced map on 2 ranks against the single-rank one: velocity {num / den:.2e}, pressure {perr:.2e}")
            assert num / den < 1e-9 and perr < 1e-5
            h.matvec(hv[3], hv[0], mode)
            assert _rel(S.download_velocity(h, hv[3]), S.download_velocity(h, hv[2])) > 1e-6      # the force acts
        g.forced_map(gv[2], gv[3], gv[1], NSK_ADJOINT)                              # q = 0: the force alone, on every rank
        u0 = S.download_velocity(g, gv[2])
        assert all(np.any(u0[:, e]) for e in g.elems)
        st1 = g.stats()
        for k in ("recaptures", "budget_helm", "budget_pres"):                      # graphs and budgets of the unforced maps: untouched
            assert st0[k] == st1[k], (k, st0[k], st1[k])
        g.matvec(gv[4], gv[0], NSK_DIRECT)
        assert np.array_equal(_flat(g, gv[4]), plain)
        for bad in (2, 3, 4, -1, 9):
            with pytest.raises(NskError) as e:
                g.forced_map(gv[2], gv[0], gv[1], bad)
            assert e.value.code == -1 and "mode" in str(e.value)
        with pytest.raises(NskError) as e:
            g.forced_map(gv[1], gv[0], gv[1], NSK_ADJOINT)                          # force == f
        assert e.value.code == -1 and "force" in str(e.value)
    finally:
        g.close()
        h.free(hv)
        h.set_nsteps(nsteps)


def test_forced_map_on_the_box_equals_single_rank(setups):
    st = setups("box6")
    h, c = st.h, st.case
    x, y, z = c.x, c.y, c.z
    q = np.array([np.sin(1.3 * x + z) * np.cos(2.0 * y) * c.mask, np.cos(0.7 * x + 0.2) * np.sin(3.0 * y - z) * c.mask,
                  np.sin(x + y) * np.cos(2.0 * z) * c.mask])
    f = st.raw[2] * c.mask
    nsteps = h.nsteps
    h.set_nsteps(4)
    g = ShardGroup(h, c, 2)
    hv = _upload(h, (q, f)) + h.alloc(1)
    try:
        g.set_nsteps(4)
        gv = _upload(g, (q, f)) + g.alloc(1)
        h.forced_map(hv[2], hv[0], hv[1], NSK_DIRECT)
        g.forced_map(gv[2], gv[0], gv[1], NSK_DIRECT)
        ref, got = h.download3(hv[2]), g.download3(gv[2])
        sc = max(np.abs(ref[k]).max() for k in range(3))
        for k in range(3):
            assert np.abs(got[k] - ref[k]).max() < 1e-8 * sc
        assert np.abs(got[3] - ref[3]).max() < 1e-4 * np.abs(ref[3]).max()
    finally:
        g.close()
        h.free(hv)
        h.set_nsteps(nsteps)


# ---- 6. drivers ------------------------------------------------------------------------------------------------------

def test_postprocess_driver_writes_the_single_rank_files(setups, tmp_path):
    st = setups("cyl6")
    h = st.h
    g = ShardGroup(h, st.case, 2)
    d1, d2 = tmp_path / "single", tmp_path / "sharded"
    d1.mkdir(); d2.mkdir()
    hv, gv = _upload(h, [st.ub] + st.raw), _upload(g, [st.ub] + st.raw)
    try:
        o1 = S.postprocess(h, *hv, outdir=str(d1), session="1cyl")
        o2 = S.postprocess(g, *gv, outdir=str(d2), session="1cyl")
        for vec, u in zip(gv, [st.ub] + st.raw):                                    # the caller's vectors are left as they are
            np.testing.assert_array_equal(S.download_velocity(g, vec), u)
    finally:
        h.free(hv)
        g.close()
    names = sorted(os.listdir(d1))
    assert names == sorted(os.listdir(d2)) and len(names) == 9, (names, sorted(os.listdir(d2)))
    for nm in names:
        a, b = nekio.read_fld(str(d1 / nm)), nekio.read_fld(str(d2 / nm))
        np.testing.assert_array_equal(a.x, b.x)
        fa, fb = (a.t, b.t) if nm.startswith("wm_") else (a.u, b.u)
        assert fa.shape == fb.shape and _rel(fb, fa) <= 1e-12, nm
    assert np.max(np.abs(o1["integrals"] - o2["integrals"])) <= 1e-12 * np.max(np.abs(o1["integrals"]))
    assert abs(o1["gamma_delta"][0] - o2["gamma_delta"][0]) <= 1e-12 * abs(o1["gamma_delta"][0])


# ---- 7. refusals -----------------------------------------------------------------------------------------------------

def test_refusals(setups):
    st = setups("cyl6")
    h, lib = st.h, st.h.lib
    ints = np.zeros(10)
    dp = C.POINTER(C.c_double)
    a = h.alloc(5)
    one = lambda v: (C.c_void_p * 1)(v.value)
    ctx = (C.c_void_p * 1)(h.ctx.value)
    try:                                                                            # a full-mesh context is no shard
        calls = [lambda: lib.nsk_group_biorthogonalize(ctx, 1, one(a[0]), one(a[1]), one(a[2]), one(a[3]), None),
                 lambda: lib.nsk_group_wavemaker(ctx, 1, one(a[0]), one(a[1]), one(a[2]), one(a[3]), one(a[4])),
                 lambda: lib.nsk_group_bf_sensitivity(ctx, 1, one(a[0]), one(a[1]), one(a[2]), one(a[3]), one(a[4]), one(a[4]), None),
                 lambda: lib.nsk_group_energy_budget(ctx, 1, one(a[0]), one(a[1]), one(a[2]), None, None, ints.ctypes.data_as(dp)),
                 lambda: lib.nsk_group_forced_map(ctx, 1, NSK_ADJOINT, one(a[0]), one(a[1]), one(a[2]))]
        for call in calls:
            assert call() == -1
            assert b"needs shard contexts" in lib.nsk_last_error()
    finally:
        h.free(a)
    g = ShardGroup(h, st.case, 2)
    try:
        ub, dRe, dIm, aRe, aIm = _upload(g, [st.ub] + st.raw)
        o1, o2, o3, o4, z1, z2 = g.alloc(6)
        g.zero(z1); g.zero(z2)
        bad = [lambda: g.biorthogonalize(dRe, dRe, aRe, aIm),
               lambda: g.wavemaker(dRe, dIm, aRe, aIm, aIm),
               lambda: g.bf_sensitivity(dRe, dIm, aRe, aIm, o1, o1),
               lambda: g.bf_sensitivity(dRe, dIm, aRe, aIm, o1, dRe),
               lambda: g.bf_sensitivity(dRe, dIm, aRe, aIm, o1, o2, parts=[o3, o4, o3, z1]),
               lambda: g.energy_budget(ub, dRe, dIm, prod=[o1, o1]),
               lambda: g.energy_budget(ub, dRe, dIm, prod=[o1, o2], diss=o1),
               lambda: g.energy_budget(ub, dRe, dIm, prod=[o1, ub]),
               lambda: g.energy_budget(ub, dRe, dIm, diss=dIm)]
        for call in bad:
            with pytest.raises(NskError) as e:
                call()
            assert e.value.code == -1 and len(str(e.value)) > 30
        for call in (lambda: g.biorthogonalize(z1, z2, aRe, aIm), lambda: g.energy_budget(ub, z1, z2)):
            with pytest.raises(NskError) as e:
                call()
            assert e.value.code == -1 and "zero" in str(e.value)
        np.testing.assert_array_equal(S.download_velocity(g, dRe), st.raw[0])      # refused calls wrote nothing
        np.testing.assert_array_equal(S.download_velocity(g, aIm), st.raw[3])
    finally:
        g.close()


# ---- 8. two processes ------------------------------------------------------------------------------------------------

def test_postprocessing_across_two_processes():
    """Two ranks, one process each, sharing this GPU; halos and sums over gloo on the host (nsk_comm_init_host): rank-local
    set-up, released parents, bf_sensitivity and energy_budget of the cylinder at lx1 = 6 against numpy on every rank."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29681", os.path.join(ROOT, "tests", "mp_sens_worker.py")],
                         capture_output=True, text=True, timeout=600, env=env)
    line = [l for l in out.stdout.splitlines() if "MPSENS" in l]
    print(line, out.stderr[-1500:] if out.returncode else "")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count("MPSENS rank") == 2                                     # (the two ranks' lines may share one line of the pipe)
