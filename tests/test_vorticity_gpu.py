"""Vorticity of eigenmodes on the device (nsk_vorticity, nsk_group_vorticity: comp_vort3 as outpost_ks calls it for its Rv
files) against the numpy restatement sensitivity.np_vorticity (relative L2 error <= 1e-12, the bound of
tests/test_sensitivity_gpu.py for device against numpy) and against the reference's own dRv file (bm1-weighted relative L2
<= 1e-5: the two fp32 files leave 2.1e-6, the nearest wrong averaging convention 4.6e-5; tests/test_vorticity_host.py).

The cylinder context at lx1 = 6, its shard groups' parent, and the numpy references are built once per module."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from nekstab_amd import krylov, mesh, mesh3d, nekio, outpost
from nekstab_amd import sensitivity as S
from nekstab_amd.capi import NekStabHip, NskError
from nekstab_amd.sharded import ShardGroup, local_parents, shard_halo_counts
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
KW = dict(tol_helm=1e-12, tol_pres=1e-6, tol_relative=1, schwarz_layers=2, max_helm_iter=240, max_pres_iter=96)
KW3 = dict(tol_helm=1e-12, tol_pres=1e-7, tol_relative=1, max_helm_iter=200, max_pres_iter=48)
UBF = lambda x, y, z: np.stack([1.0 - 0.3 * y * y + 0.1 * np.sin(x + z), 0.2 * np.cos(x) * y + 0.1 * z, 0.15 * np.sin(y + 0.5 * z)])
_CACHE = {}


def _rel(a, b):
    return np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b))


def _cyl_case(lx1):
    return mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), lx1)


def _cyl_mode(lx1):
    """the reference's leading direct mode (real part), brought to lx1 by interp_gll"""
    return S.interp_gll(np.load(os.path.join(GOLDEN, "cylinder_modes.npz"))["dRe_u"].astype(np.float64), lx1)


def _box(name):
    shape = {"box6": (4, 3, 2, 6, 0.05), "box8": (4, 3, 2, 8, 0.05), "box10": (2, 2, 2, 10, 0.06)}[name]
    return mesh3d.box_case_3d(*shape[:4], lengths=(2.0, 1.0, 0.8), outflow_xmax=True, re=40.0, endtime=0.05, ub_func=UBF, warp=shape[4])


def _smooth_mode(c):
    """the first of the analytic modes of tests/test_sensitivity_sharded_gpu.py (every derivative non-zero)"""
    x, y, z = c.x, c.y, c.z
    f = lambda a, b, cc, d: np.sin(a * x + 0.3) * np.cos(b * y - 0.2) * np.exp(cc * z) + d * x * y * z
    return np.array([f(1.1, 0.7, 0.3, 0.2), f(0.5, 1.3, -0.4, 0.1), f(0.9, 0.4, 0.8, -0.3)])


class Setup:
    """One case: its full-mesh context, the mode and the numpy vorticity of the WHOLE mesh (computed once, read only)."""

    def __init__(self, name):
        if name == "cyl6":
            self.case, self.u = _cyl_case(6), _cyl_mode(6)
            self.h = NekStabHip(self.case, self.case.meta["vert"], self.case.meta["nvert"], **KW)
        else:
            self.case = _box(name)
            self.u = _smooth_mode(self.case)
            self.h = NekStabHip(self.case, self.case.meta["vert"], self.case.meta["nvert"], **KW3)
        self.geom = S.NpGeom(self.case)
        self.ref = S.np_vorticity(self.geom, self.u)
        self.ref.setflags(write=False)


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


def _all(h, v):
    return h.download3(v) if h.ndim == 3 else h.download(v)


def _vorticity(h, u):
    """upload u, run the device entry, return every downloaded slot of the output (velocity components, pressure)"""
    q, w = h.alloc(2)
    try:
        S.upload_velocity(h, q, u)
        h.vorticity(w, q)
        return [np.array(a) for a in _all(h, w)]
    finally:
        h.free([q, w])


# ---- 4. cylinder at lx1 = 6, the reference's mode ------------------------------------------------------------------

def test_cylinder_lx6_matches_numpy_and_the_reference_file(setups):
    """A context that carries one scalar field (theta), so that every kind of slot of the output is there to be zeroed; the
    output vector is filled with non-zero values first."""
    st = setups("cyl6")
    case, g, u = st.case, st.geom, st.u
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **KW)
    try:
        h.set_nscal(1)
        q, w, w2 = h.alloc(3)
        rng = np.random.default_rng(5)
        pr, th = rng.standard_normal((case.nel, 4, 4)), rng.standard_normal(case.x.shape)
        h.upload(q, u[0], u[1], pr)
        h.upload_scalar(q, 0, th)
        for o in (w, w2):
            h.upload(o, th, th + 1.0, pr + 2.0)
            h.upload_scalar(o, 0, th - 3.0)
        before = [np.array(a) for a in h.download(q)] + [h.download_scalar(q, 0)]
        h.vorticity(w, q)
        after = [np.array(a) for a in h.download(q)] + [h.download_scalar(q, 0)]
        for a, b in zip(before, after):
            assert np.array_equal(a, b)                                             # q is read only
        wx, wy, wp = h.download(w)
        wt = h.download_scalar(w, 0)
        err = _rel(wx, st.ref[0])
        fx = np.load(os.path.join(GOLDEN, "cylinder_vorticity.npz"))["w"].astype(np.float64)
        errf = np.sqrt(np.sum(g.bm1 * (wx - fx) ** 2) / np.sum(g.bm1 * fx ** 2))
        print(f"device against numpy: {err:.2e}; against the reference's dRv file (weighted L2): {errf:.3e}")
        assert err <= 1e-12
        assert errf <= 1e-5
        assert not np.any(wy) and not np.any(wp) and not np.any(wt)                 # exactly zero
        wall = case.mask == 0.0                                                     # no Dirichlet mask: the walls keep their vorticity
        assert np.any(st.ref[0][wall]) and _rel(wx[wall], st.ref[0][wall]) <= 1e-12
        h.vorticity(w2, q)
        assert np.array_equal(h.download(w2)[0], wx) and not np.any(h.download(w2)[1])     # a second call: the same bits
    finally:
        h.close()


# ---- 5. quadrilaterals at lx1 = 8, 10, 12 --------------------------------------------------------------------------

@pytest.mark.parametrize("lx1", [8, 10, 12])
def test_quadrilaterals_match_numpy(lx1):
    case, u = _cyl_case(lx1), _cyl_mode(lx1)
    ref = S.np_vorticity(S.NpGeom(case), u)
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **KW)
    try:
        wx, wy, wp = _vorticity(h, u)
        err = _rel(wx, ref[0])
        print(f"lx1 = {lx1}: device against numpy {err:.2e}")
        assert err <= 1e-12
        assert not np.any(wy) and not np.any(wp)
    finally:
        h.close()


# ---- 6. hexahedra, z-invariant -------------------------------------------------------------------------------------

def test_extruded_cylinder_equals_the_2d_device_result(setups):
    st = setups("cyl6")
    case, n, nz = st.case, 6, 2
    w2 = _vorticity(st.h, st.u)[0]                                                  # the 2-D DEVICE result
    c3 = mesh3d.extrude_case(case, nz, 1.0)
    u3 = np.array([mesh3d.extrude_field(st.u[0], nz), mesh3d.extrude_field(st.u[1], nz), np.zeros((c3.nel, n, n, n))])
    h = NekStabHip(c3, c3.meta["vert"], c3.meta["nvert"], **KW3)
    try:
        ox, oy, oz, op = _vorticity(h, u3)
    finally:
        h.close()
    s = np.max(np.abs(w2))
    oz = oz.reshape(nz, case.nel, n, n, n)
    for kz in range(nz):
        for lev in range(n):
            assert np.max(np.abs(oz[kz, :, lev] - w2)) <= 1e-12 * s, (kz, lev)
    print(f"omega_x, omega_y over max |omega_z|: {np.max(np.abs(ox)) / s:.2e}, {np.max(np.abs(oy)) / s:.2e}")
    assert np.max(np.abs(ox)) <= 1e-12 * s and np.max(np.abs(oy)) <= 1e-12 * s
    assert not np.any(op)


# ---- 7. hexahedra, genuinely 3-D -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["box6", "box8", "box10"])
def test_deformed_boxes_match_numpy(setups, name):
    st = setups(name)
    out = _vorticity(st.h, st.u)
    for c in range(3):
        err = _rel(out[c], st.ref[c])
        print(f"{name} component {c}: device against numpy {err:.2e}")
        assert err <= 1e-12, c
    assert not np.any(out[3])


# ---- 8. no side effects --------------------------------------------------------------------------------------------

def test_a_vorticity_call_leaves_the_maps_and_their_graphs_alone(setups):
    st = setups("cyl6")
    h = st.h
    nsteps = h.nsteps
    h.set_nsteps(5)
    q, f, w = h.alloc(3)
    try:
        S.upload_velocity(h, q, st.u * st.case.mask)
        h.matvec(f, q)                                                              # (settles budgets and captures)
        h.matvec(f, q)
        m1 = [np.array(a) for a in h.download(f)]
        s0 = h.stats()
        h.vorticity(w, q)
        s1 = h.stats()
        assert s0["recaptures"] == s1["recaptures"]
        h.matvec(f, q)
        m2 = h.download(f)
        for a, b in zip(m1, m2):
            assert np.array_equal(a, b)
        assert h.stats()["recaptures"] == s0["recaptures"]
    finally:
        h.free([q, f, w])
        h.set_nsteps(nsteps)


# ---- 9. shards -----------------------------------------------------------------------------------------------------

def _check_group(g, st):
    """group vorticity against WHOLE-mesh numpy, every component; two calls give the same bits; returns the fields"""
    nd = g.ndim
    q, w, w2 = g.alloc(3)
    try:
        S.upload_velocity(g, q, st.u)
        g.vorticity(w, q)
        g.vorticity(w2, q)
        out, out2 = _all(g, w), _all(g, w2)
        np.testing.assert_array_equal(S.download_velocity(g, q), st.u)              # q is left as it is
    finally:
        g.free([q, w, w2])
    for c in range(len(st.ref)):
        err = _rel(out[c], st.ref[c])
        print(f"component {c}: sharded device against whole-mesh numpy {err:.2e}")
        assert err <= 1e-12, c
    for a in out[len(st.ref):]:
        assert not np.any(a)                                                        # vy (2-D) and the pressure: 0
    for a, b in zip(out, out2):
        assert np.array_equal(a, b)
    return out


@pytest.mark.parametrize("name,nranks", [("cyl6", 2), ("cyl6", 3), ("box6", 2), ("box6", 3)])
def test_virtual_ranks_match_whole_mesh_numpy(setups, name, nranks):
    st = setups(name)
    g = ShardGroup(st.h, st.case, nranks)
    try:
        halo = [shard_halo_counts(g.lib, c, nranks)[0] for c in g.ctx]
        assert all(h.sum() > 0 for h in halo), halo                                 # every rank exchanges a halo
        _check_group(g, st)
    finally:
        g.close()


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
        _check_group(g, st)
    finally:
        g.close()
        for p in parents:
            p.close()


def test_two_processes_on_one_gpu():
    """Two ranks, one process each, sharing this GPU; the halo travels over gloo on the host (nsk_comm_init_host): rank-local
    set-up, released parents, the cylinder at lx1 = 6 against whole-mesh numpy on every rank."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", "29683", os.path.join(ROOT, "tests", "mp_vort_worker.py")],
                         capture_output=True, text=True, timeout=600, env=env)
    print([l for l in out.stdout.splitlines() if "MPVORT" in l], out.stderr[-1500:] if out.returncode else "")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count("MPVORT rank") == 2


# ---- 10. files -----------------------------------------------------------------------------------------------------

def test_outpost_ks_writes_the_device_vorticity(setups, tmp_path):
    st = setups("cyl6")
    h, case = st.h, st.case
    nsteps = h.nsteps
    h.set_nsteps(5)
    v0 = h.alloc(1)[0]
    res = None
    try:
        S.upload_velocity(h, v0, st.u * case.mask)
        res = krylov.krylov_schur(h, v0, 8, mode=0, schur_tgt=0)
        tol = 2.0 * float(np.max(res.residual)) + 1e-300                            # loose: every Ritz pair counts as converged
        d0, d1 = tmp_path / "plain", tmp_path / "vor"
        w0 = outpost.outpost_ks(h, res, case, str(d0), eigen_tol=tol, maxmodes=2)
        w1 = outpost.outpost_ks(h, res, case, str(d1), eigen_tol=tol, maxmodes=2, ifvor=True)
        names = ["dRe1cyl0.f00001", "dIm1cyl0.f00001", "dRe1cyl0.f00002", "dIm1cyl0.f00002"]
        assert [os.path.basename(f) for f in w0] == names                           # what outpost_ks returned before the switch existed
        assert [os.path.basename(f) for f in w1] == names + ["dRv1cyl0.f00001", "dRv1cyl0.f00002"]
        assert not [f for f in os.listdir(d0) if "Rv" in f]
        for a, b in zip(w0, w1):
            assert open(a, "rb").read() == open(b, "rb").read()
        re, im, w = h.alloc(3)
        try:
            for i in range(2):
                krylov.assemble_mode(h, res, i, re, im)
                h.vorticity(w, re)
                dev = h.download(w)[0]
                rv, fr = nekio.read_fld(w1[4 + i]), nekio.read_fld(w1[2 * i])
                assert rv.rdcode == "XU" and rv.p is None and rv.t is None
                assert (rv.time, rv.istep, rv.wdsize) == (fr.time, fr.istep, fr.wdsize)
                assert np.array_equal(rv.u[0, :, 0], dev.astype(np.float32).astype(np.float64))
                assert not np.any(rv.u[1]) and np.any(rv.u[0])
        finally:
            h.free([re, im, w])
    finally:
        h.free([v0] + (list(res.Q) if res is not None else []))
        h.set_nsteps(nsteps)


# ---- 11. refusals --------------------------------------------------------------------------------------------------

def test_refusals(setups):
    st = setups("cyl6")
    h, lib = st.h, st.h.lib
    q, w = h.alloc(2)
    try:
        S.upload_velocity(h, q, st.u)
        with pytest.raises(NskError) as e:
            h.vorticity(q, q)                                                       # w == q
        assert e.value.code == -1 and "input" in str(e.value)
        assert lib.nsk_vorticity(h.ctx, None, w) == -1
        np.testing.assert_array_equal(S.download_velocity(h, q), st.u)              # the refused call wrote nothing
        ctx = (C.c_void_p * 1)(h.ctx.value)
        one = lambda v: (C.c_void_p * 1)(v.value)
        assert lib.nsk_group_vorticity(ctx, 1, one(q), one(w)) == -1                # a full-mesh context is no shard
        assert b"needs shard contexts" in lib.nsk_last_error()
    finally:
        h.free([q, w])
    g = ShardGroup(h, st.case, 2)
    try:
        a, b = g.alloc(2)
        assert lib.nsk_vorticity(g.ctx[0], a.parts[0], b.parts[0]) == -1            # a shard handed to the single-rank entry
        assert b"single-rank" in lib.nsk_last_error()
        with pytest.raises(NskError) as e:
            g.vorticity(a, a)
        assert e.value.code == -1 and "input" in str(e.value)
        # arrays that hold fewer than n handles: the missing entries are NULL
        short_q = (C.c_void_p * 2)(a.parts[0].value, None)
        short_w = (C.c_void_p * 2)(b.parts[0].value, None)
        full_q, full_w = g._per_rank(a), g._per_rank(b)
        for qa, wa in ((short_q, full_w), (full_q, short_w), (None, full_w), (full_q, None)):
            assert lib.nsk_group_vorticity(g._arr, 2, qa, wa) == -1
            assert b"nsk_group_vorticity" in lib.nsk_last_error()
        assert lib.nsk_group_vorticity(g._arr, 0, full_q, full_w) == -1
        g.free([a, b])
    finally:
        g.close()
