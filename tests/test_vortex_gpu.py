"""Vortex identification on the device (nsk_vortex_criteria, nsk_group_vortex_criteria: vortex_core('lambda2' / 'q' / 'omega') of
nekStab_outpost's vox and omg files) against the numpy restatement sensitivity.np_vortex_criteria: relative L2 error <= 1e-12,
the bound of tests/test_sensitivity_gpu.py and tests/test_vorticity_gpu.py for device against numpy.

The contexts, the shard groups' parents and the numpy references are built once per module."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from nekstab_amd import krylov, mesh, mesh3d, nekio, outpost
from nekstab_amd import sensitivity as S
from nekstab_amd.capi import NekStabHip, NskError
from nekstab_amd.sharded import ShardGroup, local_parents
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
KW = dict(tol_helm=1e-12, tol_pres=1e-6, tol_relative=1, schwarz_layers=2, max_helm_iter=240, max_pres_iter=96)
KW3 = dict(tol_helm=1e-12, tol_pres=1e-7, tol_relative=1, max_helm_iter=200, max_pres_iter=48)
UBF = lambda x, y, z: np.stack([1.0 - 0.3 * y * y + 0.1 * np.sin(x + z), 0.2 * np.cos(x) * y + 0.1 * z, 0.15 * np.sin(y + 0.5 * z)])
BOXES = {"box6": (4, 3, 2, 6, 0.05), "box8": (4, 3, 2, 8, 0.05), "box10": (2, 2, 2, 10, 0.06)}
NAMES = ("lambda2", "Q", "Omega")
_CACHE = {}


def _rel(a, b):
    return np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b))


def _cyl_case(lx1):
    return mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), lx1)


def _cyl_mode(lx1):
    """the reference's leading direct mode (real part), brought to lx1 by interp_gll"""
    return S.interp_gll(np.load(os.path.join(GOLDEN, "cylinder_modes.npz"))["dRe_u"].astype(np.float64), lx1)


def _box(name, **kw):
    shape = BOXES[name]
    return mesh3d.box_case_3d(*shape[:4], lengths=(2.0, 1.0, 0.8), outflow_xmax=True, re=40.0, endtime=0.05, ub_func=UBF, warp=shape[4], **kw)


def _smooth_mode(c):
    """the first of the analytic modes of tests/test_sensitivity_sharded_gpu.py (every derivative non-zero)"""
    x, y, z = c.x, c.y, c.z
    f = lambda a, b, cc, d: np.sin(a * x + 0.3) * np.cos(b * y - 0.2) * np.exp(cc * z) + d * x * y * z
    return np.array([f(1.1, 0.7, 0.3, 0.2), f(0.5, 1.3, -0.4, 0.1), f(0.9, 0.4, 0.8, -0.3)])


class Setup:
    """One case: its full-mesh context, the mode and the numpy criteria of the WHOLE mesh at wght = 0.5 and 0 (computed once,
    read only): ref[wght] = (lambda2, Q, Omega)."""

    def __init__(self, name):
        if name == "cyl6":
            self.case, self.u = _cyl_case(6), _cyl_mode(6)
            self.h = NekStabHip(self.case, self.case.meta["vert"], self.case.meta["nvert"], **KW)
        else:
            self.case = _box(name)
            self.u = _smooth_mode(self.case)
            self.h = NekStabHip(self.case, self.case.meta["vert"], self.case.meta["nvert"], **KW3)
        self.geom = S.NpGeom(self.case)
        self.ref = {}
        for w in (0.5, 0.0):
            self.ref[w] = np.array(S.np_vortex_criteria(self.geom, self.u, w))
            self.ref[w].setflags(write=False)


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
    return [np.array(a) for a in (h.download3(v) if h.ndim == 3 else h.download(v))]


def _criteria(h, u, wght=0.5):
    """upload u, run the device entry with an omega vector: (every downloaded slot of w, every downloaded slot of omega)"""
    q, w, om = h.alloc(3)
    try:
        S.upload_velocity(h, q, u)
        h.vortex_criteria(w, q, wght, omega=om)
        return _all(h, w), _all(h, om)
    finally:
        h.free([q, w, om])


def _three(h, w, om):
    """(lambda2, Q, Omega) out of the downloaded slots: Omega is w's vz in 3-D and omega's vx in 2-D"""
    return [w[0], w[1], w[2] if h.ndim == 3 else om[0]]


def _check(fields, ref, what):
    for name, a, b in zip(NAMES, fields, ref):
        err = _rel(a, b)
        print(f"{what} {name}: device against numpy {err:.2e}")
        assert err <= 1e-12, (what, name)


# ---- 1. cylinder at lx1 = 6, the reference's mode ------------------------------------------------------------------

def test_cylinder_lx6_matches_numpy_and_fills_every_slot(setups):
    """A context that carries one scalar field (theta), so that every kind of slot of the outputs is there to be zeroed; the
    output vectors are filled with non-zero values first."""
    st = setups("cyl6")
    case, u = st.case, st.u
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **KW)
    try:
        h.set_nscal(1)
        q, w, om, w2, om2, w0, om0 = h.alloc(7)
        rng = np.random.default_rng(5)
        pr, th = rng.standard_normal((case.nel, 4, 4)), rng.standard_normal(case.x.shape)
        h.upload(q, u[0], u[1], pr)
        h.upload_scalar(q, 0, th)
        for o in (w, om, w2, om2, w0, om0):
            h.upload(o, th, th + 1.0, pr + 2.0)
            h.upload_scalar(o, 0, th - 3.0)
        before = [np.array(a) for a in h.download(q)] + [h.download_scalar(q, 0)]
        h.vortex_criteria(w, q, 0.5, omega=om)
        h.vortex_criteria(w0, q, 0.0, omega=om0)
        h.vortex_criteria(w2, q, 0.5, omega=om2)                                    # (after a call with another weight)
        after = [np.array(a) for a in h.download(q)] + [h.download_scalar(q, 0)]
        for a, b in zip(before, after):
            assert np.array_equal(a, b)                                             # q is read only
        got = {}
        for wght, vw, vo in ((0.5, w, om), (0.0, w0, om0)):
            lam, qq, wp = h.download(vw)
            ox, oy, op = h.download(vo)
            _check([lam, qq, ox], st.ref[wght], f"cyl6 wght = {wght}:")
            assert not np.any(wp) and not np.any(h.download_scalar(vw, 0))          # exactly zero
            assert not np.any(oy) and not np.any(op) and not np.any(h.download_scalar(vo, 0))
            got[wght] = [np.array(lam), np.array(qq), np.array(ox)]
        for a, b in zip(h.download(w2) + h.download(om2), h.download(w) + h.download(om)):
            assert np.array_equal(a, b)                                             # a second call: the same bits
        for name, a, b in zip(NAMES, got[0.5], got[0.0]):
            assert _rel(a, b) > 1e-6, name                                          # the filter does something
        # the default weight is the reference's 0.5, and omega may be left out
        h.upload(w2, th, th + 1.0, pr + 2.0)
        h.vortex_criteria(w2, q)
        for a, b in zip(h.download(w2), h.download(w)):
            assert np.array_equal(a, b)
    finally:
        h.close()


# ---- 2. quadrilaterals at lx1 = 8, 10, 12 --------------------------------------------------------------------------

@pytest.mark.parametrize("lx1", [8, 10, 12])
def test_quadrilaterals_match_numpy(lx1):
    case, u = _cyl_case(lx1), _cyl_mode(lx1)
    geom = S.NpGeom(case)
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **KW)
    try:
        for wght in (0.5, 0.0):
            w, om = _criteria(h, u, wght)
            _check(_three(h, w, om), S.np_vortex_criteria(geom, u, wght), f"lx1 = {lx1} wght = {wght}:")
            assert not np.any(w[2]) and not np.any(om[1]) and not np.any(om[2])
    finally:
        h.close()


# ---- 3. hexahedra, genuinely 3-D -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["box6", "box8", "box10"])
def test_deformed_boxes_match_numpy(setups, name):
    st = setups(name)
    for wght in (0.5, 0.0):
        w, om = _criteria(st.h, st.u, wght)
        _check(_three(st.h, w, om), st.ref[wght], f"{name} wght = {wght}:")
        assert np.array_equal(w[2], om[0])                                          # w's vz is omega's vx, bit for bit
        assert not np.any(w[3]) and not np.any(om[1]) and not np.any(om[2]) and not np.any(om[3])


# ---- 4. hexahedra, z-invariant: degenerate at every node -----------------------------------------------------------

def test_extruded_cylinder_is_degenerate_at_every_node_and_equals_the_2d_device_result(setups):
    """w = 0 and d/dz = 0: A = diag(A_2D, 0), and A_2D is (nearly: the mode is discretely, not pointwise, divergence-free) a
    multiple of the identity.  lambda2 against numpy's eigvalsh relative to the field's L2 norm; Q half and Omega equal to the
    2-D DEVICE result on every plane (the filter leaves constants alone, so z-invariance survives it)."""
    st = setups("cyl6")
    case, n, nz = st.case, 6, 2
    w2, om2 = _criteria(st.h, st.u, 0.5)                                            # the 2-D DEVICE result
    c3 = mesh3d.extrude_case(case, nz, 1.0)
    u3 = np.array([mesh3d.extrude_field(st.u[0], nz), mesh3d.extrude_field(st.u[1], nz), np.zeros((c3.nel, n, n, n))])
    ref = S.np_vortex_criteria(S.NpGeom(c3), u3, 0.5)
    h = NekStabHip(c3, c3.meta["vert"], c3.meta["nvert"], **KW3)
    try:
        w3, om3 = _criteria(h, u3, 0.5)
    finally:
        h.close()
    err = _rel(w3[0], ref[0])
    print(f"extruded cylinder: lambda2 device against numpy {err:.2e}")
    assert err <= 1e-12
    sq, so = np.max(np.abs(w2[1])), np.max(np.abs(om2[0]))
    q3, o3 = w3[1].reshape(nz, case.nel, n, n, n), w3[2].reshape(nz, case.nel, n, n, n)
    for kz in range(nz):
        for lev in range(n):
            assert np.max(np.abs(2.0 * q3[kz, :, lev] - w2[1])) <= 1e-12 * sq, (kz, lev)
            assert np.max(np.abs(o3[kz, :, lev] - om2[0])) <= 1e-12 * so, (kz, lev)
    assert np.array_equal(w3[2], om3[0]) and not np.any(w3[3])


# ---- 5. shards -----------------------------------------------------------------------------------------------------

def _check_group(g, st):
    """group criteria against WHOLE-mesh numpy, rank by rank through the element lists of nsk_shard_elems; two calls give the
    same bits; q is left as it is"""
    q, w, om, w2, om2 = g.alloc(5)
    try:
        S.upload_velocity(g, q, st.u)
        g.vortex_criteria(w, q, 0.5, omega=om)
        g.vortex_criteria(w2, q, 0.5, omega=om2)
        out, oom, out2, oom2 = _all(g, w), _all(g, om), _all(g, w2), _all(g, om2)
        np.testing.assert_array_equal(S.download_velocity(g, q), st.u)
    finally:
        g.free([q, w, om, w2, om2])
    fields = _three(g, out, oom)
    assert sorted(np.concatenate(g.elems).tolist()) == list(range(st.case.nel))
    for r, e in enumerate(g.elems):
        for name, a, b in zip(NAMES, fields, st.ref[0.5]):
            err = _rel(a[e], b[e])
            print(f"rank {r} {name}: sharded device against whole-mesh numpy {err:.2e}")
            assert err <= 1e-12, (r, name)
    for a in out[g.ndim:] + oom[1:]:
        assert not np.any(a)
    for a, b in zip(out + oom, out2 + oom2):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name,nranks", [("cyl6", 2), ("cyl6", 3), ("box8", 2), ("box8", 3)])
def test_virtual_ranks_match_whole_mesh_numpy(setups, name, nranks):
    st = setups(name)
    g = ShardGroup(st.h, st.case, nranks)
    try:
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
    """Two ranks, one process each (fresh children), sharing this GPU: rank-local set-up, released parents, the cylinder at
    lx1 = 6 against whole-mesh numpy on every rank; the criteria exchange nothing."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29687", os.path.join(ROOT, "tests", "mp_vortex_worker.py")],
                         capture_output=True, text=True, timeout=600, env=env)
    print([l for l in out.stdout.splitlines() if "MPVOX" in l], out.stderr[-1500:] if out.returncode else "")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.count("MPVOX rank") == 2


# ---- 6. no side effects --------------------------------------------------------------------------------------------

def test_a_vortex_criteria_call_leaves_the_maps_and_their_graphs_alone(setups):
    st = setups("cyl6")
    h = st.h
    nsteps = h.nsteps
    h.set_nsteps(5)
    q, f, w, om = h.alloc(4)
    try:
        S.upload_velocity(h, q, st.u * st.case.mask)
        h.matvec(f, q)                                                              # (settles budgets and captures)
        h.matvec(f, q)
        m1 = [np.array(a) for a in h.download(f)]
        s0 = h.stats()
        h.vortex_criteria(w, q, 0.5, omega=om)
        s1 = h.stats()
        assert s0 == s1                                                             # no step, no recapture, no counter moved
        h.matvec(f, q)
        m2 = h.download(f)
        for a, b in zip(m1, m2):
            assert np.array_equal(a, b)
        assert h.stats()["recaptures"] == s0["recaptures"]
    finally:
        h.free([q, f, w, om])
        h.set_nsteps(nsteps)


# ---- 7. contexts of nsk_init_masks ---------------------------------------------------------------------------------

def test_a_context_with_component_masks_gives_the_same_bits(setups):
    st = setups("box6")
    cs = _box("box6", sym={"ymin": "SYM", "zmax": "ON "})
    assert cs.cmask is not None and np.array_equal(cs.x, st.case.x)
    h = NekStabHip(cs, cs.meta["vert"], cs.meta["nvert"], **KW3)
    try:
        ws, oms = _criteria(h, st.u, 0.5)
    finally:
        h.close()
    w, om = _criteria(st.h, st.u, 0.5)
    for a, b in zip(ws + oms, w + om):
        assert np.array_equal(a, b)


# ---- 8. files ------------------------------------------------------------------------------------------------------

def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def test_outpost_vox_writes_the_device_fields(setups, tmp_path):
    for name in ("cyl6", "box6"):
        st = setups(name)
        h, case = st.h, st.case
        for be in (h, ShardGroup(h, case, 2)):
            d = tmp_path / (name + type(be).__name__)
            q, w, om = be.alloc(3)
            try:
                S.upload_velocity(be, q, st.u)
                files = outpost.outpost_vox(be, q, case, str(d), session="1cyl", num=3)
                be.vortex_criteria(w, q, 0.5, omega=om)
                dw, dom = _all(be, w), _all(be, om)
            finally:
                be.free([q, w, om])
                if be is not h:
                    be.close()
            vox = nekio.read_fld(files[0])
            assert os.path.basename(files[0]) == "vox1cyl0.f00003" and vox.rdcode == "XU" and vox.p is None and vox.t is None
            if h.ndim == 2:
                assert [os.path.basename(f) for f in files] == ["vox1cyl0.f00003", "omg1cyl0.f00003"]
                assert sorted(os.listdir(d)) == ["omg1cyl0.f00003", "vox1cyl0.f00003"]
                omg = nekio.read_fld(files[1])
                assert omg.rdcode == "XT" and omg.u is None and omg.p is None
                assert np.array_equal(np.asarray(omg.t).reshape(dom[0].shape), _f32(dom[0])) and np.any(dom[0])
                for c in range(2):
                    assert np.array_equal(vox.u[c, :, 0], _f32(dw[c])) and np.any(dw[c])
            else:
                assert len(files) == 1 and os.listdir(d) == ["vox1cyl0.f00003"]
                for c in range(3):
                    assert np.array_equal(vox.u[c], _f32(dw[c])) and np.any(dw[c])


def test_outpost_ks_writes_the_vox_files_of_the_modes(setups, tmp_path):
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
        d0, d1 = tmp_path / "vor", tmp_path / "vox"
        w0 = outpost.outpost_ks(h, res, case, str(d0), eigen_tol=tol, maxmodes=2, ifvor=True)
        w1 = outpost.outpost_ks(h, res, case, str(d1), eigen_tol=tol, maxmodes=2, ifvor=True, ifvox=True)
        new = ["dRx1cyl0.f00001", "dRo1cyl0.f00001", "dRx1cyl0.f00002", "dRo1cyl0.f00002"]
        assert [os.path.basename(f) for f in w1] == [os.path.basename(f) for f in w0] + new
        assert sorted(set(os.listdir(d1)) - set(os.listdir(d0))) == sorted(new)
        for a, b in zip(w0, w1):                                                    # the other files do not depend on the switch
            assert open(a, "rb").read() == open(b, "rb").read()
        re, im, w, om = h.alloc(4)
        try:
            for i in range(2):
                krylov.assemble_mode(h, res, i, re, im)
                h.vortex_criteria(w, re, 0.5, omega=om)
                dw, dom = h.download(w), h.download(om)
                rx, ro, fr = nekio.read_fld(w1[len(w0) + 2 * i]), nekio.read_fld(w1[len(w0) + 2 * i + 1]), nekio.read_fld(w1[2 * i])
                assert rx.rdcode == "XU" and rx.p is None and rx.t is None and ro.rdcode == "XT" and ro.u is None
                for f in (rx, ro):
                    assert (f.time, f.istep, f.wdsize) == (fr.time, fr.istep, fr.wdsize)
                for c in range(2):
                    assert np.array_equal(rx.u[c, :, 0], _f32(dw[c])) and np.any(dw[c])
                assert np.array_equal(np.asarray(ro.t).reshape(dom[0].shape), _f32(dom[0])) and np.any(dom[0])
        finally:
            h.free([re, im, w, om])
    finally:
        h.free([v0] + (list(res.Q) if res is not None else []))
        h.set_nsteps(nsteps)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------

def test_refusals(setups):
    st = setups("cyl6")
    h, lib = st.h, st.h.lib
    q, w, om = h.alloc(3)
    name = b"nsk_vortex_criteria"
    try:
        S.upload_velocity(h, q, st.u)
        for args in ((q, q, None), (w, q, q), (w, q, w)):                           # w == q, omega == q, omega == w
            with pytest.raises(NskError) as e:
                h.vortex_criteria(args[0], args[1], 0.5, omega=args[2])
            assert e.value.code == -1 and "nsk_vortex_criteria" in str(e.value) and "distinct" in str(e.value)
        for bad in (-0.1, 1.0000001, float("nan"), float("inf")):
            with pytest.raises(NskError) as e:
                h.vortex_criteria(w, q, bad)
            assert e.value.code == -1 and "nsk_vortex_criteria" in str(e.value) and "weight" in str(e.value)
        assert lib.nsk_vortex_criteria(h.ctx, None, 0.5, w, om) == -1 and name in lib.nsk_last_error()
        assert lib.nsk_vortex_criteria(h.ctx, q, 0.5, None, om) == -1 and name in lib.nsk_last_error()
        assert lib.nsk_vortex_criteria(None, q, 0.5, w, om) == -1 and name in lib.nsk_last_error()
        np.testing.assert_array_equal(S.download_velocity(h, q), st.u)              # the refused calls wrote nothing
        h.vortex_criteria(w, q, 1.0)                                                # the ends of [0, 1] are accepted
        ctx = (C.c_void_p * 1)(h.ctx.value)
        one = lambda v: (C.c_void_p * 1)(v.value)
        assert lib.nsk_group_vortex_criteria(ctx, 1, one(q), 0.5, one(w), None) == -1      # a full-mesh context is no shard
        assert b"needs shard contexts" in lib.nsk_last_error() and b"nsk_group_vortex_criteria" in lib.nsk_last_error()
    finally:
        h.free([q, w, om])
    g = ShardGroup(h, st.case, 2)
    gname = b"nsk_group_vortex_criteria"
    try:
        a, b, c = g.alloc(3)
        assert lib.nsk_vortex_criteria(g.ctx[0], a.parts[0], 0.5, b.parts[0], None) == -1  # a shard handed to the single-rank entry
        assert b"single-rank" in lib.nsk_last_error() and name in lib.nsk_last_error()
        for args in ((a, a, None), (b, a, a), (b, a, b)):
            with pytest.raises(NskError) as e:
                g.vortex_criteria(args[0], args[1], 0.5, omega=args[2])
            assert e.value.code == -1 and "nsk_group_vortex_criteria" in str(e.value)
        with pytest.raises(NskError) as e:
            g.vortex_criteria(b, a, 2.0)
        assert "nsk_group_vortex_criteria" in str(e.value) and "weight" in str(e.value)
        # arrays that hold fewer than n handles: the missing entries are NULL
        short = lambda v: (C.c_void_p * 2)(v.parts[0].value, None)
        fq, fw, fo = g._per_rank(a), g._per_rank(b), g._per_rank(c)
        for qa, wa, oa in ((short(a), fw, fo), (fq, short(b), fo), (fq, fw, short(c)), (None, fw, fo), (fq, None, fo)):
            assert lib.nsk_group_vortex_criteria(g._arr, 2, qa, 0.5, wa, oa) == -1
            assert gname in lib.nsk_last_error()
        assert lib.nsk_group_vortex_criteria(g._arr, 0, fq, 0.5, fw, fo) == -1
        g.free([a, b, c])
    finally:
        g.close()
