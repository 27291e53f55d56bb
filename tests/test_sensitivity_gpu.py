"""Sensitivity post-processing on the device (nsk_biorthogonalize, nsk_wavemaker, nsk_bf_sensitivity, nsk_forced_map) against
the numpy restatement (nekstab_amd/sensitivity.py), the reference's own bf_sensitivity output and a forced oracle step."""
import ctypes as C
import os

import numpy as np
import pytest

from nekstab_amd import mesh, mesh3d, nekio
from nekstab_amd import sensitivity as S
from nekstab_amd.capi import NSK_ADJOINT, NSK_DIRECT, NekStabHip, NskError

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KW = dict(tol_helm=1e-10, tol_pres=1e-6, tol_relative=1, max_helm_iter=100, max_pres_iter=48)


def _case(lx1):
    return mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), lx1)


def _modes(lx1):
    m = np.load(os.path.join(GOLDEN, "cylinder_modes.npz"))
    return [S.interp_gll(m[k + "_u"].astype(np.float64), lx1) for k in ("dRe", "dIm", "aRe", "aIm")]


def _rel(a, b):
    return np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b))


def _upload_modes(h, modes):
    vecs = h.alloc(4)
    for v, u in zip(vecs, modes):
        S.upload_velocity(h, v, u)
    return vecs


@pytest.fixture(scope="module", params=[6, 8], ids=["lx6", "lx8"])
def ctx2(request):
    lx1 = request.param
    case = _case(lx1)
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **KW)
    yield lx1, case, h
    h.close()


def test_biorthogonalize_matches_numpy(hip6, case6):
    h, case = hip6, case6
    g = S.NpGeom(case)
    modes = _modes(6)
    ref = S.np_biorthogonalize(g, *modes)
    v = _upload_modes(h, modes)
    try:
        gamma, delta = h.biorthogonalize(*v)
        assert abs(gamma - ref[4]) <= 1e-12 * abs(ref[4]) and abs(delta - ref[5]) <= 1e-12 * abs(ref[5])
        dRe, dIm, aRe, aIm = v
        re = h.dot(aRe, dRe) + h.dot(aIm, dIm)
        im = h.dot(aRe, dIm) - h.dot(aIm, dRe)
        assert abs(re - 1.0) <= 1e-12 and abs(im) <= 1e-12
        assert abs(h.dot(dRe, dRe) + h.dot(dIm, dIm) - 1.0) <= 1e-12
        for k, vec in enumerate(v):
            assert _rel(S.download_velocity(h, vec), ref[k]) <= 1e-12
    finally:
        h.free(v)


def test_wavemaker_and_bf_sensitivity_match_numpy_and_reference(ctx2):
    lx1, case, h = ctx2
    g = S.NpGeom(case)
    dRe, dIm, aRe, aIm, _, _ = S.np_biorthogonalize(g, *_modes(lx1))
    ref = S.np_bf_sensitivity(g, dRe, dIm, aRe, aIm)
    v = _upload_modes(h, (dRe, dIm, aRe, aIm))
    outs = h.alloc(7)
    try:
        h.wavemaker(*v, outs[6])
        wm = S.download_velocity(h, outs[6])
        assert _rel(wm[0], S.np_wavemaker(dRe, dIm, aRe, aIm)) <= 1e-12 and not np.any(wm[1])
        h.bf_sensitivity(*v, outs[0], outs[1], parts=outs[2:6])
        got = {k: S.download_velocity(h, o) for k, o in zip(("sr", "si", "tr", "ti", "pr", "pi"), outs)}
        for k in got:
            assert _rel(got[k], ref[k]) <= 1e-12, k
        assert np.array_equal(got["sr"], got["tr"] + got["pr"]) and np.array_equal(got["si"], got["ti"] + got["pi"])
        assert not np.any(h.download(outs[0])[2])                                        # pressure of the outputs: 0
        # without parts: the same sr / si
        h.bf_sensitivity(*v, outs[2], outs[3])
        assert _rel(S.download_velocity(h, outs[2]), got["sr"]) <= 1e-13
        assert _rel(S.download_velocity(h, outs[3]), got["si"]) <= 1e-13
        if lx1 == 6:                                                                      # the reference's sr_ / si_
            fx = np.load(os.path.join(GOLDEN, "cylinder_bf_sensitivity.npz"))
            for k in ("sr", "si"):
                r = fx[k + "_u"].astype(np.float64)
                err = np.sqrt(g.inner(got[k] - r, got[k] - r, g.bm1) / g.inner(r, r, g.bm1))
                print(f"{k} against the reference's file: weighted L2 {err:.2e}")
                assert err <= 1e-2
    finally:
        h.free(v + outs)


@pytest.mark.parametrize("lx1", [6, 8])
def test_hexahedra_extruded_cylinder_equals_2d(lx1):
    """z-extruded cylinder: every z plane of the 3-D outputs is the 2-D field, the z components are 0."""
    case = _case(lx1)
    nz = 2
    c3 = mesh3d.extrude_case(case, nz, 1.0)
    m2 = _modes(lx1)
    ref = S.np_bf_sensitivity(S.NpGeom(case), *m2)
    n = lx1
    m3 = [np.array([mesh3d.extrude_field(a[0], nz), mesh3d.extrude_field(a[1], nz), np.zeros((c3.nel, n, n, n))]) for a in m2]
    h = NekStabHip(c3, c3.meta["vert"], c3.meta["nvert"], **KW)
    try:
        v = _upload_modes(h, m3)
        outs = h.alloc(6)
        h.bf_sensitivity(*v, outs[0], outs[1], parts=outs[2:])
        for k, o in zip(("sr", "si", "tr", "ti", "pr", "pi"), outs):
            a = S.download_velocity(h, o).reshape(3, nz, case.nel, n, n, n)
            s = np.max(np.abs(ref[k]))
            for kz in range(nz):
                for lev in range(n):
                    assert np.max(np.abs(a[:2, kz, :, lev] - ref[k])) <= 1e-12 * s, (k, kz, lev)
            assert np.max(np.abs(a[2])) <= 1e-12 * s
        h.wavemaker(*v, outs[0])
        wm = S.download_velocity(h, outs[0])[0].reshape(nz, case.nel, n, n, n)
        w2 = S.np_wavemaker(*m2)
        assert np.max(np.abs(wm - w2[None, :, None])) <= 1e-12 * np.max(w2)
        h.free(v + outs)
    finally:
        h.close()


def test_hexahedra_genuinely_3d_field_matches_numpy():
    """Deformed box, smooth fields with every derivative non-zero: pins the 3-D terms, d v / d z of the transport term included."""
    ubf = lambda x, y, z: np.stack([1.0 - 0.3 * y * y + 0.1 * np.sin(x + z), 0.2 * np.cos(x) * y + 0.1 * z, 0.15 * np.sin(y + 0.5 * z)])
    c = mesh3d.box_case_3d(2, 2, 2, 6, lengths=(2.0, 1.0, 0.8), outflow_xmax=True, re=40.0, endtime=0.05, warp=0.06, ub_func=ubf)
    x, y, z = c.x, c.y, c.z
    f = lambda a, b, cc, d: np.sin(a * x + 0.3) * np.cos(b * y - 0.2) * np.exp(cc * z) + d * x * y * z
    modes = [np.array([f(1.1, 0.7, 0.3, 0.2), f(0.5, 1.3, -0.4, 0.1), f(0.9, 0.4, 0.8, -0.3)]),
             np.array([f(0.6, 1.0, 0.5, 0.0), f(1.4, 0.2, 0.1, 0.4), f(0.3, 0.9, -0.6, 0.2)]),
             np.array([f(0.8, 0.5, -0.2, 0.3), f(0.2, 1.1, 0.7, -0.1), f(1.2, 0.6, 0.4, 0.0)]),
             np.array([f(1.3, 0.3, 0.6, -0.2), f(0.7, 0.8, -0.5, 0.3), f(0.4, 1.2, 0.2, 0.1)])]
    ref = S.np_bf_sensitivity(S.NpGeom(c), *modes)
    h = NekStabHip(c, c.meta["vert"], c.meta["nvert"], **KW)
    try:
        v = _upload_modes(h, modes)
        outs = h.alloc(6)
        h.bf_sensitivity(*v, outs[0], outs[1], parts=outs[2:])
        for k, o in zip(("sr", "si", "tr", "ti", "pr", "pi"), outs):
            assert _rel(S.download_velocity(h, o), ref[k]) <= 1e-12, k
        h.free(v + outs)
    finally:
        h.close()


# ---- forced maps -----------------------------------------------------------------------------------------------------

def _force(case):
    fx = np.load(os.path.join(GOLDEN, "cylinder_bf_sensitivity.npz"))
    return fx["sr_u"].astype(np.float64)


def _state(case):
    m = _modes(6)
    return m[0] * case.mask


def test_forced_map_with_zero_force_is_bit_identical_to_matvec():
    """Two fresh contexts with the same history: nsk_matvec and nsk_forced_map(force = 0), direct then adjoint."""
    case = _case(6)
    q = _state(case)
    res = []
    for forced in (False, True):
        h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **KW)
        try:
            h.set_nsteps(12)
            a, b, z = h.alloc(3)
            S.upload_velocity(h, a, q)
            h.zero(z)
            out = []
            for mode in (NSK_DIRECT, NSK_ADJOINT):
                if forced:
                    h.forced_map(b, a, z, mode)
                else:
                    h.matvec(b, a, mode)
                out.append(h.download(b))
            res.append(out)
        finally:
            h.close()
    for k in range(2):
        for x0, x1 in zip(res[0][k], res[1][k]):
            assert np.array_equal(x0, x1), k


def test_forced_map_superposition_and_oracle(case6, oracle6):
    """map(q, f) = map(q, 0) + map(0, f) at tight tolerances; the forced adjoint map from 0 against the oracle whose adjoint
    convection term also carries - B f (the force then enters where step() adds the sponge)."""
    from oracle.linns import LinNS2D
    f = _force(case6)
    q = _state(case6)
    h = NekStabHip(case6, case6.meta["vert"], case6.meta["nvert"], tol_helm=1e-13, tol_pres=1e-12, tol_relative=1,
                   max_helm_iter=200, max_pres_iter=144)
    h.set_nsteps(10)
    a, fv, z, r1, r2, r3 = h.alloc(6)
    try:
        S.upload_velocity(h, a, q)
        S.upload_velocity(h, fv, f)
        h.zero(z)
        for mode in (NSK_DIRECT, NSK_ADJOINT):
            h.forced_map(r1, a, fv, mode)
            h.matvec(r2, a, mode)
            h.forced_map(r3, z, fv, mode)
            lhs, rhs = S.download_velocity(h, r1), S.download_velocity(h, r2) + S.download_velocity(h, r3)
            assert _rel(lhs, rhs) <= 1e-10, mode
        got = S.download_velocity(h, r3)                         # adjoint, from zero

        class ForcedLinNS2D(LinNS2D):
            def convect_adj(self, cx, cy, Ux, Uy):
                ax, ay = super().convect_adj(cx, cy, Ux, Uy)
                return ax - self.bm1 * f[0], ay - self.bm1 * f[1]

        o = ForcedLinNS2D.__new__(ForcedLinNS2D)
        o.__dict__.update(oracle6.__dict__)
        zz = np.zeros_like(case6.x)
        ref = o.matvec((zz, zz, np.zeros((case6.nel, 4, 4))), adjoint=True, nsteps=10)
        err = _rel(got, np.array(ref[:2]))
        print(f"forced adjoint map from 0, 10 steps, against the oracle: {err:.2e}")
        assert err <= 1e-9
    finally:
        h.close()


def test_steady_force_sensitivity_end_to_end(tmp_path):
    """ts_steady_force_sensitivity at lx1 = 6 with force sr_: x solves (I - exp(L^+ T)) x = forced map of 0, so the forced
    adjoint map of x returns x."""
    case = _case(6)
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], tol_helm=1e-11, tol_pres=1e-8, tol_relative=1,
                   max_helm_iter=120, max_pres_iter=96)
    tol = 1e-10
    try:
        fv, chk, z, rhs = h.alloc(4)
        S.upload_velocity(h, fv, _force(case))
        its = []
        x, calls = S.steady_force_sensitivity(h, fv, k_dim=80, tol=tol, maxiter=10, log=lambda *a: its.append(a),
                                              outdir=str(tmp_path), session="1cyl")
        print(f"steady_force_sensitivity: {calls} linearised maps, GMRES log {[a for a in its if a[0] == 'gmres']}")
        h.zero(z)
        h.forced_map(rhs, z, fv, NSK_ADJOINT)
        h.forced_map(chk, x, fv, NSK_ADJOINT)
        h.axpy(chk, -1.0, x)
        res = h.norm(chk) / h.norm(rhs)
        print(f"relative residual of the fixed point: {res:.2e} (GMRES residual tolerance {np.sqrt(tol):.0e})")
        assert res <= 10 * np.sqrt(tol)
        fsr = nekio.read_fld(str(tmp_path / "fsr1cyl0.f00001"))
        assert fsr.u.shape == (2, case.nel, 1, 6, 6)
        h.free([fv, chk, z, rhs, x])
    finally:
        h.close()


def test_files_with_reference_prefixes_read_back(hip6, case6, tmp_path):
    v = _upload_modes(hip6, _modes(6))
    try:
        wm, gd = S.wave_maker(hip6, *v, outdir=str(tmp_path))
        out, _ = S.bf_sensitivity(hip6, *v, outdir=str(tmp_path))
    finally:
        hip6.free(v)
    f = nekio.read_fld(str(tmp_path / "wm_1cyl0.f00001"))
    assert f.t.shape == (case6.nel, 1, 6, 6) and f.x.shape == (2, case6.nel, 1, 6, 6)
    np.testing.assert_allclose(f.t[:, 0], wm, rtol=0, atol=0)
    for k in ("tr", "ti", "pr", "pi", "sr", "si"):
        f = nekio.read_fld(str(tmp_path / (k + "_1cyl0.f00001")))
        assert f.u.shape == (2, case6.nel, 1, 6, 6)
        np.testing.assert_array_equal(f.u[:, :, 0], out[k])
    dl, dw = S.delta_forcing(case6.ub, out["sr"], out["si"])
    S.write_delta_forcing(hip6, str(tmp_path / "dfr1cyl0.f00001"), dl, dw)
    assert nekio.read_fld(str(tmp_path / "dfr1cyl0.f00001")).u.shape == (2, case6.nel, 1, 6, 6)


def test_shards_and_bad_modes_are_refused(hip6, case6):
    from nekstab_amd.sharded import ShardGroup
    lib = hip6.lib
    g = ShardGroup(hip6, case6, 2)
    try:
        a = g.alloc(1)[0]
        p = a.parts[0]
        arr = (C.c_void_p * 4)(p, p, p, p)
        gd = np.zeros(2)
        assert lib.nsk_biorthogonalize(g.ctx[0], p, p, p, p, gd.ctypes.data_as(C.POINTER(C.c_double))) == -1
        assert b"single-rank" in lib.nsk_last_error()
        assert lib.nsk_wavemaker(g.ctx[0], p, p, p, p, p) == -1
        assert lib.nsk_bf_sensitivity(g.ctx[0], p, p, p, p, p, p, arr) == -1
        assert lib.nsk_forced_map(g.ctx[0], NSK_ADJOINT, p, p, p) == -1
        g.free([a])
    finally:
        g.close()
    a, b, c = hip6.alloc(3)
    try:
        for mode in (2, 3, 4, -1, 9):
            with pytest.raises(NskError) as e:
                hip6.forced_map(b, a, c, mode)
            assert e.value.code == -1
    finally:
        hip6.free([a, b, c])
