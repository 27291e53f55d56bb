"""Floquet maps over a Fourier-compressed periodic base flow (core/fourier.f; nsk_set_orbit_fourier, nsk_set_orbit_modes,
nsk_get_orbit_modes, option "orbit_phase"): k_orbit_dft and k_baseflow_fourier against the oracle, against the stored orbit
of nsk_set_orbit and, on hexahedra, against the quadrilateral path and steady contexts.  Every test builds its own contexts."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

HIP6 = dict(tol_helm=1e-13, tol_pres=1e-13, tol_relative=0, schwarz_layers=2, max_helm_iter=120, max_pres_iter=48)     # the fixture hip6
PERIOD = 2.3             # of the synthetic orbits: not the contexts' endtime
MEASURED_E8 = 2.26e-5    # err(8) of test_truncation_on_the_shedding_orbit as measured on the MI355X


def _synthetic_modes(ub, x, w=None):
    """M = 2 modes built from the base flow `ub` [2, ...] times functions of x: single-valued on shared nodes, the periodic
    y-pair included.  `w` (optional): a third, z-invariant component per mode, [5, ...] in the order A_0, A_1, B_1, A_2, B_2."""
    A = [ub, 0.3 * ub * np.cos(0.1 * x), 0.1 * ub * np.exp(-(x / 10.0) ** 2)]
    B = [0.2 * np.stack([ub[1], ub[0]]) * np.sin(0.07 * x), np.zeros_like(ub)]
    if w is not None:
        A = [np.concatenate([a, w[i][None]]) for a, i in zip(A, (0, 1, 3))]
        B = [np.concatenate([b, w[i][None]]) for b, i in zip(B, (2, 4))]
    return np.stack(A), np.stack(B)


def _upload_modes2(h, A, B):
    va, vb = h.alloc(len(A)), h.alloc(len(B))
    for v, m in zip(va + vb, list(A) + list(B)):
        h.upload(v, m[0], m[1], np.zeros(h.npres))
    return va, vb


def _upload_modes3(h, A, B, nz):
    from nekstab_amd import mesh3d
    va, vb = h.alloc(len(A)), h.alloc(len(B))
    for v, m in zip(va + vb, list(A) + list(B)):
        w = mesh3d.extrude_field(m[2], nz) if m.shape[0] == 3 else np.zeros((h.nel, h.lx1, h.lx1, h.lx1))
        h.upload3(v, mesh3d.extrude_field(m[0], nz), mesh3d.extrude_field(m[1], nz), w, np.zeros(h.npres))
    return va, vb


def _rel(h, a, b):
    """|a - b| / |b| in the device's inner product; a is overwritten"""
    h.axpy(a, -1.0, b)
    return h.norm(a) / h.norm(b)


def _bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("mode,phase", [(0, 0.0), (1, 0.0), (0, 0.37)])
def test_synthetic_modes_vs_oracle(case6, oracle6, modes, mode, phase):
    """Six linearised steps (BDF1-3 start-up + three regular ones) over a synthetic M = 2 orbit loaded with set_orbit_modes, at a
    period that is not endtime: the oracle steps with its base flow set to np_reconstruct at (istep - 1) dt / period (+ the
    phase) before every step.  Settings and bounds of test_steps_vs_oracle, the same comparison about a steady base flow."""
    from nekstab_amd import fourier
    from nekstab_amd.capi import NekStabHip
    from tests.test_matvec_gpu import _mode, relL2
    o = oracle6
    A, B = _synthetic_modes(case6.ub, case6.x)
    h = NekStabHip(case6, case6.meta["vert"], case6.meta["nvert"], **HIP6)
    try:
        va, vb = _upload_modes2(h, A, B)
        h.set_orbit_modes(va, vb, PERIOD)
        assert h.get_orbit_modes() == (2, PERIOD)
        o.set_baseflow(fourier.np_reconstruct(A, B, 0.0))
        assert abs(o.dt - h.dt) < 1e-15 and o.nsteps == h.nsteps
        if phase:
            h.set_option("orbit_phase", phase)
            o.dt = h.dt
            o._helm = {}
        nsteps = 6
        q = _mode(o, modes, "dRe")
        h.set_nsteps(nsteps)
        vq, vf = h.alloc(2)
        h.upload(vq, *q)
        h.matvec(vf, vq, mode)
        f = h.download(vf)
        st = o.new_state(q)
        for istep in range(1, nsteps + 1):
            o.ub = fourier.np_reconstruct(A, B, phase + (istep - 1) * h.dt / PERIOD)
            st = o.step(st, istep, bool(mode))
        ref = (st["u"], st["v"], st["p"])
        ev, ep = relL2(o, f, ref), np.abs(f[2] - ref[2]).max() / np.abs(ref[2]).max()
        print("mode", mode, "phase", phase, "velocity relL2", ev, "pressure", ep)
        assert ev < 1e-9
        assert ep < 1e-5
    finally:
        h.close()
        o.set_baseflow(case6.ub)


@pytest.mark.parametrize("endtime,parity", [(0.15, 0), (0.16, 1)])
def test_full_spectrum_equals_the_stored_orbit(endtime, parity):
    """set_orbit_fourier with every harmonic (nmodes = nsteps // 2; even nsteps carries the Nyquist term) against set_orbit from the
    shedding state: the same integration bit for bit, and direct and adjoint maps that differ by the rounding of the
    reconstructed base flow only.  Then what the stored orbit cannot do: a map longer than the orbit."""
    from nekstab_amd import mesh, seed
    from nekstab_amd.capi import NekStabHip, NskError
    from nekstab_amd.quadrature import gauss_legendre, gauss_lobatto_legendre, interp_matrix
    z = np.load(os.path.join(GOLDEN, "cylinder_upo.npz"))
    case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6, endtime=endtime)
    case.ub[:] = z["u"]
    J = interp_matrix(gauss_lobatto_legendre(6)[0], gauss_legendre(4)[0])
    q0 = (z["u"][0], z["u"][1], J @ z["p"] @ J.T)
    # hip6's tolerances; its iteration caps (120 / 48) are sized for a smooth eigenmode and do not let the first steps of the
    # noise seed, which is far from solenoidal, reach 1e-13: the caps of the hexahedral orbit test instead
    kw = dict(HIP6, max_helm_iter=400, max_pres_iter=192)
    hs = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **kw)
    hf = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **kw)
    try:
        a0, ae, b0, be = hs.alloc(2) + hf.alloc(2)
        hs.upload(a0, *q0); hf.upload(b0, *q0)
        hs.set_orbit(a0, spng_str=1.7, end=ae)
        n = hs.nsteps
        assert n % 2 == parity and n >= 16, n                   # one case per parity: a mesh change must not drop one silently
        with pytest.raises(NskError) as e:
            hf.set_orbit_fourier(b0, n // 2 + 1, spng_str=1.7)
        assert e.value.code == -1
        amp = hf.set_orbit_fourier(b0, n // 2, spng_str=1.7, end=be)
        assert hf.nsteps == n and hf.dt == hs.dt and amp.shape == (2 * (n // 2) + 1,) and np.all(np.isfinite(amp)) and amp[0] > 0
        assert hf.get_orbit_modes() == (n // 2, endtime)
        assert _bits(hs.download(ae), hf.download(be))
        qx, qy = seed.add_noise(case)
        vs, fs, vf, ff = hs.alloc(2) + hf.alloc(2)
        hs.upload(vs, qx, qy, np.zeros(hs.npres)); hs.scal(vs, 1.0 / hs.norm(vs))
        hf.upload(vf, *hs.download(vs))
        for mode in (0, 1):
            hs.matvec(fs, vs, mode); hf.matvec(ff, vf, mode)
            r = hs.download(fs)
            hs.upload(a0, *hf.download(ff))
            err = _rel(hs, a0, fs)
            print("nsteps", n, "mode", mode, "Fourier (full spectrum) vs stored orbit: relL2", err, "|f|", np.abs(r[0]).max())
            assert err < 1e-9
        hs.set_nsteps(n + 5); hf.set_nsteps(n + 5)
        hf.matvec(ff, vf, 0)
        assert np.all(np.isfinite(hf.download(ff)[0]))
        with pytest.raises(NskError):
            hs.matvec(fs, vs, 0)
    finally:
        hs.close(); hf.close()


def test_truncation_on_the_shedding_orbit():
    """The real 795-step vortex-shedding orbit (settings of test_floquet_multipliers) kept as 8 harmonics; get_orbit_modes, then
    set_orbit_modes with the first 2, 4, 8 of them (no re-integration) and one direct map of the noise seed over the period
    for each, against the stored orbit's.  Measured on the MI355X (relative L2 distance from the stored-orbit map):
    err(2) = 4.18e-3, err(4) = 2.01e-4, err(8) = 2.26e-5 (|mode k| falls from 2.66 at k = 1 to 1.1e-3 at k = 8; three harmonics hold
    99 % of the amplitude sum); the bound on err(8) is ten times its measured value (the solves stop at different iterates at
    the loose production tolerance)."""
    from nekstab_amd import fourier, mesh, seed
    from nekstab_amd.capi import NekStabHip
    from nekstab_amd.quadrature import gauss_legendre, gauss_lobatto_legendre, interp_matrix
    z = np.load(os.path.join(GOLDEN, "cylinder_upo.npz"))
    T = float(z["period"])
    case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6, endtime=T)
    case.ub[:] = z["u"]
    kw = dict(tol_helm=1e-11, tol_pres=1e-2, tol_relative=1, nproj=8, max_helm_iter=150, max_pres_iter=48)
    J = interp_matrix(gauss_lobatto_legendre(6)[0], gauss_legendre(4)[0])
    q0 = (z["u"][0], z["u"][1], J @ z["p"] @ J.T)
    hs = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **kw)
    hf = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **kw)
    try:
        a0, b0 = hs.alloc(1) + hf.alloc(1)
        hs.upload(a0, *q0); hf.upload(b0, *q0)
        hs.set_orbit(a0, spng_str=1.7)
        amp = hf.set_orbit_fourier(b0, 8, spng_str=1.7)
        assert hs.nsteps == 795 and hf.nsteps == 795
        rep = fourier.amplitude_report(amp)
        print("amplitudes |mode k|, k = 0..8:", rep["ampl"], "share", rep["share"], "m99", rep["m99"])
        assert np.all(np.diff(rep["ampl"][1:]) < 0)
        A, B = hf.alloc(9), hf.alloc(8)
        assert hf.get_orbit_modes(A, B) == (8, T)
        qx, qy = seed.add_noise(case)
        vs, fs, vf, ff = hs.alloc(2) + hf.alloc(2)
        hs.upload(vs, qx, qy, np.zeros(hs.npres)); hs.scal(vs, 1.0 / hs.norm(vs))
        hf.upload(vf, *hs.download(vs))
        hs.matvec(fs, vs, 0)
        hf.upload(b0, *hs.download(fs))                          # the stored-orbit map, on the Fourier context
        err = {}
        for m in (2, 4, 8):
            hf.set_orbit_modes(A[:m + 1], B[:m], T)
            assert hf.nsteps == 795 and abs(hf.dt - hs.dt) < 1e-15, (m, hf.nsteps, hf.dt, hs.dt)
            hf.matvec(ff, vf, 0)
            err[m] = _rel(hf, ff, b0)
            print("harmonics", m, ": |map - stored-orbit map| / |stored-orbit map| =", err[m])
        assert err[8] < err[2]
        assert err[8] < 10 * MEASURED_E8
    finally:
        hs.close(); hf.close()



@pytest.mark.parametrize("lx1", [6, 8])
def test_hexahedra(lx1):
    """The cylinder extruded over two periodic layers, as test_time_periodic_base_flow_on_hexahedra_equals_the_quadrilateral_path
    sets it up (lx1 = 6: LDS convection kernels, lx1 = 8: the matrix-core one).  (a) the synthetic modes extruded with w = 0:
    hexahedral direct and adjoint maps over six steps equal the quadrilateral ones plane by plane, to that test's bounds.
    (b) modes with a z-invariant third component, one step of dt = endtime = 1e-3 at phase 0 and 0.37: equal to a steady
    hexahedral context whose base flow is np_reconstruct at that phase."""
    from nekstab_amd import fourier, mesh, mesh3d, seed
    from nekstab_amd.capi import NekStabHip
    kw = dict(tol_helm=1e-12, tol_pres=1e-7, tol_relative=1, nproj=0, max_helm_iter=400, max_pres_iter=192)
    nz, lz = 2, 0.5
    c2 = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), lx1, endtime=0.4)
    c3 = mesh3d.extrude_case(c2, nz, lz, periodic=True)
    A, B = _synthetic_modes(c2.ub, c2.x)
    qx, qy = seed.add_noise(c2)
    h2 = NekStabHip(c2, c2.meta["vert"], c2.meta["nvert"], **kw)
    h3 = NekStabHip(c3, c3.meta["vert"], c3.meta["nvert"], **kw)
    try:
        h2.set_orbit_modes(*_upload_modes2(h2, A, B), PERIOD)
        h3.set_orbit_modes(*_upload_modes3(h3, A, B, nz), PERIOD)
        assert h3.nsteps == h2.nsteps and abs(h3.dt - h2.dt) < 1e-15
        h2.set_nsteps(6); h3.set_nsteps(6)
        v2, f2 = h2.alloc(2); v3, f3 = h3.alloc(2)
        h2.upload(v2, qx, qy, np.zeros(h2.npres))
        h3.upload3(v3, mesh3d.extrude_field(qx, nz), mesh3d.extrude_field(qy, nz), np.zeros(c3.x.shape), np.zeros(h3.npres))
        for mode in (0, 1):
            h2.matvec(f2, v2, mode); h3.matvec(f3, v3, mode)
            r2 = h2.download(f2); r3 = h3.download3(f3)
            sc = max(np.abs(r2[0]).max(), np.abs(r2[1]).max())
            err = max(np.abs(r3[k] - mesh3d.extrude_field(r2[k], nz)).max() for k in range(2)) / sc
            print("lx1", lx1, "mode", mode, "hexahedral vs quadrilateral map over the Fourier orbit:", err, "w", np.abs(r3[2]).max() / sc)
            assert err < 1e-6 and np.abs(r3[2]).max() < 1e-7 * sc
    finally:
        h2.close(); h3.close()
    # (b) the third component
    tol = dict(tol_helm=1e-13, tol_pres=1e-13, tol_relative=0, nproj=0, max_helm_iter=400, max_pres_iter=192)
    c2 = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), lx1, endtime=1e-3)
    c3 = mesh3d.extrude_case(c2, nz, lz, periodic=True)
    u = c2.ub
    w = np.stack([0.2 * u[0] * np.cos(0.05 * c2.x), 0.1 * u[1], 0.05 * u[0] * np.sin(0.1 * c2.x), 0.02 * u[0], 0.03 * u[1]])
    A, B = _synthetic_modes(u, c2.x, w)
    hf = NekStabHip(c3, c3.meta["vert"], c3.meta["nvert"], **tol)
    hs = NekStabHip(c3, c3.meta["vert"], c3.meta["nvert"], **tol)
    try:
        hf.set_orbit_modes(*_upload_modes3(hf, A, B, nz), PERIOD)
        vf, ff = hf.alloc(2); vs, fs, ub = hs.alloc(3)
        ex = lambda f: mesh3d.extrude_field(f, nz)
        # a smooth three-component perturbation that varies in z, at unit norm (the noise seed does not reach the absolute
        # tolerance within the iteration caps at lx1 = 8)
        m3 = ex(c2.mask)
        q = (np.sin(c3.x) * m3, np.cos(0.5 * c3.x) * m3, np.sin(c3.x) * np.cos(2.0 * np.pi * c3.z / lz) * m3, np.zeros(hf.npres))
        hs.upload3(vs, *q); hs.scal(vs, 1.0 / hs.norm(vs))
        hf.upload3(vf, *hs.download3(vs))
        for phase in (0.0, 0.37):
            U = fourier.np_reconstruct(A, B, phase)
            hs.upload3(ub, ex(U[0]), ex(U[1]), ex(U[2]), np.zeros(hs.npres))
            hs.set_baseflow(ub)
            hf.set_option("orbit_phase", phase)
            assert hf.nsteps == 1 and hs.nsteps == 1 and hf.dt == 1e-3 and hs.dt == 1e-3
            for mode in (0, 1):
                hf.matvec(ff, vf, mode); hs.matvec(fs, vs, mode)
                hs.upload3(ub, *hf.download3(ff))
                err = _rel(hs, ub, fs)
                print("lx1", lx1, "phase", phase, "mode", mode, "one step, Fourier vs steady hexahedral context: relL2", err)
                assert err < 1e-9
    finally:
        hf.close(); hs.close()


def test_refusals_and_the_way_back(case6, oracle6_nosolve, modes):
    from nekstab_amd.capi import NekStabHip, NskError
    from nekstab_amd.sharded import ShardGroup
    A, B = _synthetic_modes(case6.ub, case6.x)
    h = NekStabHip(case6, case6.meta["vert"], case6.meta["nvert"], **HIP6)
    s = NekStabHip(case6, case6.meta["vert"], case6.meta["nvert"], **HIP6)
    try:
        lib = h.lib
        with pytest.raises(NskError) as e:
            h.get_orbit_modes()
        assert e.value.code == -1 and "no Fourier orbit" in str(e.value)
        # shards refuse both setters
        g = ShardGroup(h, case6, 2)
        a = g.alloc(1)[0]
        arr = (C.c_void_p * 1)(a.parts[0])
        assert lib.nsk_set_orbit_fourier(g.ctx[0], a.parts[0], 0.0, 1, None, None) == -1 and b"shard" in lib.nsk_last_error()
        assert lib.nsk_set_orbit_modes(g.ctx[0], 0, 1.0, arr, None) == -1 and b"shard" in lib.nsk_last_error()
        g.free([a]); g.close()
        # Fourier orbit, a map over it, then back: the context maps as a fresh steady one, bit for bit
        va, vb = _upload_modes2(h, A, B)
        h.set_orbit_modes(va, vb, PERIOD)
        with pytest.raises(NskError):
            h.add_lane()                                         # nsk_clone refuses, as with a stored orbit
        for x in (-0.1, 1.0):
            with pytest.raises(NskError):
                h.set_option("orbit_phase", x)
        vq, vf = h.alloc(2); sq, sf = s.alloc(2)
        from tests.test_matvec_gpu import _mode
        q = _mode(oracle6_nosolve, modes, "dRe")                 # the perturbation of test_steps_vs_oracle: converges within hip6's caps
        h.upload(vq, *q); s.upload(sq, *q)
        h.set_nsteps(3)
        h.matvec(vf, vq, 0)
        fourier_map = h.download(vf)
        h.set_baseflow(va[0]); s.set_baseflow(va[0])             # A_0 = the case's base flow
        with pytest.raises(NskError):
            h.get_orbit_modes()
        h.set_nsteps(5); s.set_nsteps(5)
        h.matvec(vf, vq, 0); s.matvec(sf, sq, 0)
        assert _bits(h.download(vf), s.download(sf))
        assert not _bits(fourier_map, s.download(sf))
    finally:
        h.close(); s.close()
