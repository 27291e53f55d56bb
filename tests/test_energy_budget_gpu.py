"""The stability energy budget on the device (nsk_energy_budget, core/postproc.f:657-872, uparam(1) = 4.1) against the numpy
restatement (nekstab_amd/sensitivity.np_energy_budget), and the uparam(1) = 4.0 driver (budget, wavemaker, bf_sensitivity)."""
import ctypes as C
import os

import numpy as np
import pytest

from nekstab_amd import mesh, mesh3d, nekio
from nekstab_amd import sensitivity as S
from nekstab_amd.capi import NekStabHip, NskError

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


def _upload(h, fields):
    vecs = h.alloc(len(fields))
    for v, u in zip(vecs, fields):
        S.upload_velocity(h, v, u)
    return vecs


def _run(h, ub, dRe, dIm):
    """Device budget with every output: (integrals, prod [ndim, ndim, ...], diss field, diss vector's other entries)."""
    nd = h.ndim
    v = _upload(h, (ub, dRe, dIm))
    outs = h.alloc(nd + 1)
    try:
        I = h.energy_budget(*v, prod=outs[:nd], diss=outs[nd])
        prod = np.array([S.download_velocity(h, o) for o in outs[:nd]])
        dv = h.download3(outs[nd]) if nd == 3 else h.download(outs[nd])
        pp = [(h.download3(o) if nd == 3 else h.download(o))[nd] for o in outs[:nd]]
    finally:
        h.free(v + outs)
    return I, prod, np.asarray(dv[0]), [np.asarray(a) for a in dv[1:]] + pp


def _check(I, prod, diss, ref):
    for c in range(prod.shape[0]):
        for j in range(prod.shape[1]):
            assert _rel(prod[c, j], ref["prod"][c, j]) <= 1e-12, (c, j)
    assert _rel(diss, ref["diss"]) <= 1e-12
    assert np.max(np.abs(I - ref["integrals"])) <= 1e-12 * np.max(np.abs(ref["integrals"])), (I, ref["integrals"])


@pytest.fixture(scope="module", params=[6, 8], ids=["lx6", "lx8"])
def ctx2(request):
    lx1 = request.param
    case = _case(lx1)
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **KW)
    yield lx1, case, h
    h.close()


def test_cylinder_budget_matches_numpy(ctx2):
    """Production fields, dissipation field and the 10 integrals of the committed mode; the other entries of the outputs are 0;
    signs of the cylinder's budget (P[1][2] feeds the instability, viscosity dissipates, the mode grows)."""
    lx1, case, h = ctx2
    dRe, dIm = _modes(lx1)[:2]
    ref = S.np_energy_budget(S.NpGeom(case), case.ub, dRe, dIm, 1.0 / case.re)
    I, prod, diss, rest = _run(h, case.ub, dRe, dIm)
    print(f"lx1 = {lx1}: energy budget {np.array2string(I, precision=4)}, sum {I.sum():.4e}")
    _check(I, prod, diss, ref)
    assert all(not np.any(a) for a in rest)
    assert np.all(I[[2, 5, 6, 7, 8]] == 0.0)
    assert I[1] > 0 and I[9] < 0 and I.sum() > 0


@pytest.mark.parametrize("lx1", [10, 12])
def test_quadrilaterals_higher_orders_match_numpy(lx1):
    case = _case(lx1)
    dRe, dIm = _modes(lx1)[:2]
    ref = S.np_energy_budget(S.NpGeom(case), case.ub, dRe, dIm, 1.0 / case.re)
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **KW)
    try:
        I, prod, diss, _ = _run(h, case.ub, dRe, dIm)
    finally:
        h.close()
    _check(I, prod, diss, ref)


@pytest.mark.parametrize("lx1", [6, 8, 10])
def test_hexahedra_extruded_cylinder_equals_2d(lx1, tmp_path):
    """z-extruded cylinder (two periodic layers, length 1): every z plane of the 3-D fields is the 2-D field, the entries of the
    third component and direction are 0, each integral is the 2-D one times the extrusion length (the mode's norm, and with it
    the 1 / alpha^2 of the budget, carries the same factor, which is 1 here).  At lx1 = 6 the driver writes three KIN files."""
    case = _case(lx1)
    nz, lz, n = 2, 1.0, lx1
    c3 = mesh3d.extrude_case(case, nz, lz)
    dRe, dIm = _modes(lx1)[:2]
    ref = S.np_energy_budget(S.NpGeom(case), case.ub, dRe, dIm, 1.0 / case.re)
    ext = lambda a: np.array([mesh3d.extrude_field(a[0], nz), mesh3d.extrude_field(a[1], nz), np.zeros((c3.nel, n, n, n))])
    h = NekStabHip(c3, c3.meta["vert"], c3.meta["nvert"], **KW)
    try:
        I, prod, diss, rest = _run(h, ext(case.ub), ext(dRe), ext(dIm))
        if lx1 == 6:
            v = _upload(h, (ext(case.ub), ext(dRe), ext(dIm)))
            I2, total, _ = S.energy_budget(h, *v, outdir=str(tmp_path), session="1cyl")
            h.free(v)
            np.testing.assert_array_equal(I2, I)
            assert total == float(np.sum(I))
            for c in range(3):
                f = nekio.read_fld(str(tmp_path / S.fld_name("KIN", "1cyl", c + 1)))
                assert f.u.shape == (3, c3.nel, n, n, n)
                np.testing.assert_array_equal(f.u, prod[c])
            assert not os.path.exists(tmp_path / S.fld_name("KIN", "1cyl", 4))
    finally:
        h.close()
    s = np.max(np.abs(ref["prod"]))
    for c in range(3):
        for j in range(3):
            a = prod[c, j].reshape(nz, case.nel, n, n, n)
            if c < 2 and j < 2:
                for kz in range(nz):
                    for lev in range(n):
                        assert np.max(np.abs(a[kz, :, lev] - ref["prod"][c, j])) <= 1e-12 * s, (c, j, kz, lev)
            else:
                assert np.max(np.abs(a)) <= 1e-12 * s, (c, j)
    d = diss.reshape(nz, case.nel, n, n, n)
    sd = np.max(np.abs(ref["diss"]))
    for kz in range(nz):                     # second derivatives, pointwise: rounding reaches 4e-12 of the largest |D| at lx1 = 10
        for lev in range(n):
            assert _rel(d[kz, :, lev], ref["diss"]) <= 1e-12 and np.max(np.abs(d[kz, :, lev] - ref["diss"])) <= 1e-11 * sd, (kz, lev)
    assert all(not np.any(a) for a in rest)
    sI = np.max(np.abs(ref["integrals"]))
    assert np.max(np.abs(I - lz * ref["integrals"])) <= 1e-12 * sI, (I, ref["integrals"])
    assert np.max(np.abs(I[[2, 5, 6, 7, 8]])) <= 1e-12 * sI


def test_hexahedra_genuinely_3d_field_matches_numpy():
    """Deformed box, smooth base flow and mode with every derivative non-zero: all 10 integrals non-zero, fields and integrals
    as numpy's."""
    ubf = lambda x, y, z: np.stack([1.0 - 0.3 * y * y + 0.1 * np.sin(x + z), 0.2 * np.cos(x) * y + 0.1 * z,
                                    0.15 * np.sin(y + 0.5 * z + 0.4 * x)])
    c = mesh3d.box_case_3d(2, 2, 2, 6, lengths=(2.0, 1.0, 0.8), outflow_xmax=True, re=40.0, endtime=0.05, warp=0.06, ub_func=ubf)
    x, y, z = c.x, c.y, c.z
    f = lambda a, b, cc, d: np.sin(a * x + 0.3) * np.cos(b * y - 0.2) * np.exp(cc * z) + d * x * y * z
    dRe = np.array([f(1.1, 0.7, 0.3, 0.2), f(0.5, 1.3, -0.4, 0.1), f(0.9, 0.4, 0.8, -0.3)])
    dIm = np.array([f(0.6, 1.0, 0.5, 0.0), f(1.4, 0.2, 0.1, 0.4), f(0.3, 0.9, -0.6, 0.2)])
    ub = ubf(x, y, z)
    ref = S.np_energy_budget(S.NpGeom(c), ub, dRe, dIm, 1.0 / 40.0)
    assert np.min(np.abs(ref["integrals"])) > 1e-4 * np.max(np.abs(ref["integrals"])), ref["integrals"]
    h = NekStabHip(c, c.meta["vert"], c.meta["nvert"], **KW)
    try:
        I, prod, diss, rest = _run(h, ub, dRe, dIm)
    finally:
        h.close()
    _check(I, prod, diss, ref)
    assert all(not np.any(a) for a in rest)


def test_scale_invariance_inputs_untouched_and_reproducible(hip6, case6):
    """dRe, dIm scaled by 3: the same budget to 1e-13; the inputs keep their bits; two calls give the same bits, with and
    without field outputs."""
    h = hip6
    dRe, dIm = _modes(6)[:2]
    v = _upload(h, (case6.ub, dRe, dIm))
    w = _upload(h, (case6.ub, 3.0 * dRe, 3.0 * dIm))
    outs = h.alloc(3)
    try:
        before = [h.download(a) for a in v]
        I1 = h.energy_budget(*v, prod=outs[:2], diss=outs[2])
        f1 = [h.download(o) for o in outs]
        after = [h.download(a) for a in v]
        for x0, x1 in zip(before, after):
            for a0, a1 in zip(x0, x1):
                assert np.array_equal(a0, a1)
        I2 = h.energy_budget(*v, prod=outs[:2], diss=outs[2])
        np.testing.assert_array_equal(I1, I2)
        for o, x0 in zip(outs, f1):
            for a0, a1 in zip(x0, h.download(o)):
                assert np.array_equal(a0, a1)
        np.testing.assert_array_equal(h.energy_budget(*v), I1)            # no field outputs: the same sums
        I3 = h.energy_budget(*w)
        assert np.max(np.abs(I3 - I1)) <= 1e-13 * np.max(np.abs(I1)), (I3, I1)
    finally:
        h.free(v + w + outs)


def test_refusals(hip6, case6):
    from nekstab_amd.sharded import ShardGroup
    h, lib = hip6, hip6.lib
    ints = np.zeros(10)
    ip = ints.ctypes.data_as(C.POINTER(C.c_double))
    g = ShardGroup(h, case6, 2)
    try:
        a = g.alloc(1)[0]
        p = a.parts[0]
        assert lib.nsk_energy_budget(g.ctx[0], p, p, p, None, None, ip) == -1
        assert b"single-rank" in lib.nsk_last_error()
        g.free([a])
    finally:
        g.close()
    ub, dRe, dIm, o1, o2, z = h.alloc(6)
    try:
        S.upload_velocity(h, ub, case6.ub)
        dr, di = _modes(6)[:2]
        S.upload_velocity(h, dRe, dr)
        S.upload_velocity(h, dIm, di)
        h.zero(z)
        assert lib.nsk_energy_budget(h.ctx, ub, dRe, dIm, None, None, None) == -1                    # integrals = NULL
        for prod, diss in (([o1, o1], None), ([o1, o2], o1), ([o1, o2], dRe), ([ub, o2], None), (None, dIm)):
            with pytest.raises(NskError) as e:
                h.energy_budget(ub, dRe, dIm, prod=prod, diss=diss)
            assert e.value.code == -1
        with pytest.raises(NskError) as e:
            h.energy_budget(ub, z, z)
        assert e.value.code == -1 and "zero" in str(e.value)
        np.testing.assert_array_equal(S.download_velocity(h, dRe), dr)                             # refused calls wrote nothing
    finally:
        h.free([ub, dRe, dIm, o1, o2, z])


def test_postprocess_writes_every_file_and_leaves_the_modes(hip6, case6, tmp_path):
    """uparam(1) = 4.0: KIN, wm_, tr_ .. si_ files; its wm_ and sr_ are those of wave_maker / bf_sensitivity run alone on freshly
    uploaded modes (the budget left the modes untouched)."""
    h = hip6
    modes = _modes(6)
    v = _upload(h, [case6.ub] + modes)
    try:
        out = S.postprocess(h, *v, outdir=str(tmp_path), session="1cyl")
        for vec, u in zip(v, [case6.ub] + modes):                                                # the caller's vectors
            np.testing.assert_array_equal(S.download_velocity(h, vec), u)
    finally:
        h.free(v)
    names = [S.fld_name("KIN", "1cyl", 1), S.fld_name("KIN", "1cyl", 2)] + \
        [S.fld_name(k + "_", "1cyl") for k in ("wm", "tr", "ti", "pr", "pi", "sr", "si")]
    for nm in names:
        assert os.path.exists(tmp_path / nm), nm
    assert not os.path.exists(tmp_path / S.fld_name("KIN", "1cyl", 3))
    for c in range(2):
        f = nekio.read_fld(str(tmp_path / S.fld_name("KIN", "1cyl", c + 1)))
        assert f.u.shape == (2, case6.nel, 1, 6, 6)
        np.testing.assert_array_equal(f.u[:, :, 0], out["prod"][c])
    ref = S.np_energy_budget(S.NpGeom(case6), case6.ub, modes[0], modes[1], 1.0 / case6.re)
    assert np.max(np.abs(out["integrals"] - ref["integrals"])) <= 1e-12 * np.max(np.abs(ref["integrals"]))
    assert out["budget_sum"] == float(np.sum(out["integrals"]))
    d = _upload(h, modes)
    try:
        wm, _ = S.wave_maker(h, *d)
    finally:
        h.free(d)
    d = _upload(h, modes)
    try:
        sens, _ = S.bf_sensitivity(h, *d)
    finally:
        h.free(d)
    np.testing.assert_array_equal(out["wm"], wm)
    np.testing.assert_array_equal(out["sr"], sens["sr"])
    np.testing.assert_array_equal(nekio.read_fld(str(tmp_path / S.fld_name("wm_", "1cyl"))).t[:, 0], wm)
    np.testing.assert_array_equal(nekio.read_fld(str(tmp_path / S.fld_name("sr_", "1cyl"))).u[:, :, 0], sens["sr"])
