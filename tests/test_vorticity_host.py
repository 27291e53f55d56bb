"""Vorticity of eigenmodes (comp_vort3, the Rv files of outpost_ks), host side: the numpy restatement against the reference's
own dRv file and against an exact curl, and the file naming of outpost_ks.  No GPU."""
import os
from types import SimpleNamespace

import numpy as np

from nekstab_amd import mesh, mesh3d, nekio, outpost
from nekstab_amd import sensitivity as S
from tests.conftest import GOLDEN


def _wrel(g, a, b):
    """bm1-weighted relative L2 distance of a from b"""
    return np.sqrt(np.sum(g.bm1 * (a - b) ** 2) / np.sum(g.bm1 * b ** 2))


def test_np_vorticity_matches_the_reference_file_and_the_bound_discriminates(case6):
    """np_vorticity of the reference's leading direct mode (lx1 = 6) against the vorticity the reference wrote for it.  Both
    files are fp32, which leaves 2.14e-6; the bound 1e-5 is 5x that.  The two plausible wrong averages -- multiplicity-weighted
    (dsavg) and none (element-local) -- measure 4.6e-5 and 2.0e-3: both must stay outside 3e-5."""
    g = S.NpGeom(case6)
    u = np.load(os.path.join(GOLDEN, "cylinder_modes.npz"))["dRe_u"].astype(np.float64)
    fx = np.load(os.path.join(GOLDEN, "cylinder_vorticity.npz"))
    ref = fx["w"].astype(np.float64)
    assert fx["w"].dtype == np.float32 and ref.shape == (1996, 6, 6) and bool(fx["vy_is_zero"])
    w = S.np_vorticity(g, u)
    assert w.shape == (1, 1996, 6, 6)
    err = _wrel(g, w[0], ref)
    local = g.grad(u[1])[0] - g.grad(u[0])[1]
    e_avg, e_loc = _wrel(g, g.dsavg(local), ref), _wrel(g, local, ref)
    print(f"weighted relative L2 against the reference's dRv file: mass-weighted {err:.3e} (max abs {np.abs(w[0] - ref).max():.2e}, "
          f"field max {np.abs(ref).max():.3f}), dsavg {e_avg:.2e}, element-local {e_loc:.2e}")
    assert err <= 1e-5
    assert e_avg > 3e-5 and e_loc > 3e-5


def test_np_vorticity_is_exact_for_a_cubic_field_on_affine_hexahedra():
    c = mesh3d.box_case_3d(2, 3, 2, 6, lengths=(2.0, 1.0, 0.8), warp=0.0)
    x, y, z = c.x, c.y, c.z
    u = np.array([x * y * z + 0.5 * y ** 3 - 0.3 * x * z ** 2 + 0.2 * x ** 2 * y,
                  0.7 * x ** 3 - x * y ** 2 + 0.4 * y * z ** 2 + z,
                  0.6 * z ** 3 + x ** 2 * z - 0.8 * x * y * z + 0.1 * y ** 2])
    # curl = (dw/dy - dv/dz, du/dz - dw/dx, dv/dx - du/dy)
    exact = np.array([(-0.8 * x * z + 0.2 * y) - (0.8 * y * z + 1.0),
                      (x * y - 0.6 * x * z) - (2.0 * x * z - 0.8 * y * z),
                      (2.1 * x ** 2 - y ** 2) - (x * z + 1.5 * y ** 2 + 0.2 * x ** 2)])
    w = S.np_vorticity(S.NpGeom(c), u)
    assert w.shape == exact.shape
    err = np.max(np.abs(w - exact), axis=(1, 2, 3, 4)) / np.max(np.abs(exact))
    print("max error of the three components over the largest magnitude:", err)
    assert np.all(err <= 1e-11)


class _StandIn:
    """the vector interface outpost_ks needs, on numpy arrays: a vector is a dict of velocity u [2, nel, n, n] and pressure"""

    def __init__(self, case):
        self.case, self.nsteps, self.dt, self.calls = case, 100, 0.01, []
        self.geom = S.NpGeom(case)

    def alloc(self, n=1):
        c = self.case
        return [dict(u=np.zeros((2, c.nel, c.lx1, c.lx1)), p=np.zeros((c.nel, c.lx1 - 2, c.lx1 - 2))) for _ in range(n)]

    def free(self, vecs):
        pass

    def basis_gemv(self, Q, y, re, im=None):
        re["u"] = sum(np.real(c) * q["u"] for c, q in zip(y, Q))
        im["u"] = sum(np.imag(c) * q["u"] for c, q in zip(y, Q))

    def dot(self, a, b):
        return self.geom.inner(a["u"], b["u"])

    def scal(self, a, s):
        a["u"] = a["u"] * s

    def download(self, v):
        return v["u"][0], v["u"][1], v["p"]

    def vorticity(self, w, q):
        self.calls.append(q)
        w["u"] = np.array([S.np_vorticity(self.geom, q["u"])[0], np.zeros_like(q["u"][0])])
        w["p"] = np.zeros_like(q["p"])


def test_outpost_ks_names_the_rv_files_as_the_reference_and_writes_none_by_default(tmp_path):
    case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6)
    be = _StandIn(case)
    rng = np.random.default_rng(3)
    k = 3
    Q = be.alloc(k)
    for q in Q:
        q["u"] = rng.standard_normal(q["u"].shape)
    vals = np.array([0.9 + 0.3j, 0.9 - 0.3j, 0.5 + 0.0j])
    res = SimpleNamespace(H=np.zeros((k + 1, k)), Q=Q, vals=vals, vecs=np.linalg.qr(rng.standard_normal((k, k)) + 1j * rng.standard_normal((k, k)))[0],
                          residual=np.array([1e-9, 1e-9, 1e-2]), schur_cnt=0)
    d0, d1 = tmp_path / "plain", tmp_path / "vor"
    w0 = outpost.outpost_ks(be, res, case, str(d0), eigen_tol=1e-6)
    assert not be.calls and not [f for f in os.listdir(d0) if "Rv" in f]
    assert [os.path.basename(f) for f in w0] == ["dRe1cyl0.f00001", "dIm1cyl0.f00001", "dRe1cyl0.f00002", "dIm1cyl0.f00002"]
    w1 = outpost.outpost_ks(be, res, case, str(d1), eigen_tol=1e-6, ifvor=True)
    assert [os.path.basename(f) for f in w1] == [os.path.basename(f) for f in w0] + ["dRv1cyl0.f00001", "dRv1cyl0.f00002"]
    assert sorted(set(os.listdir(d1)) - set(os.listdir(d0))) == ["dRv1cyl0.f00001", "dRv1cyl0.f00002"]
    for i in (1, 2):
        rv, re = nekio.read_fld(str(d1 / ("dRv1cyl0.f%05d" % i))), nekio.read_fld(str(d1 / ("dRe1cyl0.f%05d" % i)))
        assert rv.rdcode == "XU" and re.rdcode == "XUP" and rv.p is None and rv.t is None
        assert (rv.time, rv.istep, rv.wdsize) == (re.time, re.istep, re.wdsize) == (float(i), 101, 4)
        ref = S.np_vorticity(be.geom, re.u[:, :, 0])[0]              # the Re file's own (fp32-rounded) velocity
        assert np.max(np.abs(rv.u[0, :, 0] - ref)) <= 1e-4 * np.max(np.abs(ref)) and not np.any(rv.u[1])
        np.testing.assert_array_equal(rv.x, re.x)
    for a, b in zip(w0, w1):                                         # the Re / Im files do not depend on the switch
        assert open(a, "rb").read() == open(b, "rb").read()
