"""Sensitivity post-processing of direct and adjoint modes, restating core/sensitivity.f (uparam(1) = 4.x):

    energy_budget                    4.1   stability_energy_budget (core/postproc.f:657-872): production and dissipation
    wave_maker                       4.2   Giannetti & Luchini (2007), structural sensitivity |d| |a|
    bf_sensitivity                   4.3   Marquet, Sipp & Jacquin (2008), sensitivity to base-flow modifications
    ts_steady_force_sensitivity      4.41 / 4.42   sensitivity to a steady force: GMRES on (I - exp(L^+ T))
    delta_forcing                    4.43  eigenvalue drift under a steady force proportional to the base flow (eq. 5.1)
    postprocess                      4.0   energy_budget, wave_maker, bf_sensitivity in the reference's order (core/usr_extra.f)

The fields are computed on the device (nsk_energy_budget, nsk_biorthogonalize, nsk_wavemaker, nsk_bf_sensitivity,
nsk_forced_map; on element shards their nsk_group_* twins: every driver below takes a ``sharded.ShardGroup`` in place of the
single-rank context and writes the same files); delta_forcing is pointwise and stays on the host.  Output files carry the reference's prefixes (KIN, wm_, tr_,
ti_, pr_, pi_, sr_, si_, fsr, fsi, dfr) so that nekStab's own scripts read them.  ``np_*`` functions are the numpy
restatement the device is tested against; ``np_vorticity`` is that of nsk_vorticity (comp_vort3, the Rv files that
``outpost.outpost_ks(..., ifvor=True)`` writes), ``np_vortex_criteria`` with ``gll_filter_matrix`` that of nsk_vortex_criteria
(lambda2, Q, Omega of vortex_core: the vox / omg files of ``outpost.outpost_vox``).

Three departures from the reference, all deliberate:
  * in 3-D the transport term uses d v / d z where core/sensitivity.f:219, 222, 228, 231 read d w / d z (Marquet's formula;
    the two agree in 2-D and on z-invariant fields);
  * biorthogonalisation scales the direct mode's pressure with its velocity (the reference passes one shared pressure array);
  * the energy budget takes the mode divided by its norm, as the reference's comment says (core/postproc.f:703-707 multiplies
    by it): the budget does not depend on the mode's scale, and the two readings agree for a mode of unit norm.
"""
from __future__ import annotations

import os

import numpy as np

from . import nekio, newton
from .capi import NSK_ADJOINT, NSK_FORCE_SENSITIVITY
from .quadrature import deriv_matrix, gauss_legendre, gauss_lobatto_legendre, interp_matrix


def fld_name(prefix: str, session: str, num: int = 1) -> str:
    """Nek's outpost file name: prefix + session + '0.f' + 5-digit number (e.g. sr_1cyl0.f00001)."""
    return "%s%s0.f%05d" % (prefix, session, num)


# ----------------------------------------------------------------------------------------------------------------------
# mode files at another polynomial order (load_fld interpolates GLL -> GLL on read)
# ----------------------------------------------------------------------------------------------------------------------

def interp_gll(f: np.ndarray, lx_to: int, *, ndim: int = 2) -> np.ndarray:
    """(..., [nz,] ny, nx) element fields on GLL(lx_from) points -> GLL(lx_to), tensor-product interpolation per element."""
    lx_from = f.shape[-1]
    if lx_from == lx_to:
        return np.array(f, dtype=np.float64)
    J = interp_matrix(gauss_lobatto_legendre(lx_from)[0], gauss_lobatto_legendre(lx_to)[0])
    if ndim == 2:
        return np.einsum("ai,bj,...ji->...ba", J, J, f, optimize=True)
    return np.einsum("ai,bj,ck,...kji->...cba", J, J, J, f, optimize=True)


def gll_to_gauss(p: np.ndarray, lx1: int, *, ndim: int = 2) -> np.ndarray:
    """Pressure stored on GLL(lx_from) points (field files) -> the lx1 - 2 Gauss points of the state vector."""
    J = interp_matrix(gauss_lobatto_legendre(p.shape[-1])[0], gauss_legendre(lx1 - 2)[0])
    if ndim == 2:
        return np.einsum("ai,bj,...ji->...ba", J, J, p, optimize=True)
    return np.einsum("ai,bj,ck,...kji->...cba", J, J, J, p, optimize=True)


def load_mode(path: str, lx1: int):
    """A mode file (dRe / dIm / aRe / aIm ...) at order lx1, whatever order it was written at: (u [ndim, nel, ...], p on the
    lx1 - 2 Gauss points or None).  core/sensitivity.f reads lx1 = 6 direct and lx1 = 8 adjoint files in one case."""
    fld = nekio.read_fld(path)
    ndim = 3 if fld.nz > 1 else 2
    u = fld.u if ndim == 3 else fld.u[:, :, 0]
    u = interp_gll(u, lx1, ndim=ndim)
    p = None
    if fld.p is not None:
        p0 = fld.p if ndim == 3 else fld.p[:, 0]
        p = gll_to_gauss(p0, lx1, ndim=ndim)
    return u, p


# ----------------------------------------------------------------------------------------------------------------------
# numpy restatement (the yardstick of the device entries)
# ----------------------------------------------------------------------------------------------------------------------

class NpGeom:
    """GLL-mesh geometry of a case: mass matrix bm1 / bm1s, gradm1 and dsavg (Nek5000 restated in numpy)."""

    def __init__(self, case):
        self.ndim = int(getattr(case, "ndim", 2))
        n = case.lx1
        z, w = gauss_lobatto_legendre(n)
        self.D = deriv_matrix(z)
        self.gid = np.asarray(case.gid, dtype=np.int64)
        self.nglob = int(case.nglob)
        X = [np.asarray(case.x, dtype=np.float64), np.asarray(case.y, dtype=np.float64)]
        if self.ndim == 3:
            X.append(np.asarray(case.z, dtype=np.float64))
        J = np.array([self._drst(a) for a in X])          # J[a][r] = d x_a / d r_r
        if self.ndim == 2:
            self.jac = J[0][0] * J[1][1] - J[0][1] * J[1][0]
            inv = [[J[1][1], -J[0][1]], [-J[1][0], J[0][0]]]            # inv[r][a] * jac = d r_r / d x_a
        else:
            cof = lambda a, r: (J[(a + 1) % 3][(r + 1) % 3] * J[(a + 2) % 3][(r + 2) % 3]
                                - J[(a + 1) % 3][(r + 2) % 3] * J[(a + 2) % 3][(r + 1) % 3])
            self.jac = sum(J[0][r] * cof(0, r) for r in range(3))
            inv = [[cof(a, r) for a in range(3)] for r in range(3)]
        self.inv = [[inv[r][a] / self.jac for a in range(self.ndim)] for r in range(self.ndim)]
        W = w[:, None] * w[None, :] if self.ndim == 2 else w[:, None, None] * w[None, :, None] * w[None, None, :]
        self.bm1 = self.jac * W
        self.bm1s = np.where(np.asarray(case.spng) != 0.0, 0.0, self.bm1)
        self.mult = np.bincount(self.gid.ravel(), minlength=self.nglob)[self.gid]

    def _drst(self, f):
        D = self.D
        if self.ndim == 2:
            return [f @ D.T, np.einsum("jq,eqi->eji", D, f)]
        return [np.einsum("iq,ekjq->ekji", D, f), np.einsum("jq,ekqi->ekji", D, f), np.einsum("kq,eqji->ekji", D, f)]

    def grad(self, f):
        """gradm1: [d f / d x_a] on the element-local nodes."""
        dr = self._drst(f)
        return [sum(self.inv[r][a] * dr[r] for r in range(self.ndim)) for a in range(self.ndim)]

    def dsavg(self, f):
        g = np.bincount(self.gid.ravel(), weights=f.ravel(), minlength=self.nglob)[self.gid]
        return g / self.mult

    def inner(self, a, b, w=None):
        w = self.bm1s if w is None else w
        return float(sum(np.sum(x * w * y) for x, y in zip(a, b)))


def np_biorthogonalize(geom: NpGeom, dRe, dIm, aRe, aIm):
    """biorthogonalize (core/sensitivity.f:428-504) on velocity fields: returns (dRe, dIm, aRe, aIm, gamma, delta)."""
    s = 1.0 / np.sqrt(geom.inner(dRe, dRe) + geom.inner(dIm, dIm))
    dRe, dIm = np.asarray(dRe) * s, np.asarray(dIm) * s
    gamma = geom.inner(aRe, dRe) + geom.inner(aIm, dIm)
    delta = geom.inner(aRe, dIm) - geom.inner(aIm, dRe)
    den = gamma ** 2 + delta ** 2
    aRe, aIm = np.asarray(aRe), np.asarray(aIm)
    return dRe, dIm, (gamma * aRe - delta * aIm) / den, (gamma * aIm + delta * aRe) / den, gamma, delta


def np_wavemaker(dRe, dIm, aRe, aIm):
    return np.sqrt(np.sum(np.asarray(dRe) ** 2 + np.asarray(dIm) ** 2, axis=0)) * \
        np.sqrt(np.sum(np.asarray(aRe) ** 2 + np.asarray(aIm) ** 2, axis=0))


def np_bf_sensitivity(geom: NpGeom, dRe, dIm, aRe, aIm):
    """bf_sensitivity (core/sensitivity.f:93-284) on biorthogonalised velocity fields: dict of tr, ti, pr, pi, sr, si,
    each [ndim, nel, ...].  G[c][a] = dsavg(d u_c / d x_a)."""
    nd = geom.ndim
    G = {k: [[geom.dsavg(g) for g in geom.grad(m[c])] for c in range(nd)]
         for k, m in (("dRe", dRe), ("dIm", dIm), ("aRe", aRe), ("aIm", aIm))}
    tr = np.array([-sum(aRe[j] * G["dRe"][j][i] + aIm[j] * G["dIm"][j][i] for j in range(nd)) for i in range(nd)])
    ti = np.array([sum(aRe[j] * G["dIm"][j][i] - aIm[j] * G["dRe"][j][i] for j in range(nd)) for i in range(nd)])
    pr = np.array([sum(dRe[j] * G["aRe"][i][j] + dIm[j] * G["aIm"][i][j] for j in range(nd)) for i in range(nd)])
    pi = np.array([sum(dRe[j] * G["aIm"][i][j] - dIm[j] * G["aRe"][i][j] for j in range(nd)) for i in range(nd)])
    return dict(tr=tr, ti=ti, pr=pr, pi=pi, sr=tr + pr, si=ti + pi)


def np_energy_budget(geom: NpGeom, ub, dRe, dIm, nu):
    """stability_energy_budget (core/postproc.f:657-872) on velocity fields [ndim, nel, ...]: dict of
      prod       [ndim, ndim, nel, ...]   P[c][j] = -1/2 (uR_c uR_j + uI_c uI_j) d U_c / d x_j  (gradm1 of U, no dsavg)
      diss       [nel, ...]               D = 1/2 nu sum_j (uR_j Lap uR_j + uI_j Lap uI_j),  Lap a = sum_i dsavg(d/dx_i dsavg(d a/dx_i))
      integrals  [10]                     bm1-weighted sums of P[1][1..3], P[2][1..3], P[3][1..3], D (missing dimension: 0)
    with the mode divided by alpha = sqrt(||dRe||^2 + ||dIm||^2) (bm1s-weighted; the reference's comment, not its code)."""
    nd = geom.ndim
    alpha = np.sqrt(geom.inner(dRe, dRe) + geom.inner(dIm, dIm))
    uR, uI = np.asarray(dRe) / alpha, np.asarray(dIm) / alpha
    gU = [geom.grad(np.asarray(ub[c])) for c in range(nd)]
    prod = np.array([[-0.5 * (uR[c] * uR[j] + uI[c] * uI[j]) * gU[c][j] for j in range(nd)] for c in range(nd)])

    def lap(a):
        return sum(geom.dsavg(geom.grad(geom.dsavg(geom.grad(a)[i]))[i]) for i in range(nd))

    diss = 0.5 * nu * sum(uR[j] * lap(uR[j]) + uI[j] * lap(uI[j]) for j in range(nd))
    integrals = np.zeros(10)
    for c in range(nd):
        for j in range(nd):
            integrals[3 * c + j] = np.sum(geom.bm1 * prod[c, j])
    integrals[9] = np.sum(geom.bm1 * diss)
    return dict(prod=prod, diss=diss, integrals=integrals)


def np_vorticity(geom: NpGeom, u):
    """comp_vort3 as outpost_ks calls it (core/eigensolvers.f:632) on a velocity field [ndim, nel, ...]: element-local curl,
    times the unassembled mass bm1, summed over co-located nodes, divided by the assembled mass (no Dirichlet mask).
    Returns [1, nel, ...] in 2-D (d v / d x - d u / d y) and [3, nel, ...] in 3-D."""
    G = [geom.grad(np.asarray(u[c], dtype=np.float64)) for c in range(geom.ndim)]          # G[c][a] = d u_c / d x_a
    if geom.ndim == 2:
        curl = [G[1][0] - G[0][1]]
    else:
        curl = [G[2][1] - G[1][2], G[0][2] - G[2][0], G[1][0] - G[0][1]]
    dssum = lambda f: np.bincount(geom.gid.ravel(), weights=f.ravel(), minlength=geom.nglob)[geom.gid]
    mass = dssum(geom.bm1)
    return np.array([dssum(c * geom.bm1) / mass for c in curl])


def gll_filter_matrix(lx1: int, wght: float) -> np.ndarray:
    """The 1-D matrix of Nek5000's filter_s0(f, wght, 1, .) on the lx1 GLL points: F = Phi diag(1, ..., 1, 1 - wght) Phi^-1 with
    Phi[j][k] = phi_k(xi_j), phi_0 = L_0, phi_1 = L_1, phi_k = L_k - L_{k-2} (L: Legendre).  F leaves every polynomial of degree
    <= lx1 - 2 as it is and multiplies phi_{lx1-1} by 1 - wght; wght = 0 gives the identity exactly."""
    if not (np.isfinite(wght) and 0.0 <= wght <= 1.0):
        raise ValueError("wght must lie in [0, 1]")
    if wght == 0.0:
        return np.eye(lx1)
    z = gauss_lobatto_legendre(lx1)[0]
    L = np.polynomial.legendre.legvander(z, lx1 - 1)               # L[j][k] = L_k(xi_j)
    phi = L.copy()
    phi[:, 2:] -= L[:, :-2]
    diag = np.ones(lx1)
    diag[-1] = 1.0 - wght
    return np.linalg.solve(phi.T, (phi * diag).T).T


def np_vortex_criteria(geom: NpGeom, u, wght=0.5):
    """vortex_core('lambda2' / 'q' / 'omega') of nekStab_outpost (core/usr_extra.f:269-273) on a velocity field [ndim, nel, ...]:
    returns (lambda2, q, omega), each [nel, ...].  g[i][j] = d u_i / d x_j element-local (comp_gije), S and O its symmetric and
    antisymmetric parts, ndim x ndim:
      lambda2   the second largest eigenvalue of S S + O O (Jeong & Hussain): the middle of three, the smaller of two
      q         compute_secondInv (core/postproc.f:374-403): 3-D the sum of the principal 2 x 2 minors of g; 2-D
                (g11 + g22)^2 - 2 g12 g21 - g11^2 - g22^2, twice the determinant (twice the 3-D value of a z-invariant field)
      omega     compute_omega_jc (core/postproc.f:31-79): b / (a + b + 1e-5), a = (||S||_F^2)^2, b = (||O||_F^2)^2
    each then filtered element by element with ``gll_filter_matrix(lx1, wght)`` along every reference direction."""
    nd = geom.ndim
    g = np.array([geom.grad(np.asarray(u[c], dtype=np.float64)) for c in range(nd)])       # g[i][j]
    gm = np.moveaxis(g, (0, 1), (-2, -1))                                                   # [nel, ..., i, j]
    S, O = 0.5 * (gm + np.swapaxes(gm, -1, -2)), 0.5 * (gm - np.swapaxes(gm, -1, -2))
    lam = np.linalg.eigvalsh(S @ S + O @ O)[..., nd - 2]                                    # ascending: index nd - 2 is the second largest
    if nd == 3:
        q = (g[1][1] * g[2][2] - g[1][2] * g[2][1]) + (g[0][0] * g[1][1] - g[0][1] * g[1][0]) + (g[2][2] * g[0][0] - g[0][2] * g[2][0])
    else:
        q = (g[0][0] + g[1][1]) * (g[0][0] + g[1][1]) - 2 * g[0][1] * g[1][0] - g[0][0] * g[0][0] - g[1][1] * g[1][1]
    a, b = np.sum(S * S, axis=(-1, -2)) ** 2, np.sum(O * O, axis=(-1, -2)) ** 2
    om = b / (a + b + 1e-5)
    if wght == 0.0:
        return lam, q, om
    F = gll_filter_matrix(geom.D.shape[0], wght)

    def filt(f):
        if nd == 2:
            return np.einsum("ai,bj,eji->eba", F, F, f, optimize=True)
        return np.einsum("ai,bj,ck,ekji->ecba", F, F, F, f, optimize=True)

    return filt(lam), filt(q), filt(om)


def delta_forcing(ub, fsr, fsi, alpha=1.0):
    """delta_forcing (core/sensitivity.f, uparam(1) = 4.43): eigenvalue drift of a steady force alpha |U| U, pointwise:
    (delta_lambda, delta_omega) = (-alpha |U| fsr . U, alpha |U| fsi . U)."""
    ub, fsr, fsi = (np.asarray(a, dtype=np.float64) for a in (ub, fsr, fsi))
    work = np.sqrt(np.sum(ub ** 2, axis=0))
    return -alpha * work * np.sum(fsr * ub, axis=0), alpha * work * np.sum(fsi * ub, axis=0)


# ----------------------------------------------------------------------------------------------------------------------
# device drivers
# ----------------------------------------------------------------------------------------------------------------------

def upload_velocity(h, v, u, p=None):
    """u [ndim, nel, ...] (and p on the Gauss points, default 0) into the device vector v."""
    if p is None:
        p = np.zeros((h.nel,) + (h.lx2,) * h.ndim)
    if h.ndim == 3:
        h.upload3(v, u[0], u[1], u[2], p)
    else:
        h.upload(v, u[0], u[1], p)


def download_velocity(h, v):
    out = h.download3(v) if h.ndim == 3 else h.download(v)
    return np.array(out[:h.ndim])


def _coords(h):
    k = h._keep
    X = [k["x"], k["y"]] + ([k["z"]] if h.ndim == 3 else [])
    return np.array([np.asarray(a).reshape((h.nel,) + (h.lx1,) * h.ndim) for a in X])


def _write(h, path, *, u=None, t=None):
    """outpost: coordinates + velocity (or a scalar in the temperature slot), arrays as (ncomp, nel, nz, ny, nx)."""
    ex = (lambda a: a[..., None, :, :]) if h.ndim == 2 else (lambda a: a)
    nekio.write_fld(path, x=ex(_coords(h)), u=None if u is None else ex(np.asarray(u)), t=None if t is None else ex(np.asarray(t)))


def energy_budget(h, ub, dRe, dIm, *, outdir=None, session="1cyl"):
    """uparam(1) = 4.1.  Base flow and direct mode as device vectors (left as they are).  Returns (integrals [10], their sum,
    production fields [ndim, ndim, nel, ...]); writes KIN<session>0.f00001 .. f0000<ndim> into ``outdir`` when given, file c
    holding P[c][1..ndim] in its velocity slots (outpost(..., "KIN") once per base-flow component)."""
    vecs = h.alloc(h.ndim)
    try:
        integrals = h.energy_budget(ub, dRe, dIm, prod=vecs)
        prod = np.array([download_velocity(h, v) for v in vecs])
    finally:
        h.free(vecs)
    if outdir is not None:
        for c in range(h.ndim):
            _write(h, os.path.join(outdir, fld_name("KIN", session, c + 1)), u=prod[c])
    return integrals, float(np.sum(integrals)), prod


def postprocess(h, ub, dRe, dIm, aRe, aIm, *, outdir=None, session="1cyl"):
    """uparam(1) = 4.0 (core/usr_extra.f:216-221): energy_budget, then wave_maker, then bf_sensitivity, writing every file of the
    three into ``outdir`` when given.  Base flow and modes are device vectors, left as they are: as the reference reloads the
    mode files for each step, wave_maker and bf_sensitivity each biorthogonalise their own copy of the modes.  Returns a dict:
    integrals, budget_sum, prod, wm, gamma_delta and the bf_sensitivity fields (tr, ti, pr, pi, sr, si)."""
    integrals, total, prod = energy_budget(h, ub, dRe, dIm, outdir=outdir, session=session)
    modes = (dRe, dIm, aRe, aIm)
    work = h.alloc(4)
    try:
        for w, m in zip(work, modes):
            h.copy(w, m)
        wm, gd = wave_maker(h, *work, outdir=outdir, session=session)
        for w, m in zip(work, modes):
            h.copy(w, m)
        sens, _ = bf_sensitivity(h, *work, outdir=outdir, session=session)
    finally:
        h.free(work)
    return dict(integrals=integrals, budget_sum=total, prod=prod, wm=wm, gamma_delta=gd, **sens)


def wave_maker(h, dRe, dIm, aRe, aIm, *, outdir=None, session="1cyl"):
    """uparam(1) = 4.2.  Modes as device vectors (biorthogonalised in place).  Returns (field [nel, ...], (gamma, delta));
    writes wm_<session>0.f00001 into ``outdir`` when given."""
    gd = h.biorthogonalize(dRe, dIm, aRe, aIm)
    (wm,) = h.alloc(1)
    try:
        h.wavemaker(dRe, dIm, aRe, aIm, wm)
        field = download_velocity(h, wm)[0]
    finally:
        h.free([wm])
    if outdir is not None:
        _write(h, os.path.join(outdir, fld_name("wm_", session)), t=field)
    return field, gd


def bf_sensitivity(h, dRe, dIm, aRe, aIm, *, outdir=None, session="1cyl"):
    """uparam(1) = 4.3.  Modes as device vectors (biorthogonalised in place).  Returns (dict of tr, ti, pr, pi, sr, si velocity
    fields, (gamma, delta)); writes tr_ ti_ pr_ pi_ sr_ si_ files into ``outdir`` when given."""
    gd = h.biorthogonalize(dRe, dIm, aRe, aIm)
    vecs = h.alloc(6)
    try:
        h.bf_sensitivity(dRe, dIm, aRe, aIm, vecs[0], vecs[1], parts=vecs[2:])
        out = {k: download_velocity(h, v) for k, v in zip(("sr", "si", "tr", "ti", "pr", "pi"), vecs)}
    finally:
        h.free(vecs)
    if outdir is not None:
        for k in ("tr", "ti", "pr", "pi", "sr", "si"):
            _write(h, os.path.join(outdir, fld_name(k + "_", session)), u=out[k])
    return out, gd


def steady_force_sensitivity(h, force, *, k_dim=100, tol=None, maxiter=10, log=None, outdir=None, session="1cyl",
                             prefix="fsr"):
    """uparam(1) = 4.41 (force = sr, prefix fsr) / 4.42 (force = si, prefix fsi): ts_steady_force_sensitivity.
    rhs = forced adjoint map of 0 under ``force`` (a device vector), normalised; GMRES on (I - exp(L^+ T)) x = rhs with the
    reference's ts_gmres(rhs, sol, 10, k_dim); x scaled back.  ``tol`` is the reference's max(param(21), param(22)) on the
    SQUARED residual (default 1e-12).  Returns (device vector x -- free it with h.free --, linearised-map calls)."""
    rhs, sol, zero = h.alloc(3)
    try:
        h.zero(zero)
        h.forced_map(rhs, zero, force, NSK_ADJOINT)               # initialize_rhs_ts_steady_force_sensitivity
        alpha = h.norm(rhs)                                       # krylov_normalize
        h.scal(rhs, 1.0 / alpha)
        calls = newton.ts_gmres(h, rhs, sol, k_dim, 1e-12 if tol is None else tol, maxiter=maxiter, log=log,
                                mode=NSK_FORCE_SENSITIVITY)
        h.scal(sol, alpha)
    finally:
        h.free([rhs, zero])
    if outdir is not None:
        _write(h, os.path.join(outdir, fld_name(prefix, session)), u=download_velocity(h, sol))
    return sol, calls


def write_delta_forcing(h, path, dl, dw):
    """dfr file of delta_forcing: (delta_lambda, delta_omega [, 0]) in the velocity slots."""
    u = [dl, dw] + ([np.zeros_like(dl)] if h.ndim == 3 else [])
    _write(h, path, u=np.array(u))
