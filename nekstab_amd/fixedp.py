"""Steady base flows by fixed-point iteration over the device backend: selective frequency damping and BoostConv.

``SFD`` (core/fixedp.f:114-242, uparam(1) = 1.1): the full equations are integrated with the force -chi (v - qbar), qbar a low-pass-filtered copy of the
velocity (cut-off omega_c), until the flow stops moving.  The filter, the force and the per-step residual run on the device
inside the step loop (nsk_sfd_map / nsk_group_sfd_map); this module holds the parameters, the loop over maps, the convergence
rule and the files:

  residu.dat              (4E15.7)  time, residu, (residu - previous) / dt, tol; one line per time step          :215
  BF_<session>0.f00001    the converged state in fp64 (param(63) = 1)                                             :226-228
  BFV<session>0.f00001    its vorticity (comp_vort3), ``ifvor=True``                                              :232-235

``BoostConv`` (core/fixedp.f:282-468, uparam(1) = 1.2): behind every ``skip``-th time step of the unforced full equations the
velocity change r of that step is recombined with ``snp`` stored pairs of earlier residual and correction differences (a least
squares problem in the bm1 inner product) into a larger correction xi, and the step is replaced by v <- v_before + xi.  The
state, the sums and the small solve live on the device (nsk_boostconv_map / nsk_group_boostconv_map); ``np_boostconv_core`` is
the literal numpy restatement of boostconv_core (modified Gram-Schmidt and all) the device is tested against; ``boostconv``
drives the maps and writes

  residu.dat              (3E15.7)  time, residu, (residu - previous) / dt; one line per BoostConv call            :309
  BF_<session>0.f00001    the converged state in fp64; BFV<session>0.f00001 with ``ifvor=True``                    :319-323

TDF and DMT (uparam(1) = 1.4, 1.3), ``ifdyntol`` and SFD's continuation mode (uparam(5) = 0) are not built.
"""
from __future__ import annotations

import math
import os

import numpy as np

from . import nekio
from .outpost import _fortran_e
from .quadrature import gauss_legendre, gauss_lobatto_legendre, interp_matrix


def sfd_parameters(strouhal, sigma):
    """(omega_c, chi) from uparam(4) = ``strouhal`` and uparam(5) = ``sigma`` (:137-152): frq = 2 pi |St|, sig = |sigma|;
    St > 0 (Akervik et al. 2006): omega_c = frq / 2, chi = 2 sig; St < 0 (Casacuberta et al. 2018):
    omega_c = (sqrt(frq^2 + sig^2) - sig) / 2, chi = (sqrt(frq^2 + sig^2) + sig) / 2."""
    frq, sig = 2.0 * math.pi * abs(strouhal), abs(sigma)
    if strouhal > 0:
        return 0.5 * frq, 2.0 * sig
    r = math.sqrt(frq * frq + sig * sig)
    return 0.5 * (r - sig), 0.5 * (r + sig)


def ab_coefficients(istep):
    """setab3 at constant dt, as call ``istep`` >= 1 of SFD uses it: (3/2, -1/2, 0) for istep <= 2 -- at istep = 1 the older
    lags are still zero -- and (23/12, -16/12, 5/12) after."""
    if istep < 1:
        raise ValueError("ab_coefficients: call 0 does not advance the filter")
    return (1.5, -0.5, 0.0) if istep <= 2 else (23.0 / 12.0, -16.0 / 12.0, 5.0 / 12.0)


def np_sfd_filter(v, qbar0, omega_c, dt, volume=None, bm1=None):
    """The filter and the residual of one map in numpy, the restatement the device is tested against: v = [v^0 .. v^n]
    (arrays of one shape), qbar0 the filter state at call 0.  Returns (qbar^n, residu_1 .. residu_n); the residual needs
    ``bm1`` (broadcast against a v^j summed over its leading component axis) and ``volume``."""
    q = np.array(qbar0, dtype=np.float64)
    vxo = np.asarray(v[0], dtype=np.float64)
    ub = np.zeros_like(q)
    uc = np.zeros_like(q)
    res = []
    for j in range(1, len(v)):
        a, b, c = ab_coefficients(j)
        ua = vxo - q
        q = q + omega_c * dt * (a * ua + b * ub + c * uc)
        ub, uc = ua, ub
        if bm1 is not None:
            res.append(math.sqrt(float(np.sum(bm1 * (vxo - v[j]) ** 2)) / volume))
        vxo = np.asarray(v[j], dtype=np.float64)
    return q, np.array(res)


def residu_line(time, residu, rate, tol=None):
    """One line of residu.dat: Fortran (4E15.7) (SFD), or (3E15.7) without ``tol`` (BoostConv, :309)."""
    return "".join(_fortran_e(float(x), 15, 7) for x in (time, residu, rate, tol) if x is not None)


def write_residu(path, rows):
    with open(path, "w") as fh:
        for r in rows:
            fh.write(residu_line(*r) + "\n")


def np_boostconv_core(state, r, bm1, snp):
    """boostconv_core (core/fixedp.f:331-393) with qr_dec (:395-449) and linear_system (:451-468) in numpy, statement by
    statement.  ``state``: a dict, empty before the first call; it then holds X, Y (snp, *r.shape), the 1-based ``rot`` and the
    last coefficients ``c``.  ``r``: the residual, its leading axis the velocity components; ``bm1`` broadcasts against one
    component.  Returns xi; the caller sets v = v_before + xi (:306)."""
    r = np.array(r, dtype=np.float64)

    def ip(a, b):                                             # glsc3 per component, added (:377-378)
        return sum(float(np.sum(a[k] * bm1 * b[k])) for k in range(a.shape[0]))

    if not state:
        X = np.zeros((snp,) + r.shape)
        Y = np.zeros((snp,) + r.shape)
        Y[0] = r
        X[0] = r
        state.update(X=X, Y=Y, rot=1, c=np.zeros(snp))
        return r.copy()
    X, Y, rot = state["X"], state["Y"], state["rot"]
    Y[rot - 1] -= r
    X[rot - 1] -= Y[rot - 1]
    with np.errstate(all="ignore"):                           # (the reference does not guard its first column)
        Q = np.zeros_like(Y)
        R = np.zeros((snp, snp))
        d = Y[0].copy()
        norma = np.float64(math.sqrt(ip(d, d)))
        d = d * (1.0 / norma)
        Q[0] = d
        R[0, 0] = norma
        for j in range(1, snp):
            d = Y[j].copy()
            for i in range(j):
                R[i, j] = ip(d, Q[i])
                d -= Q[i] * R[i, j]
            norma = ip(d, d)
            if norma < 1e-60:
                norma = 1.0
                Q[j] = 0.0
            else:
                Q[j] = d * (1.0 / math.sqrt(norma))
            R[j, j] = math.sqrt(norma)
        cc = np.array([ip(r, Q[j]) for j in range(snp)])
        c = np.zeros(snp)
        for j in range(snp - 1, -1, -1):
            c[j] = cc[j]
            for k in range(j + 1, snp):
                c[j] -= R[j, k] * c[k]
            c[j] = c[j] / R[j, j]
    rot = rot % snp + 1
    Y[rot - 1] = r
    xi = r.copy()
    for j in range(snp):
        xi += X[j] * c[j]
    X[rot - 1] = xi
    state["rot"], state["c"] = rot, c
    return xi.copy()


def _fields(be, v):
    """Device state -> (x, u, p on mesh 1) in the field-file layout (ndim, nel, nz, ny, nx), coordinates from the backend."""
    from .sensitivity import _coords
    n = be.lx1
    J21 = interp_matrix(gauss_legendre(n - 2)[0], gauss_lobatto_legendre(n)[0])
    x = _coords(be)
    if be.ndim == 3:
        vx, vy, vz, pr = be.download3(v)
        return x, np.stack([vx, vy, vz]), np.einsum("ci,bj,ak,ekji->ecba", J21, J21, J21, pr, optimize=True)
    vx, vy, pr = be.download(v)
    return x[:, :, None], np.stack([vx, vy])[:, :, None], (J21 @ pr @ J21.T)[:, None]


def sfd(be, q, *, strouhal, sigma, tol, max_time, outdir=None, ifvor=False, log=None, session="1cyl"):
    """q <- the state SFD ends at, started from q with qbar = q (the reference's run from istep = 0).  The run is a chain of
    maps of ``be.nsteps`` steps (the sampling period), ``be.set_baseflow`` on the current state between them for the CFL rule,
    q and qbar carried across; the BDF / EXT ramp and the filter's Adams-Bashforth ramp restart at every map.  It stops at the
    first time step with global count > 100 and residu < ``tol`` (:222) or once ``max_time`` is reached.  ``outdir``:
    residu.dat, and on convergence BF_<session>0.f00001 (fp64) and, with ``ifvor``, BFV<session>0.f00001.
    ``be``: a NekStabHip or a ShardGroup.  ``log(step, time, residu)`` per time step.
    Returns (converged, steps, history): history[k] = residu of global step k + 1."""
    omega_c, chi = sfd_parameters(strouhal, sigma)
    f, qbar, qbar0 = be.alloc(3)
    be.copy(qbar, q)
    rows, hist = [], []
    steps, time, prev, converged = 0, 0.0, 0.0, False
    nsteps_map = None
    try:
        while not converged and time < max_time:
            be.set_baseflow(q)                                # dt of the CFL rule on the current state; nsteps = period / dt
            nsteps_map = be.nsteps
            dt = be.dt
            n = max(1, min(be.nsteps, int(math.ceil((max_time - time) / dt - 1e-9))))
            if n != be.nsteps:
                be.set_nsteps(n)
            be.copy(qbar0, qbar)
            res = be.sfd_map(f, q, qbar, chi, omega_c)
            stop = None
            for k, r in enumerate(res):
                if steps + k + 1 > 100 and r < tol:
                    stop = k + 1
                    break
            if stop is not None and stop < n:                 # the state AT that step: the same map, cut there
                be.set_nsteps(stop)
                be.copy(qbar, qbar0)
                res = be.sfd_map(f, q, qbar, chi, omega_c)
                n = stop
                # (the pressure projection space of a quadrilateral context carries over between maps, so the cut map repeats
                #  the first one to solver tolerance, not to the bit: its own residual decides; if it says no, the run goes on
                #  from this step)
                if not res[n - 1] < tol:
                    stop = None
            for r in res[:n]:
                steps += 1
                time += dt
                rows.append((time, r, (r - prev) / dt, tol))
                hist.append(r)
                prev = r
                if log:
                    log(steps, time, r)
            be.copy(q, f)
            converged = stop is not None
    finally:
        if nsteps_map is not None and be.nsteps != nsteps_map:
            be.set_nsteps(nsteps_map)
        be.free([f, qbar, qbar0])
    if outdir is not None:
        os.makedirs(outdir, exist_ok=True)
        write_residu(os.path.join(outdir, "residu.dat"), rows)
        if converged:
            _write_bf(be, q, outdir, session, time, steps, ifvor)
    return converged, steps, np.array(hist)


def _write_bf(be, q, outdir, session, time, steps, ifvor):
    x, u, p1 = _fields(be, q)
    nekio.write_fld(os.path.join(outdir, "BF_%s0.f00001" % session), x=x, u=u, p=p1, time=time, istep=steps, wdsize=8)
    if ifvor:
        w = be.alloc(1)
        try:
            be.vorticity(w[0], q)
            x, u, _ = _fields(be, w[0])
        finally:
            be.free(w)
        # (param(63) is back to 0 before this outpost, :229: single precision, as the Rv files of outpost_ks)
        nekio.write_fld(os.path.join(outdir, "BFV%s0.f00001" % session), x=x, u=u, time=time, istep=steps, wdsize=4)


def boostconv(be, q, *, snp=10, skip=10, tol, max_time, outdir=None, ifvor=False, log=None, session="1cyl"):
    """q <- the state BoostConv ends at, started from q (the reference's run from istep = 0: bst_snp = ``snp``, bst_skp =
    ``skip``).  The run is a chain of maps of ``be.nsteps`` steps, ``be.set_baseflow`` on the current state between them for
    the CFL rule, the global step count carried into every map so that the calls fall on its multiples of ``skip`` whatever
    the maps' lengths; the BDF / EXT ramp restarts at every map, the BoostConv state does not.  It stops at the first call
    with residu < ``tol`` (:315) -- the call at step 0, whose "residual" is the velocity itself, is not asked -- or once
    ``max_time`` is reached.  ``outdir``: residu.dat, and on convergence BF_<session>0.f00001 (fp64) and, with ``ifvor``,
    BFV<session>0.f00001.  ``be``: a NekStabHip or a ShardGroup.  ``log(step, time, residu)`` per call.
    Returns (converged, steps, history): history[k] = residu of call k."""
    f, = be.alloc(1)
    be.boostconv_init(snp)
    rows, hist = [], []
    steps, time, prev, converged = 0, 0.0, 0.0, False
    nsteps_map = None
    try:
        while not converged and time < max_time:
            be.set_baseflow(q)                                # dt of the CFL rule on the current state; nsteps = period / dt
            nsteps_map = be.nsteps
            dt = be.dt
            n = max(1, min(be.nsteps, int(math.ceil((max_time - time) / dt - 1e-9))))
            if n != be.nsteps:
                be.set_nsteps(n)
            res = be.boostconv_map(f, q, skip, steps)
            at = ([0] if steps == 0 else []) + [j for j in range(1, n + 1) if (steps + j) % skip == 0]      # the map's calls
            assert len(at) == len(res)
            stop = next((j for j, r in zip(at, res) if j > 0 and r < tol), None)
            if stop is not None and stop < n:                 # the state AT that call: the same map from the same state, cut there
                be.boostconv_rewind()
                be.set_nsteps(stop)
                res = be.boostconv_map(f, q, skip, steps)
                n = stop
                at = [j for j in at if j <= n]
                # (as sfd(): the cut map repeats the first one to solver tolerance, not to the bit; its own residual decides)
                if not res[-1] < tol:
                    stop = None
            for j, r in zip(at, res):
                rows.append((time + j * dt, r, (r - prev) / dt))
                hist.append(r)
                prev = r
                if log:
                    log(steps + j, time + j * dt, r)
            steps += n
            time += n * dt
            be.copy(q, f)
            converged = stop is not None
    finally:
        if nsteps_map is not None and be.nsteps != nsteps_map:
            be.set_nsteps(nsteps_map)
        be.free([f])
    if outdir is not None:
        os.makedirs(outdir, exist_ok=True)
        write_residu(os.path.join(outdir, "residu.dat"), rows)
        if converged:
            _write_bf(be, q, outdir, session, time, steps, ifvor)
    return converged, steps, np.array(hist)
