"""``outpost_ks`` (core/eigensolvers.f:508-721): spectra tables and converged eigenmodes in the
reference's on-disk formats, so nekStab's own post-processing (p_spec.py, wave_maker, ...) can read
them unchanged.

  Spectre_H<op>.dat        (3E15.7)  Re mu, Im mu, residual          :590
  Spectre_NS<op>.dat       (3E15.7)  Re/Im log(mu)/T, residual      :593-595
  Spectre_NS<op>_conv.dat  (2E15.7)  converged & outposted <= maxmodes   :601-604
  <op>Re<session>0.f0000i / <op>Im...  eigenmode i = Q y_i, |Re|^2+|Im|^2 = 1 (bm1s), time = i  :607-642
  <op>Rv<session>0.f0000i  vorticity of the real part of eigenmode i (comp_vort3; ``ifvor=True``)   :629-637
  <op>Rx<session>0.f0000i  lambda2, Q [, Omega] of the real part of eigenmode i (``ifvox=True``; 2-D: <op>Ro..., Omega as temperature)
  vox / omg<session>0.f0000n  ``outpost_vox``: the vortex-identification files of nekStab_outpost (core/usr_extra.f:269-281)
  Spectre_<op>.info        key=value manifest of the run (mesh, uparam, solver, eigensolver)   :664-717
"""
from __future__ import annotations

import os

import numpy as np

from . import nekio
from .checkpoint import state_to_fields
from .krylov import assemble_mode, log_transform


def _fortran_e(x, width, digits):
    """Fortran ``Ew.d`` edit descriptor (0.1234567E+01): python's %E normalises to 1.234567E+00."""
    if x == 0.0:
        m, e = 0.0, 0
    else:
        e = int(np.floor(np.log10(abs(x)))) + 1
        m = x / 10.0 ** e
        if abs(round(m, digits)) >= 1.0:              # 0.99999996 -> 1.0000000: renormalise like the Fortran runtime
            m /= 10.0
            e += 1
    return ("%.*fE%+03d" % (digits, m, e)).rjust(width)


def write_info(path, be, case, res, *, evop, sampling_period, eigen_tol, schur_tgt, schur_del, outposted, uparam=None,
               tol_pres=None, tol_vel=None, nranks=1, ctarg=None, k_dim=None):
    """``Spectre_<op>.info`` as outpost_ks writes it (core/eigensolvers.f:664-717): formats (A,I16), (A,F16.4),
    (A,F16.12), (A,E15.7), (A,E13.4); same keys in the same order.  Version strings name this build."""
    up = list(uparam) if uparam is not None else [0.0] * 10
    up += [0.0] * (10 - len(up))
    nd = int(getattr(case, "ndim", 2))
    L = ["Nek5000 version:" + "none (nekstab_amd: MI355X-native time stepper)", "nekStab version:" + "nekstab_amd",
         "[mesh]",
         "lx1=             %16d" % case.lx1, "polyOrder N=     %16d" % (case.lx1 - 1), "tot elemts=      %16d" % case.nel,
         "tot points=      %16d" % (case.nel * case.lx1 ** nd), "MPI ranks=       %16d" % nranks, "e/rank=          %16d" % (case.nel // nranks),
         "[userParams]"]
    L += ["uparam%02d=        %16.12f" % (i + 1, up[i]) for i in range(10)]
    L += ["[solver]",
          "ctarg=           %16.4f" % (case.cfl if ctarg is None else ctarg), "nsteps=          %16d" % be.nsteps,
          "dt=              " + _fortran_e(be.dt, 15, 7), "Re=              %16.4f" % case.re,
          "residualTol PRE= " + _fortran_e(0.0 if tol_pres is None else tol_pres, 13, 4),
          "residualTol VEL= " + _fortran_e(0.0 if tol_vel is None else tol_vel, 13, 4),
          "[eigensolver]",
          "sampling period =%16.12f" % sampling_period, "k_dim=           %16d" % (res.H.shape[1] if k_dim is None else k_dim),
          "eigentol=        " + _fortran_e(eigen_tol, 13, 4), "schur_target=    %16d" % schur_tgt, "schur_del=       %16.4f" % schur_del,
          "schur iterations=%16d" % res.schur_cnt, "outposted=       %16d" % outposted]
    with open(path, "w") as fh:
        fh.write("\n".join(L) + "\n")


def read_info(path):
    """key -> string value of a ``Spectre_<op>.info`` manifest (ours or the reference's)."""
    out = {}
    for line in open(path):
        line = line.rstrip("\n")
        if "=" in line and not line.startswith("["):
            k, v = line.split("=", 1)
            out[k.strip()] = v.strip()
    return out


def outpost_vox(be, q, case, outdir, *, session, num=1, wght=0.5, prefix="vox", prefix_omg="omg", time=0.0, istep=0, wdsize=4):
    """The vortex-identification files of nekStab_outpost with ``ifvox = .true.`` (core/usr_extra.f:269-281) for the velocity of
    the device vector ``q`` (a context or a ``ShardGroup`` as ``be``; ``be.vortex_criteria``):
      vox<session>0.f0000n   lambda2, Q [, Omega] in the velocity slots, no pressure and no temperature (read code XU)
      omg<session>0.f0000n   2-D only: Omega as the temperature field, no velocity (read code XT)
    ``wght``: the weight of filter_s0 (the reference's 0.5; 0: unfiltered).  Returns the paths written."""
    os.makedirs(outdir, exist_ok=True)
    nd = int(getattr(case, "ndim", 2))
    w, om = be.alloc(2)
    try:
        be.vortex_criteria(w, q, wght, omega=om if nd == 2 else None)
        x, u, _ = state_to_fields(be, case, w)
        out = [os.path.join(outdir, "%s%s0.f%05d" % (prefix, session, num))]
        nekio.write_fld(out[0], x=x, u=u, time=time, istep=istep, wdsize=wdsize)
        if nd == 2:
            _, uo, _ = state_to_fields(be, case, om)
            out.append(os.path.join(outdir, "%s%s0.f%05d" % (prefix_omg, session, num)))
            nekio.write_fld(out[1], x=x, t=uo[0], time=time, istep=istep, wdsize=wdsize)
    finally:
        be.free([w, om])
    return out


def outpost_ks(be, res, case, outdir, *, evop="d", sampling_period=1.0, eigen_tol=1e-6, maxmodes=20,
               session="1cyl", wdsize=4, schur_tgt=0, schur_del=0.10, uparam=None, tol_pres=None, tol_vel=None, nranks=1,
               ifvor=False, ifvox=False):
    """``ifvor``: also write, for every converged mode, ``<evop>Rv<session>0.f0000i`` = the vorticity of its real part
    (comp_vort3 + outpost(vort, 'Rv') with ifpo = ifto = .false., core/eigensolvers.f:629-637: read code XU, time / istep / wdsize
    of the Re file), computed on the device (``be.vorticity``).
    ``ifvox``: also write ``<evop>Rx<session>0.f0000i`` = the vox file of its real part (lambda2, Q [, Omega]; ``outpost_vox``)
    and, in 2-D, ``<evop>Ro<session>0.f0000i`` = its omg file (Omega as temperature), with the header of the Re file.
    Returns the Re / Im paths, then the Rv paths, then the Rx (and Ro) paths."""
    os.makedirs(outdir, exist_ok=True)
    k = res.H.shape[1]
    lam = log_transform(res.vals, sampling_period)
    nekio.write_spectre(os.path.join(outdir, f"Spectre_H{evop}.dat"), res.vals, res.residual)
    nekio.write_spectre(os.path.join(outdir, f"Spectre_NS{evop}.dat"), lam, res.residual)
    conv = []
    re, im = be.alloc(2)
    vor = be.alloc(1) if ifvor else []
    written, written_rv, written_rx = [], [], []
    for i in range(k):
        if res.residual[i] < eigen_tol and len(conv) < maxmodes:
            conv.append(lam[i])
            assemble_mode(be, res, i, re, im)
            idx = len(conv)
            for tag, v in (("Re", re), ("Im", im)):
                x, u, p1 = state_to_fields(be, case, v)          # pressure -> mesh 1 for output (map21); 2-D and 3-D
                f = os.path.join(outdir, "%s%s%s0.f%05d" % (evop, tag, session, idx))
                nekio.write_fld(f, x=x, u=u, p=p1, time=float(i + 1), istep=be.nsteps + 1, wdsize=wdsize)
                written.append(f)
            if ifvor:
                be.vorticity(vor[0], re)
                x, u, _ = state_to_fields(be, case, vor[0])
                f = os.path.join(outdir, "%sRv%s0.f%05d" % (evop, session, idx))
                nekio.write_fld(f, x=x, u=u, time=float(i + 1), istep=be.nsteps + 1, wdsize=wdsize)
                written_rv.append(f)
            if ifvox:
                written_rx += outpost_vox(be, re, case, outdir, session=session, num=idx, prefix=evop + "Rx",
                                          prefix_omg=evop + "Ro", time=float(i + 1), istep=be.nsteps + 1, wdsize=wdsize)
    nekio.write_spectre(os.path.join(outdir, f"Spectre_NS{evop}_conv.dat"), np.array(conv))
    write_info(os.path.join(outdir, f"Spectre_{evop}.info"), be, case, res, evop=evop, sampling_period=sampling_period,
               eigen_tol=eigen_tol, schur_tgt=schur_tgt, schur_del=schur_del, outposted=len(conv), uparam=uparam,
               tol_pres=tol_pres, tol_vel=tol_vel, nranks=nranks)
    be.free([re, im] + vor)
    return written + written_rv + written_rx
