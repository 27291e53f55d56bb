"""Time-periodic base flows as temporal Fourier modes (core/fourier.f), host side.

The device keeps an orbit as ``A_0, A_1, B_1, .., A_M, B_M`` (``nsk_set_orbit_fourier`` / ``nsk_set_orbit_modes``) with

    U(t_n) = A_0 + sum_{k=1..M} A_k cos(2 pi k n / N) + B_k sin(2 pi k n / N),   n = 0..N-1
    A_k = (c_k / N) sum_n U_n cos(2 pi k n / N),   B_k likewise with sin,
    c_0 = 1;  c_k = 2;  except c_{N/2} = 1 when N is even (the Nyquist term, whose B is 0)

``np_dft_modes`` / ``np_reconstruct`` restate that convention in numpy: they are the yardstick of the device kernels
(k_orbit_dft, k_baseflow_fourier).  ``write_modes`` / ``read_modes`` move the modes of a context to and from the
reference's ``fRe`` / ``fIm`` field files (fourier_decomposition, core/fourier.f:67-85), ``amplitude_report`` is its 99 %
criterion for choosing M (:63-68).  The context may be a ``NekStabHip`` or a ``sharded.ShardGroup`` (whole-mesh fields on the
host, every rank keeps its own elements' part).
"""
from __future__ import annotations

import os

import numpy as np

from . import nekio


def np_dft_modes(snaps, M):
    """Modes (A [M+1, ...], B [M, ...]) of the N snapshots ``snaps`` [N, ...] of one period, 0 <= M <= N // 2."""
    U = np.asarray(snaps, dtype=np.float64)
    N = U.shape[0]
    if not 0 <= M <= N // 2:
        raise ValueError("np_dft_modes: 0 <= M <= N // 2")
    n = np.arange(N)
    A = np.empty((M + 1,) + U.shape[1:])
    B = np.zeros((M,) + U.shape[1:])
    A[0] = U.sum(axis=0) / N
    for k in range(1, M + 1):
        ang = 2.0 * np.pi * ((k * n) % N) / N
        nyq = 2 * k == N
        ck = (1.0 if nyq else 2.0) / N
        A[k] = ck * np.tensordot(np.cos(ang), U, axes=(0, 0))
        if not nyq:
            B[k - 1] = ck * np.tensordot(np.sin(ang), U, axes=(0, 0))
    return A, B


def np_reconstruct(A, B, s):
    """The base flow at time ``s``, a fraction of the period (any real number: the orbit is periodic)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    out = A[0].copy()
    for k in range(1, A.shape[0]):
        fr = k * float(s)
        fr -= np.floor(fr)
        out += A[k] * np.cos(2.0 * np.pi * fr) + B[k - 1] * np.sin(2.0 * np.pi * fr)
    return out


def amplitude_report(amp):
    """``amp`` = the 2M+1 norms of A_0, A_1, B_1, .. (``set_orbit_fourier``).  Returns ``ampl`` [M+1], |mode k| =
    sqrt(|A_k|^2 + |B_k|^2), ``share`` [M], share[m-1] = sum_{k=1..m} |mode k| / sum_{k>=1} |mode k| (what keeping m harmonics
    captures), and ``m99``, the smallest m with share >= 0.99 -- the reference's criterion, core/fourier.f:63-68."""
    amp = np.asarray(amp, dtype=np.float64)
    if amp.size % 2 != 1:
        raise ValueError("amplitude_report: 2M+1 amplitudes")
    M = (amp.size - 1) // 2
    ampl = np.empty(M + 1)
    ampl[0] = abs(amp[0])
    for k in range(1, M + 1):
        ampl[k] = np.hypot(amp[2 * k - 1], amp[2 * k])
    tot = ampl[1:].sum()
    share = np.cumsum(ampl[1:]) / tot if tot > 0.0 else np.ones(M)
    m99 = int(np.argmax(share >= 0.99)) + 1 if M and np.any(share >= 0.99) else M
    return {"ampl": ampl, "share": share, "m99": m99}


def _to_field(h, v):
    """velocity of a state vector as write_fld's (ndim, nel, nz, ny, nx)"""
    if getattr(h, "ndim", 2) == 3:
        vx, vy, vz, _ = h.download3(v)
        return np.stack([vx, vy, vz])
    vx, vy, _ = h.download(v)
    return np.stack([vx, vy])[:, :, None]


def _from_field(h, v, u):
    pr = np.zeros(h.npres)
    if getattr(h, "ndim", 2) == 3:
        h.upload3(v, u[0], u[1], u[2], pr)
    else:
        h.upload(v, u[0], u[1], pr)


def write_modes(h, outdir, session="1cyl"):
    """The modes of the active Fourier orbit of ``h`` as field files, UN-normalised (the reference divides each field by its
    amplitude, core/fourier.f:81-83; here the amplitudes stand beside the fields instead):

      fRe<session>0.f0000(k+1)   A_k, k = 0..M   (velocity only, 8-byte reals, time = k)
      fIm<session>0.f0000(k+1)   B_k, k = 1..M
      fft_ampl.dat               line 1: period  M
                                 line 2+k, k = 0..M: |A_k|  |B_k|  k / period   (|B_0| = 0; bm1-weighted L2 norms)

    Returns the list of files written."""
    M, period = h.get_orbit_modes()
    A, B = h.alloc(M + 1), h.alloc(M) if M else []
    files = []
    try:
        h.get_orbit_modes(A, B)
        os.makedirs(outdir, exist_ok=True)
        rows = []
        for k in range(M + 1):
            f = os.path.join(outdir, "fRe%s0.f%05d" % (session, k + 1))
            nekio.write_fld(f, u=_to_field(h, A[k]), time=float(k), wdsize=8)
            files.append(f)
            nb = 0.0
            if k:
                f = os.path.join(outdir, "fIm%s0.f%05d" % (session, k + 1))
                nekio.write_fld(f, u=_to_field(h, B[k - 1]), time=float(k), wdsize=8)
                files.append(f)
                nb = h.norm(B[k - 1])
            rows.append((h.norm(A[k]), nb, k / period))
        f = os.path.join(outdir, "fft_ampl.dat")
        with open(f, "w") as fh:
            fh.write("%r %d\n" % (float(period), M))
            for r in rows:
                fh.write("%r %r %r\n" % tuple(float(x) for x in r))
        files.append(f)
    finally:
        h.free(list(A) + list(B))
    return files


def read_modes(h, outdir, session="1cyl"):
    """Load what ``write_modes`` wrote into ``h`` (``set_orbit_modes``: no integration).  Returns (M, period, amp) with
    ``amp`` the 2M+1 amplitudes in the order of ``set_orbit_fourier``."""
    with open(os.path.join(outdir, "fft_ampl.dat")) as fh:
        first = fh.readline().split()
        period, M = float(first[0]), int(first[1])
        rows = [[float(x) for x in fh.readline().split()] for _ in range(M + 1)]
    amp = [rows[0][0]]
    for k in range(1, M + 1):
        amp += [rows[k][0], rows[k][1]]
    A, B = h.alloc(M + 1), h.alloc(M) if M else []
    try:
        for k in range(M + 1):
            _from_field(h, A[k], nekio.read_fld(os.path.join(outdir, "fRe%s0.f%05d" % (session, k + 1))).u)
            if k:
                _from_field(h, B[k - 1], nekio.read_fld(os.path.join(outdir, "fIm%s0.f%05d" % (session, k + 1))).u)
        h.set_orbit_modes(A, B, period)
    finally:
        h.free(list(A) + list(B))
    return M, period, np.array(amp)
