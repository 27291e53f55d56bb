"""Covariance of the hexahedral path (tests/test_oracle3d.py, tests/test_axes3d_gpu.py): the same problem with every element's local
axes (r, s, t) relabelled by a proper signed permutation and the physical frame moved by an orthogonal matrix Q.

A relabelling ``local`` = (perm, sign): the new local axis a is the old axis perm[a], run forwards (sign[a] = +1) or backwards
(-1; GLL and Gauss points are symmetric, so reversing an index is exact).  For an array f[e, k, j, i] (i = axis 0 fastest)
    new[e, i'_2, i'_1, i'_0] = old[e, i_2, i_1, i_0],    i_perm[a] = i'_a  or  n - 1 - i'_a.
Its determinant is the permutation's parity times the product of the signs.  The Jacobian of the transformed mapping is
det(Q) det(local) times the original one and set-up rejects a non-positive Jacobian, so the product must be +1.

What is covariant: scalars on either mesh (sponge, masks, the weak divergence, the Gauss-mesh pressure) are re-indexed by ``local``
only; vectors (coordinates, base flow, velocity, D^T p, the convection terms) are re-indexed and their components mixed by Q."""
import dataclasses
import itertools

import numpy as np

from nekstab_amd import mesh, mesh3d

IDENTITY = ((0, 1, 2), (1, 1, 1))


def _parity(perm):
    return int(round(np.linalg.det(np.eye(3)[list(perm)])))


def det_local(local):
    perm, sign = local
    return _parity(perm) * int(np.prod(sign))


def proper_relabellings():
    """the 24 signed permutations of (r, s, t) with determinant +1"""
    out = []
    for perm in itertools.permutations(range(3)):
        for sign in itertools.product((1, -1), repeat=3):
            if det_local((perm, sign)) == 1:
                out.append((tuple(perm), tuple(sign)))
    return out


def inverse(local):
    perm, sign = local
    ip, isg = [0, 0, 0], [0, 0, 0]
    for a in range(3):
        ip[perm[a]], isg[perm[a]] = a, sign[a]
    return tuple(ip), tuple(isg)


def relabel(f, local):
    """re-index the last three axes [k, j, i] of f by ``local``"""
    perm, sign = local
    f = np.asarray(f)
    nd = f.ndim
    order = list(range(nd))
    for a in range(3):
        order[nd - 1 - a] = nd - 1 - perm[a]
    g = f.transpose(order)
    flips = [nd - 1 - a for a in range(3) if sign[a] < 0]
    if flips:
        g = np.flip(g, axis=flips)
    return np.ascontiguousarray(g)


def relabel_vert(vert, local):
    """columns of the corner table (c = ir + 2 is + 4 it) of the relabelled elements"""
    perm, sign = local
    vert = np.asarray(vert)
    out = np.empty_like(vert)
    for cn in range(8):
        bn = [(cn >> a) & 1 for a in range(3)]
        bo = [0, 0, 0]
        for a in range(3):
            bo[perm[a]] = bn[a] if sign[a] > 0 else 1 - bn[a]
        out[:, cn] = vert[:, bo[0] + 2 * bo[1] + 4 * bo[2]]
    return out


def _mix(Q, v):
    """sum_b Q[a, b] v[b]; exact zeros of Q are skipped, so a signed permutation matrix copies (and negates) without rounding"""
    return [sum(Q[a, b] * np.asarray(v[b]) for b in range(3) if Q[a, b] != 0.0) for a in range(3)]


def is_signed_permutation(Q):
    Q = np.asarray(Q, dtype=np.float64)
    return bool(np.all((Q == 0.0) | (np.abs(Q) == 1.0)) and np.all(np.abs(Q).sum(0) == 1.0) and np.all(np.abs(Q).sum(1) == 1.0))


def transform_case(case, local, Q):
    """The Case3D of the same problem in the frame x' = Q x with every element's axes relabelled by ``local``."""
    Q = np.asarray(Q, dtype=np.float64)
    assert Q.shape == (3, 3) and np.abs(Q @ Q.T - np.eye(3)).max() < 1e-14, "Q must be orthogonal"
    dq = np.linalg.det(Q)
    assert abs(dq * det_local(local) - 1.0) < 1e-12, "det(Q) det(local) must be +1: set-up rejects a non-positive Jacobian"
    if case.cmask is not None and not is_signed_permutation(Q):
        raise ValueError("transform_case: a case with component masks moves only under a signed permutation matrix Q "
                         "(a component mask of an oblique frame is no mask of one component)")
    xyz = [relabel(f, local) for f in _mix(Q, (case.x, case.y, case.z))]
    ub = np.stack([relabel(f, local) for f in _mix(Q, case.ub)])
    cmask = None
    if case.cmask is not None:
        cmask = np.stack([relabel(f, local) for f in _mix(np.abs(Q), case.cmask)])
    meta = dict(case.meta)
    meta["vert"] = relabel_vert(case.meta["vert"], local)
    return dataclasses.replace(case, x=xyz[0], y=xyz[1], z=xyz[2], gid=relabel(case.gid, local), mask=relabel(case.mask, local),
                               spng=relabel(case.spng, local), ub=ub, meta=meta, cmask=cmask)


def to_frame(vel3, pres, local, Q):
    """a state (three velocity components, Gauss-mesh pressure) of the original problem in the transformed frame"""
    Q = np.asarray(Q, dtype=np.float64)
    vel = [relabel(f, local) for f in _mix(Q, vel3)]
    return vel, (None if pres is None else relabel(pres, local))


def from_frame(vel3, pres, local, Q):
    """inverse of to_frame"""
    Q = np.asarray(Q, dtype=np.float64)
    inv = inverse(local)
    vel = _mix(Q.T, [relabel(f, inv) for f in vel3])
    return vel, (None if pres is None else relabel(pres, inv))


def orientation(A, C, sign=(1, 1, 1)):
    """(local, Q) that carry the third local axis t onto local axis A (the other two keep their order) and the coordinate z onto
    coordinate C (x and y keep theirs), with the local signs ``sign``; the sign of the new coordinate C is chosen so that
    det(Q) det(local) = +1."""
    rest = [a for a in range(3) if a != A]
    perm = [0, 0, 0]
    perm[A], perm[rest[0]], perm[rest[1]] = 2, 0, 1
    local = (tuple(perm), tuple(sign))
    Q = np.zeros((3, 3))
    rows = [c for c in range(3) if c != C]
    Q[C, 2], Q[rows[0], 0], Q[rows[1], 1] = 1.0, 1.0, 1.0
    if np.linalg.det(Q) * det_local(local) < 0:
        Q[C, 2] = -1.0
    return local, Q


def oblique(seed=7):
    """a rotation with no small entry, from the QR factorisation of a seeded random matrix (the first draw of the seeded stream
    whose Q has every |entry| > 0.1: no direction is nearly aligned with an axis)"""
    rng = np.random.default_rng(seed)
    while True:
        Q, R = np.linalg.qr(rng.standard_normal((3, 3)))
        Q = Q * np.sign(np.diag(R))
        if np.linalg.det(Q) < 0:
            Q[:, 2] = -Q[:, 2]
        if np.abs(Q).min() > 0.1:
            return Q


def inplane_ub(x, y, z):
    return np.stack([1.0 - 0.3 * y * y + 0.1 * np.sin(x), 0.2 * np.cos(x) * y, 0.0 * z])


def inplane_case(n=6, nz=2, nx=3):
    """nx x 2 elements curved in the plane, nz periodic layers in z, outflow at xmax, a two-dimensional base flow and a sponge:
    the spanwise direction is local axis t and coordinate z"""
    c = mesh3d.box_case_3d(nx, 2, nz, n, lengths=(2.0, 1.0, 0.8), periodic=(False, False, True), outflow_xmax=True,
                           re=40.0, endtime=0.05, ub_func=inplane_ub)
    bump = 0.06 * np.sin(np.pi * c.x / 2.0) * np.sin(np.pi * c.y)
    c.x = c.x + bump
    c.y = c.y - 0.5 * bump
    c.ub[:] = inplane_ub(c.x, c.y, c.z)
    c.spng = 0.5 * np.clip(c.x - 1.5, 0.0, None) ** 2
    return c


def plane_case(c3):
    """the quadrilateral Case of which ``c3`` = inplane_case(..) is the extrusion: its first layer's plane k = 0"""
    nel2 = c3.nel // c3.meta["box"][2]
    sl = (slice(0, nel2), 0)
    _, inv = np.unique(c3.gid[sl].ravel(), return_inverse=True)
    gid2 = inv.reshape(c3.gid[sl].shape).astype(np.int64)
    _, vinv = np.unique(c3.meta["vert"][:nel2, :4].ravel(), return_inverse=True)
    vert2 = vinv.reshape(nel2, 4).astype(np.int64)
    return mesh.Case(ndim=2, nel=nel2, lx1=c3.lx1, x=c3.x[sl].copy(), y=c3.y[sl].copy(), gid=gid2, nglob=int(gid2.max()) + 1,
                     mask=c3.mask[sl].copy(), ub=c3.ub[:2, :nel2, 0].copy(), spng=c3.spng[sl].copy(), re=c3.re, endtime=c3.endtime,
                     cfl=c3.cfl, lxd=c3.lxd, has_outflow=c3.has_outflow, meta=dict(vert=vert2, nvert=int(vert2.max()) + 1))
