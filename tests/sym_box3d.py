"""The hexahedral geometries of the symmetry-boundary tests (tests/test_symmetry3d_host.py, tests/test_symmetry3d_gpu.py): the
warped channel of tests/sym_box.py extruded in z.

    full      30 elements x 2 layers over z in [-1, 1], walls at both ends: mirror-symmetric about y = 0 and about z = 0
    yhalf     the 15-element half channel ('SYM' on y = 0), the same two layers
    zhalf     the full channel, one layer over z in [0, 1], 'SYM' on z = 0
    quarter   the half channel, one layer over z in [0, 1], 'SYM' on y = 0 and on z = 0: on the edge y = z = 0 u is free and
              v, w are fixed (three different masks); wall-'SYM' edges and corners are present
    xhalf     the transposed half channel ('SYM' on x = 0), two layers; its full domain is `full` transposed

Base flow and state are three-dimensional with the parities that keep the full-domain solution symmetric about both planes:
u, U even in y and z; v, V odd in y, even in z; w, W even in y, odd in z.  The state is multiplied by the (component) masks."""
import numpy as np

from nekstab_amd import mesh3d
from tests import sym_box

NEL2 = sym_box.NX * sym_box.NY
KINDS = ("full", "yhalf", "zhalf", "quarter", "xhalf")


def fields(x, y, z, transpose=False):
    """base flow (3, ...) and state (u, v, w): the 2-D fields of sym_box times even functions of z, and a third component odd in z"""
    ub2, u2, v2 = sym_box.fields(x, y, transpose)
    X, Y = (y, x) if transpose else (x, y)
    W = 0.2 * np.sin(np.pi * z) * (1.0 - Y * Y / 2.25) * np.cos(0.5 * np.pi * X)
    w = np.sin(1.3 * z) * np.exp(-Y * Y) * (0.5 + np.cos(0.7 * X + 0.3))
    ub = np.stack([ub2[0] * (1.0 - 0.3 * z * z), ub2[1] * (1.0 - 0.3 * z * z), W])
    return ub, u2 * (0.3 + np.cos(0.8 * z)), v2 * np.cos(1.1 * z), w


def case(lx1, kind, code="SYM", adjoint=False, transpose=False):
    """(Case3D, state (qx, qy, qz, 0)) of one of KINDS; `code` replaces every 'SYM' ('W': walls; '': the side y = 0 is left
    without a condition -- the end of an extrusion always has one, z = 0 keeps 'SYM')"""
    half_y = kind in ("yhalf", "quarter", "xhalf")
    half_z = kind in ("zhalf", "quarter")
    transpose = transpose or kind == "xhalf"
    c2, _ = sym_box.case(lx1, half_y, code, transpose=transpose, adjoint=adjoint)
    if half_z:
        c3 = mesh3d.extrude_case(c2, 1, 1.0, periodic=False, z0=0.0, zcodes=(code or "SYM", "W"))
    else:
        c3 = mesh3d.extrude_case(c2, 2, 2.0, periodic=False, z0=-1.0)
    ub, u, v, w = fields(c3.x, c3.y, c3.z, transpose)
    c3.ub[:] = ub
    m = (c3.mask,) * 3 if c3.cmask is None else c3.cmask
    n = lx1 - 2
    return c3, (u * m[0], v * m[1], w * m[2], np.zeros((c3.nel, n, n, n)))


def elements(kind, transpose=False):
    """indices of the sub-domain's elements in the full mesh (transposed for xhalf), in the sub-domain's order"""
    h2 = sym_box.half_elements(transpose or kind == "xhalf")
    if kind == "full":
        return np.arange(2 * NEL2)
    if kind in ("yhalf", "xhalf"):
        return np.concatenate([h2, NEL2 + h2])
    if kind == "zhalf":
        return NEL2 + np.arange(NEL2)
    return NEL2 + h2


def mirror(f, plane, sign, transpose=False):
    """the full-domain field f (60, n, n, n) reflected about `plane` ('y': the in-plane symmetry plane of sym_box, 'z': z = 0), times sign"""
    n = f.shape[-1]
    if plane == "z":
        return sign * f.reshape(2, NEL2, n, n, n)[::-1, :, ::-1].reshape(f.shape)
    g = np.stack([np.stack([sym_box.mirror(f[kz * NEL2:(kz + 1) * NEL2, k], 1.0, transpose) for k in range(n)], axis=1) for kz in range(2)])
    return sign * g.reshape(f.shape)


def bm1(c3):
    """diagonal mass matrix (nel, n, n, n) of the case's geometry"""
    from nekstab_amd.quadrature import deriv_matrix, gauss_lobatto_legendre
    zg, w = gauss_lobatto_legendre(c3.lx1)
    D = deriv_matrix(zg)
    d = lambda f: (np.einsum("im,ekjm->ekji", D, f), np.einsum("jm,ekmi->ekji", D, f), np.einsum("km,emji->ekji", D, f))
    (xr, xs, xt), (yr, ys, yt), (zr, zs, zt) = d(c3.x), d(c3.y), d(c3.z)
    J = xr * (ys * zt - yt * zs) - xs * (yr * zt - yt * zr) + xt * (yr * zs - ys * zr)
    return J * w[None, :, None, None] * w[None, None, :, None] * w[None, None, None, :]
