"""The mirror-symmetric channel of the symmetry-boundary tests (tests/test_symmetry_host.py, tests/test_symmetry_gpu.py).

5 x 6 straight-sided elements on x in [0, 4], y in [-1.5, 1.5], vertices moved by
    X = x + 0.15 sin(pi x / 4) cos(pi y / 1.5),    Y = y (1 + 0.1 sin(pi x / 4)):
y = 0 stays flat, every metric term is non-zero, and 30 / 15 elements leave a partial workgroup at every elements-per-workgroup
count (7, 4, 2 at lx1 = 6, 8, 10).  'v' at x = 0, 'O' at x = 4, 'W' at y = +-1.5.  The half mesh is the 15 elements with
y >= 0 in the same order with `code` ('SYM') on their y = 0 faces.  transpose = True: coordinates and components swapped
(the symmetry plane is then x = 0, its normal component is component 0); box_mesh_2d keeps the corners counter-clockwise.

A frozen base flow with U even and V odd in y and a state with u even, v odd keep the full-domain solution in the symmetric
subspace; the half domain with 'SYM' on y = 0 is the Galerkin restriction to that subspace."""
import numpy as np

from nekstab_amd import mesh

NX, NY = 5, 6
RE = 40.0


def _warp(i, j, j0):
    x = 4.0 * i / NX
    y = -1.5 + 3.0 * (j + j0) / NY
    return x + 0.15 * np.sin(np.pi * x / 4.0) * np.cos(np.pi * y / 1.5), y * (1.0 + 0.1 * np.sin(np.pi * x / 4.0))


def box(half, code="SYM", transpose=False):
    """(Re2Mesh, vlex) of the full (half = False) or the half channel; code = '' leaves the y = 0 side without a condition."""
    ny, j0 = (NY // 2, NY // 2) if half else (NY, 0)
    ymin = code if half else "W"
    if not transpose:
        return mesh.box_mesh_2d(NX, ny, lambda i, j: _warp(i, j, j0), dict(xmin="v", xmax="O", ymin=ymin, ymax="W"))

    def xy(i, j):                          # vertex (i, j) of the transposed mesh = vertex (j, i) of the original, (X, Y) swapped
        X, Y = _warp(j, i, j0)
        return Y, X
    return mesh.box_mesh_2d(ny, NX, xy, dict(ymin="v", ymax="O", xmin=ymin, xmax="W"))


def half_elements(transpose=False):
    """indices of the half's elements in the full mesh, in the half's order"""
    if not transpose:
        return np.arange(NX * NY // 2, NX * NY)
    ex, ey = np.meshgrid(np.arange(NY // 2), np.arange(NX), indexing="xy")
    return ((ex + NY // 2) + NY * ey).ravel()


def fields(x, y, transpose=False):
    """base flow (2, ...) from psi = (Y - Y^3 / 6.75) (1 + 0.3 sin(pi X / 2)) and a smooth state (u, v) with u even, v odd in Y,
    most of u's weight on the centreline; transposed: (X, Y) and the components swapped"""
    X, Y = (y, x) if transpose else (x, y)
    U = (1.0 - Y * Y / 2.25) * (1.0 + 0.3 * np.sin(0.5 * np.pi * X))
    V = -(Y - Y ** 3 / 6.75) * 0.15 * np.pi * np.cos(0.5 * np.pi * X)
    u = np.exp(-2.0 * Y * Y) * (0.6 + np.sin(1.3 * X + 0.4)) + 0.2 * np.cos(2.1 * Y) * np.cos(0.7 * X)
    v = np.sin(1.7 * Y) * np.cos(0.9 * X + 0.2) * np.exp(-0.5 * Y * Y)
    return (np.stack([V, U]), v, u) if transpose else (np.stack([U, V]), u, v)


def case(lx1, half, code="SYM", transpose=False, adjoint=False):
    """Case (Re = 40, no sponge) and its state (qx, qy, 0) = the smooth state times the (component) masks"""
    m, vlex = box(half, code, transpose)
    x, y = mesh.element_coords_2d(m, lx1)
    ub, _, _ = fields(x, y, transpose)
    c = mesh.build_case_2d(m, vlex, ub, lx1, adjoint=adjoint, endtime=1.0, re=RE, spng_str=0.0)
    _, u, v = fields(c.x, c.y, transpose)
    m0, m1 = (c.mask, c.mask) if c.cmask is None else (c.cmask[0], c.cmask[1])
    return c, (u * m0, v * m1, np.zeros((c.nel, lx1 - 2, lx1 - 2)))


def mirror(f, sign, transpose=False):
    """the full-domain field f (nel, n, n) reflected about the symmetry plane, times sign"""
    n = f.shape[-1]
    if not transpose:
        g = f.reshape(NY, NX, n, n)[::-1, :, ::-1, :]
    else:
        g = f.reshape(NX, NY, n, n)[:, ::-1, :, ::-1]
    return sign * g.reshape(f.shape)
