"""Meshes of irregular topology for the gather-scatter branches (tests/test_irregular_host.py, test_irregular_gpu.py,
test_irregular3d_gpu.py): a fan of k quadrilaterals around one vertex, and its extrusion in z.

A regular 2k-gon of circumradius 1: its even points are the side midpoints (radius cos(pi / k)), its odd points the corners.  It is
cut from the centre into k quadrilaterals (centre, midpoint, corner, next midpoint), counter-clockwise: the centre vertex has
valence k.  rings = 2 adds the 2k quadrilaterals between that polygon and the same polygon at radius 2 (3k elements): the corners of
ring 0 then have valence 3, its midpoints 4.  Every vertex but the centre is moved by
    X = x + 0.07 sin(1.3 x + 0.4) cos(0.9 y),    Y = y + 0.07 cos(0.8 x) sin(1.1 y + 0.2)
so that no two elements are congruent and every metric term is non-zero; the elements stay convex for k = 3 .. 9.
'W' on the outer boundary except for the outer faces of element 0 (one ring) / of the last two elements (two rings), which are 'O'.

Copies per node: a node's number of local copies is what decides the gather's code path (4-wide table, corner lists of 8, CSR walk).
In the extrusion over nz layers a vertex on the axis has k copies at a wall end and 2k between two layers (or everywhere, periodic);
the nodes of the axis' edges have k copies and are no element corners."""
import numpy as np

from nekstab_amd import mesh, mesh3d, nekio

RE = 40.0
ENDTIME = 0.05
LZ = 0.8


def _move(x, y):
    return x + 0.07 * np.sin(1.3 * x + 0.4) * np.cos(0.9 * y), y + 0.07 * np.cos(0.8 * x) * np.sin(1.1 * y + 0.2)


def fan(k, rings=1):
    """(Re2Mesh, vlex) of the fan of k quadrilaterals, with `rings` = 1 or 2"""
    assert k >= 3 and rings in (1, 2)
    th = np.pi * np.arange(2 * k + 1) / k
    rad = np.where(np.arange(2 * k + 1) % 2 == 0, np.cos(np.pi / k), 1.0)
    px, py = rad * np.cos(th), rad * np.sin(th)                     # point 2k = point 0
    ex, ey = [], []
    for i in range(k):
        j = 2 * i
        ex.append([0.0, px[j], px[j + 1], px[j + 2]])
        ey.append([0.0, py[j], py[j + 1], py[j + 2]])
    if rings == 2:
        for j in range(2 * k):
            ex.append([px[j], 2.0 * px[j], 2.0 * px[j + 1], px[j + 1]])
            ey.append([py[j], 2.0 * py[j], 2.0 * py[j + 1], py[j + 1]])
    ex, ey = np.array(ex), np.array(ey)
    centre = (ex == 0.0) & (ey == 0.0)
    mx, my = _move(ex, ey)
    xc, yc = np.where(centre, 0.0, mx), np.where(centre, 0.0, my)
    nel = xc.shape[0]
    bcs = []
    if rings == 1:
        for e in range(k):
            for f in (1, 2):
                bcs.append((e, f, np.zeros(5), "O" if e == 0 else "W"))
    else:
        for e in range(k, nel):
            bcs.append((e, 1, np.zeros(5), "O" if e >= nel - 2 else "W"))
    m = nekio.Re2Mesh(2, nel, xc, yc, None, [], bcs)
    return m, mesh.vertex_ids_from_coords(m)


def area(m):
    """shoelace area of the mesh"""
    x, y = m.xc, m.yc
    return 0.5 * float(np.sum(x * np.roll(y, -1, axis=1) - np.roll(x, -1, axis=1) * y))


def baseflow2(x, y):
    """a smooth base flow with no symmetry of the fan"""
    return np.stack([1.0 - 0.2 * y * y + 0.15 * np.sin(0.9 * x + 0.3 * y), 0.25 * np.cos(0.7 * x) * y + 0.1 * np.sin(1.1 * x - 0.4)])


def baseflow3(x, y, z):
    """the three-dimensional base flow of tests/test_3d_gpu.py (`_ubf`)"""
    return np.stack([1.0 - 0.3 * y * y + 0.1 * np.sin(x + z), 0.2 * np.cos(x) * y + 0.1 * z, 0.15 * np.sin(y + 0.5 * z) + 0.05 * x])


def case2(k, rings, lx1, adjoint=False):
    """quadrilateral Case on fan(k, rings): Re = 40, no sponge, base flow `baseflow2`"""
    m, vlex = fan(k, rings)
    x, y = mesh.element_coords_2d(m, lx1)
    return mesh.build_case_2d(m, vlex, baseflow2(x, y), lx1, adjoint=adjoint, endtime=ENDTIME, re=RE, spng_str=0.0)


def fan3(k, nz, lx1, periodic=False):
    """hexahedral Case3D: the one-ring fan extruded over nz layers of total height 0.8, walls at both ends or periodic,
    base flow `baseflow3`"""
    c3 = mesh3d.extrude_case(case2(k, 1, lx1), nz, LZ, periodic=periodic, zcodes=("W", "W"))
    c3.ub = baseflow3(c3.x, c3.y, c3.z)
    return c3


def census(gid, ndim):
    """{copies: (nodes that are element corners, nodes that are not)} over the global nodes of `gid`"""
    n = gid.shape[-1]
    cnt = np.bincount(gid.ravel())
    corner = np.zeros(cnt.size, dtype=bool)
    ends = np.ix_(*([[0, n - 1]] * ndim))
    corner[gid[(slice(None),) + ends].ravel()] = True
    out = {}
    for c in np.unique(cnt[cnt > 0]):
        sel = cnt == c
        out[int(c)] = (int(np.sum(sel & corner)), int(np.sum(sel & ~corner)))
    return out


def centre_node(c):
    """global id of a node with the largest number of copies (on the fan's axis)"""
    return int(np.argmax(np.bincount(c.gid.ravel())))
