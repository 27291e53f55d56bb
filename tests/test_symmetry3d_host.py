"""Symmetry boundaries on hexahedra, host side: mesh3d.box_case_3d(sym=...), mesh3d.extrude_case with a 2-D case that carries
component masks and with `zcodes`, the noise seed ('SYM' fixes the component along the face normal, 'ON ' the other two; a node
fixed in any copy is fixed in all, per component: [UPSTREAM bcmask, non-stress branch])."""
from dataclasses import replace

import numpy as np
import pytest

from nekstab_amd import mesh3d, seed
from tests import sym_box, sym_box3d

FACES = ("xmin", "xmax", "ymin", "ymax", "zmin", "zmax")


def _on(c, name):
    X = (c.x, c.y, c.z)["xyz".index(name[0])]
    return np.isclose(X, X.min() if name.endswith("min") else X.max(), atol=1e-12)


@pytest.mark.parametrize("warp", [0.0, 0.05])
@pytest.mark.parametrize("code", ["SYM", "ON "])
@pytest.mark.parametrize("face", FACES)
def test_box_face_loses_exactly_its_components(face, code, warp):
    kw = dict(lengths=(1.0, 1.5, 2.0), origin=(-0.5, 0.0, 0.25), warp=warp)
    walls = mesh3d.box_case_3d(2, 3, 2, 5, **kw)
    c = mesh3d.box_case_3d(2, 3, 2, 5, sym={face: code}, **kw)
    assert walls.cmask is None and c.cmask is not None and c.cmask.shape == (3, 12, 5, 5, 5)
    for name in ("x", "y", "z", "gid", "ub", "spng"):
        assert np.array_equal(getattr(c, name), getattr(walls, name))
    a = "xyz".index(face[0])
    fixed = (a,) if code == "SYM" else tuple(k for k in range(3) if k != a)
    here = _on(c, face)
    other = np.zeros_like(here)
    for f in FACES:
        if f != face:
            other |= _on(c, f)
    assert here.sum() == 25 * {0: 3 * 2, 1: 2 * 2, 2: 2 * 3}[a]         # the nodes of the elements' faces on that side, no other
    for k in range(3):
        assert np.array_equal(c.cmask[k][~here], walls.mask[~here])       # nothing changes off the face
        assert np.all(c.cmask[k][here & other] == 0.0)                    # an edge shared with a wall: every component fixed
        assert np.all(c.cmask[k][here & ~other] == (0.0 if k in fixed else 1.0))
    assert np.array_equal(c.mask, c.cmask[0] * c.cmask[1] * c.cmask[2])


def test_box_without_sym_is_unchanged_and_bad_input_is_refused():
    a = mesh3d.box_case_3d(2, 2, 3, 6, warp=0.03, outflow_xmax=True)
    b = mesh3d.box_case_3d(2, 2, 3, 6, warp=0.03, outflow_xmax=True, sym=None)
    bnd = _on(a, "xmin") | _on(a, "ymin") | _on(a, "ymax") | _on(a, "zmin") | _on(a, "zmax")
    assert a.cmask is None and b.cmask is None and np.array_equal(a.mask, b.mask) and np.array_equal(a.mask, 1.0 - bnd)
    with pytest.raises(ValueError):
        mesh3d.box_case_3d(2, 2, 2, 5, sym=dict(top="SYM"))
    with pytest.raises(ValueError):
        mesh3d.box_case_3d(2, 2, 2, 5, sym=dict(zmin="W"))
    with pytest.raises(ValueError):
        mesh3d.box_case_3d(2, 2, 2, 5, periodic=(False, False, True), sym=dict(zmin="SYM"))
    with pytest.raises(ValueError):
        mesh3d.box_case_3d(2, 2, 2, 5, outflow_xmax=True, sym=dict(xmax="SYM"))
    # two symmetry planes meet: on their edge only the component along it stays free
    c = mesh3d.box_case_3d(2, 2, 2, 5, sym=dict(ymin="SYM", zmin="SYM"))
    edge = _on(c, "ymin") & _on(c, "zmin") & ~_on(c, "xmin") & ~_on(c, "xmax")
    assert np.all(c.cmask[0][edge] == 1.0) and np.all(c.cmask[1][edge] == 0.0) and np.all(c.cmask[2][edge] == 0.0)


def test_extrusion_third_component_is_tangential():
    for code, wfree in (("SYM", 1.0), ("ON ", 0.0)):
        c2, _ = sym_box.case(6, True, code)
        c3 = mesh3d.extrude_case(c2, 2, 2.0, periodic=False, z0=-1.0)
        assert c3.cmask is not None and c3.cmask.shape == (3, 30, 6, 6, 6)
        ends = np.isclose(np.abs(c3.z), 1.0)
        for k in range(2):                                                # components 0 and 1: extruded, fixed on the end walls
            assert np.array_equal(c3.cmask[k], mesh3d.extrude_field(c2.cmask[k], 2) * ~ends)
        plane = np.isclose(c3.y, 0.0, atol=1e-13)
        both = mesh3d.extrude_field(1.0 * ((c2.cmask[0] == 0.0) & (c2.cmask[1] == 0.0)), 2) == 1.0      # inflow 'v', wall 'W' (warped: not y = const)
        assert both.sum() > 0 and np.isclose(c3.x, 0.0, atol=1e-13).sum() == (both & np.isclose(c3.x, 0.0, atol=1e-13)).sum()
        assert np.all(c3.cmask[2][plane & ~both & ~ends] == wfree)        # free on 'SYM', fixed on 'ON '
        assert np.all(c3.cmask[2][both | ends] == 0.0)                    # faces that fix both 2-D components; the end walls
        assert np.all(c3.cmask[2][~(plane | both | ends)] == 1.0)         # everything else, the outflow 'O' included
        assert (np.isclose(c3.x, 4.0, atol=1e-13) & ~(plane | both | ends)).sum() > 0
        # default zcodes: the shared mask is what the extrusion gave before component masks existed
        old = mesh3d.extrude_case(replace(c2, cmask=None), 2, 2.0, periodic=False, z0=-1.0)
        assert old.cmask is None and np.array_equal(c3.mask, old.mask)
        per = mesh3d.extrude_case(c2, 2, 2.0)
        assert np.array_equal(per.mask, mesh3d.extrude_case(replace(c2, cmask=None), 2, 2.0).mask)
        assert np.all(per.cmask[2][np.isclose(per.y, 0.0, atol=1e-13) & ~np.isclose(per.x, 0.0, atol=1e-13)] == wfree)


def test_extrusion_without_component_masks_is_unchanged():
    c2, _ = sym_box.case(6, False)
    a = mesh3d.extrude_case(c2, 2, 2.0, periodic=False, z0=-1.0)
    b = mesh3d.extrude_case(c2, 2, 2.0, periodic=False, z0=-1.0, zcodes=("W", "W"))
    m = mesh3d.extrude_field(c2.mask, 2) * ~np.isclose(np.abs(a.z), 1.0)
    assert a.cmask is None and b.cmask is None and np.array_equal(a.mask, m) and np.array_equal(b.mask, m)


def test_face_codes_are_needed():
    """the masks alone do not tell 'SYM' from 'ON ': without the codes the extrusion of a case with component masks is refused"""
    for code in ("ON ", "SYM"):
        c2, _ = sym_box.case(6, True, code)
        assert len(c2.meta["face_codes"]) == 2 * 5 + 2 * 3 and sum(cd == code for _, _, cd in c2.meta["face_codes"]) == 5
        meta = {k: v for k, v in c2.meta.items() if k != "face_codes"}
        with pytest.raises(ValueError, match="face codes"):
            mesh3d.extrude_case(replace(c2, meta=meta), 2, 2.0)
    full, _ = sym_box.case(6, False)                                       # no component masks: no codes needed
    meta = {k: v for k, v in full.meta.items() if k != "face_codes"}
    assert np.array_equal(mesh3d.extrude_case(replace(full, meta=meta), 2, 2.0).mask, mesh3d.extrude_case(full, 2, 2.0).mask)


def test_refinement_carries_the_face_codes():
    """refine_case_2x2 hands a parent's face code to the two children on that side: extruding the refined half channel gives the
    third component the rule applied to the refined mesh (free on the 'SYM' plane, fixed where both 2-D components are)"""
    from nekstab_amd import mesh
    for code, wfree in (("SYM", 1.0), ("ON ", 0.0)):
        c2, _ = sym_box.case(6, True, code)
        r2 = mesh.refine_case_2x2(c2)
        codes = r2.meta["face_codes"]
        assert len(codes) == 2 * len(c2.meta["face_codes"]) and len(set((e, f) for e, f, _ in codes)) == len(codes)
        for e, f, cd in codes:                                             # every coded face of a child lies on the parent's boundary
            sel = mesh._face_nodes(f)
            k = {"v": (0, 1), "W": (0, 1), "O": (), "SYM": (1,), "ON": (0,)}[cd.strip()]
            assert all(np.all(r2.cmask[c][e][sel][1:-1] == 0.0) for c in k)
        r3 = mesh3d.extrude_case(r2, 2, 2.0)
        both = mesh3d.extrude_field(1.0 * ((r2.cmask[0] == 0.0) & (r2.cmask[1] == 0.0)), 2) == 1.0
        plane = np.isclose(r3.y, 0.0, atol=1e-12)
        assert plane.sum() == 2 * 10 * 6 * 6 and np.all(r3.cmask[2][plane & ~both] == wfree)
        assert np.all(r3.cmask[2][both] == 0.0) and np.all(r3.cmask[2][~(plane | both)] == 1.0)


def test_zcodes():
    c2, _ = sym_box.case(6, False)
    with pytest.raises(ValueError):
        mesh3d.extrude_case(c2, 2, 2.0, zcodes=("SYM", "W"))             # periodic
    with pytest.raises(ValueError):
        mesh3d.extrude_case(c2, 1, 1.0, periodic=False, zcodes=("v", "W"))
    with pytest.raises(ValueError):
        mesh3d.extrude_case(c2, 1, 1.0)                                   # periodic needs two layers
    for lo, fixed in (("SYM", (2,)), ("ON ", (0, 1))):
        c3 = mesh3d.extrude_case(c2, 1, 1.0, periodic=False, z0=0.0, zcodes=(lo, "W"))       # nz = 1 is legal
        assert c3.nel == 30 and c3.nglob == c2.nglob * 6 and c3.cmask.shape == (3, 30, 6, 6, 6)
        z0, z1 = c3.z == 0.0, np.isclose(c3.z, 1.0)
        lat = mesh3d.extrude_field(c2.mask, 1)
        for k in range(3):
            assert np.array_equal(c3.cmask[k][~(z0 | z1)], lat[~(z0 | z1)]) and np.all(c3.cmask[k][z1] == 0.0)
            assert np.array_equal(c3.cmask[k][z0], 0.0 * lat[z0] if k in fixed else lat[z0])       # a lateral wall still fixes everything


def test_quarter_has_three_different_masks_and_matches_the_full_domain():
    full, qf = sym_box3d.case(6, "full")
    wf = sym_box3d.bm1(full)
    assert full.cmask is None and full.nel == 60 and np.all(wf > 0)
    for kind in ("yhalf", "zhalf", "quarter"):
        c, q = sym_box3d.case(6, kind)
        el = sym_box3d.elements(kind)
        assert c.nel == len(el) and c.cmask is not None
        for a, b in ((c.x, full.x), (c.y, full.y), (c.z, full.z), (c.ub, full.ub), (sym_box3d.bm1(c), wf)):
            assert np.allclose(a, b[..., el, :, :, :], atol=1e-13)
        for k in range(4):
            assert np.allclose(q[k], qf[k][el], atol=1e-13)
    xf, qxf = sym_box3d.case(6, "full", transpose=True)
    xh, qxh = sym_box3d.case(6, "xhalf")
    el = sym_box3d.elements("xhalf")
    assert np.allclose(xh.x, xf.x[el], atol=1e-13) and np.allclose(xh.ub, xf.ub[:, el], atol=1e-13) and all(np.allclose(a, b[el], atol=1e-13) for a, b in zip(qxh, qxf))
    assert np.all(xh.cmask[0][np.isclose(xh.x, 0.0, atol=1e-13)] == 0.0)
    # parities of the full-domain fields about both planes: u even / even, v odd in y, w odd in z
    for plane, sg in (("y", (1.0, -1.0, 1.0)), ("z", (1.0, 1.0, -1.0))):
        for k in range(3):
            assert np.abs(qf[k]).max() > 0.1 and np.abs(full.ub[k]).max() > 0.05
            assert np.allclose(sym_box3d.mirror(qf[k], plane, sg[k]), qf[k], atol=1e-13)
            assert np.allclose(sym_box3d.mirror(full.ub[k], plane, sg[k]), full.ub[k], atol=1e-13)
    assert np.allclose(sym_box3d.mirror(qxf[0], "y", -1.0, True), qxf[0], atol=1e-13)
    c, q = sym_box3d.case(6, "quarter")
    edge = np.isclose(c.y, 0.0, atol=1e-13) & (c.z == 0.0) & ~np.isclose(c.x, 0.0, atol=1e-13)
    assert edge.sum() > 0 and np.all(c.cmask[0][edge] == 1.0) and np.all(c.cmask[1][edge] == 0.0) and np.all(c.cmask[2][edge] == 0.0)
    assert not np.array_equal(c.cmask[0], c.cmask[1]) and not np.array_equal(c.cmask[1], c.cmask[2]) and not np.array_equal(c.cmask[0], c.cmask[2])
    walledge = np.isclose(c.y, c.y.max()) & (c.z == 0.0)                  # wall meets 'SYM'
    assert walledge.sum() > 0 and all(np.all(c.cmask[k][walledge] == 0.0) for k in range(3))


def test_noise_seed_takes_three_masks_on_the_quarter():
    c, _ = sym_box3d.case(6, "quarter")
    q = seed.add_noise(c)
    assert len(q) == 3
    shared = replace(c, cmask=None)
    s = seed.add_noise(shared)
    for k in range(3):
        assert np.all(q[k][c.cmask[k] == 0.0] == 0.0) and np.all(q[k][c.cmask[k] == 1.0] != 0.0)
        assert np.array_equal(q[k] * c.mask, s[k])
    yplane = np.isclose(c.y, 0.0, atol=1e-13)
    assert np.abs(q[0][yplane]).max() > 0 and np.abs(q[2][yplane]).max() > 0 and np.all(s[0][yplane] == 0.0)
