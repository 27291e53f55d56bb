"""Pins for the 3-D oracle (oracle/linns3d.py): the reference holds no 3-D golden data, so the 3-D
restatement is anchored on the (golden-pinned) 2-D oracle through z-invariance on an extruded mesh,
plus the discrete identities the 3-D-only terms must satisfy on a fully deformed mesh, plus covariance.

The chain that ties the 3-D-only terms to reference-held data:
  1. the 2-D golden fixtures and the Spectre tables pin the 2-D oracle (tests/test_oracle_golden.py) and the quadrilateral kernels;
  2. z-invariance (test_z_invariant_state_steps_like_2d) pins LinNS3D to the 2-D oracle with the spanwise direction on local axis
     t and coordinate z: the u and v equations, the r and s rows of the metric tensor, the r and s directions of the Gauss-mesh
     operators;
  3. covariance (test_oracle_is_covariant_*, helper tests/axes3d.py): relabelling every element's axes (r, s, t) by a proper signed
     permutation and moving the frame by an orthogonal Q must return the same map, re-expressed.  Applied to the extruded case
     this puts the spanwise direction on each local axis and each coordinate in turn, and obliquely, so the w equation, the U_z and
     dU/dz terms of the direct and adjoint convection, the z rows of the metric tensor inside a step and the t direction of the
     Gauss-mesh operators are each held to a term that step 2 pins; applied to a warped box with a fully three-dimensional state
     and base flow it holds every term at once.
tests/test_axes3d_gpu.py carries the same chain to the hexahedral kernels."""
import numpy as np
import pytest

from nekstab_amd import mesh3d
from oracle.linns import LinNS2D
from oracle.linns3d import LinNS3D
from tests import axes3d


_inplane_case = axes3d.inplane_case


def test_z_invariant_state_steps_like_2d():
    c = _inplane_case()
    o3 = LinNS3D(x=c.x, y=c.y, z=c.z, gid=c.gid, nglob=c.nglob, mask=c.mask, ub=c.ub, spng=c.spng, re=c.re,
                 endtime=c.endtime, has_outflow=c.has_outflow)
    nel2 = 6
    sl = (slice(0, nel2), 0)
    g2raw = c.gid[sl]
    _, inv = np.unique(g2raw.ravel(), return_inverse=True)
    gid2 = inv.reshape(g2raw.shape)
    o2 = LinNS2D(x=c.x[sl], y=c.y[sl], gid=gid2, nglob=int(gid2.max()) + 1, mask=c.mask[sl], ub=c.ub[:2, :nel2, 0],
                 spng=c.spng[sl], re=c.re, endtime=c.endtime, has_outflow=c.has_outflow)
    assert o3.nsteps == o2.nsteps and abs(o3.dt - o2.dt) < 1e-15
    assert abs(o3.bm1.sum() - 0.8 * o2.bm1.sum()) < 1e-12
    x2, y2 = c.x[sl], c.y[sl]
    u2 = np.sin(1.3 * x2) * np.cos(2.0 * y2) * c.mask[sl]
    v2 = np.cos(0.7 * x2 + 0.2) * np.sin(3.0 * y2) * c.mask[sl]
    m = c.lx1 - 2
    p2 = o2.J12 @ (0.3 * np.cos(x2) * y2) @ o2.J12.T
    for adjoint in (False, True):
        st2 = o2.new_state((u2, v2, p2))
        q3 = (mesh3d.extrude_field(u2, 2), mesh3d.extrude_field(v2, 2), np.zeros_like(c.x), mesh3d.extrude_pressure(p2, 2))
        st3 = o3.new_state(q3)
        for istep in range(1, 5):
            st2 = o2.step(st2, istep, adjoint)
            st3 = o3.step(st3, istep, adjoint)
        sc = np.abs(st2["u"]).max()
        for k in range(c.lx1):
            for layer in range(2):
                e = slice(layer * nel2, (layer + 1) * nel2)
                assert np.abs(st3["u"][0][e, k] - st2["u"]).max() < 1e-10 * sc
                assert np.abs(st3["u"][1][e, k] - st2["v"]).max() < 1e-10 * sc
        assert np.abs(st3["u"][2]).max() < 1e-11 * sc
        for k in range(m):
            assert np.abs(st3["p"][:nel2, k] - st2["p"]).max() < 1e-9 * np.abs(st2["p"]).max()


def test_discrete_identities_on_deformed_mesh():
    ubf = lambda x, y, z: np.stack([np.sin(x) * np.cos(y), -np.cos(x) * np.sin(y) + 0.2 * z, 0.3 * np.sin(y + z)])
    c = mesh3d.box_case_3d(2, 2, 2, 6, lengths=(1.0, 1.2, 0.9), re=30.0, endtime=0.02, ub_func=ubf, warp=0.08)
    o = LinNS3D(x=c.x, y=c.y, z=c.z, gid=c.gid, nglob=c.nglob, mask=c.mask, ub=c.ub, spng=c.spng, re=c.re,
                endtime=c.endtime, has_outflow=False, build_solvers=False)
    rng = np.random.default_rng(3)
    assert abs(o.bm1.sum() - 1.0 * 1.2 * 0.9) < 1e-9              # faces stay planar under the warp
    u, v = rng.standard_normal(c.x.shape), rng.standard_normal(c.x.shape)
    assert abs(np.sum(v * o.axhelm(u, 0.7, 1.3)) - np.sum(u * o.axhelm(v, 0.7, 1.3))) < 1e-10 * np.abs(u).sum()
    # D^T is the transpose of D
    w = [rng.standard_normal(c.x.shape) for _ in range(3)]
    p = rng.standard_normal((c.nel,) + (4, 4, 4))
    lhs = np.sum(p * o.opdiv(w))
    g = o.opgradt(p)
    rhs = sum(np.sum(g[k] * w[k]) for k in range(3))
    assert abs(lhs - rhs) < 1e-10 * abs(lhs)
    # the weak divergence of a linear (exactly representable) solenoidal field vanishes
    lin = [c.y + 2 * c.z, c.z - c.x, 3 * c.x + c.y]
    assert np.abs(o.opdiv(lin)).max() < 1e-11
    # convection of a linear field by a constant velocity: integral of c.grad(phi) over the box
    cv = [np.full_like(c.x, 0.5), np.full_like(c.x, -1.0), np.full_like(c.x, 2.0)]
    phi = 1.0 * c.x + 2.0 * c.y - 0.5 * c.z
    assert abs(o.convect(cv, phi).sum() - (0.5 - 2.0 - 1.0) * 1.0 * 1.2 * 0.9) < 1e-10


# ---------------- covariance: local axes relabelled, frame moved by an orthogonal matrix (tests/axes3d.py) ----------------
def _oracle(c, solvers=True):
    return LinNS3D(x=c.x, y=c.y, z=c.z, gid=c.gid, nglob=c.nglob, mask=c.mask, ub=c.ub, spng=c.spng, re=c.re,
                   endtime=c.endtime, has_outflow=c.has_outflow, build_solvers=solvers)


def _four_steps(o, q, adjoint):
    st = o.new_state(q)
    for istep in range(1, 5):
        st = o.step(st, istep, adjoint)
    return st["u"], st["p"]


def _check_steps_covariant(c, q, frames, worst):
    """four steps of LinNS3D.step, direct and adjoint, in every frame of ``frames`` = [(name, local, Q)] against the untransformed
    oracle's, carried into the frame: velocity to 1e-10 of the largest |u|, pressure to 1e-9 of the largest |p| (the tolerances of
    test_z_invariant_state_steps_like_2d); the largest deviations go into ``worst``"""
    o = _oracle(c)
    ref = {adj: _four_steps(o, q, adj) for adj in (False, True)}
    for name, local, Q in frames:
        ot = _oracle(axes3d.transform_case(c, local, Q))
        assert ot.nsteps == o.nsteps and abs(ot.dt - o.dt) < 1e-15, name
        assert abs(ot.bm1.sum() - o.bm1.sum()) < 1e-12 * o.bm1.sum(), name
        vt, pt = axes3d.to_frame(q[:3], q[3], local, Q)
        for adj in (False, True):
            u, p = _four_steps(ot, (vt[0], vt[1], vt[2], pt), adj)
            ur, pr = axes3d.to_frame(ref[adj][0], ref[adj][1], local, Q)
            su, sp = max(np.abs(a).max() for a in ur), np.abs(pr).max()
            du, dp = max(np.abs(a - b).max() for a, b in zip(u, ur)) / su, np.abs(p - pr).max() / sp
            worst[0], worst[1] = max(worst[0], du), max(worst[1], dp)
            assert du < 1e-10 and dp < 1e-9, (name, adj, du, dp)
            # and back: from_frame inverts to_frame
            ub, pb = axes3d.from_frame(u, p, local, Q)
            assert max(np.abs(a - b).max() for a, b in zip(ub, ref[adj][0])) < 1e-10 * su, (name, adj)
            assert np.abs(pb - ref[adj][1]).max() < 1e-9 * sp, (name, adj)


_CYCLIC = [np.eye(3), np.roll(np.eye(3), 1, axis=0), np.roll(np.eye(3), 2, axis=0)]


def test_axes3d_helper_is_consistent():
    rel = axes3d.proper_relabellings()
    assert len(rel) == 24 and len(set(rel)) == 24 and all(axes3d.det_local(l) == 1 for l in rel)
    rng = np.random.default_rng(0)
    f = rng.standard_normal((3, 4, 4, 4))
    vert = np.arange(24).reshape(3, 8)
    for l in rel:
        assert np.array_equal(axes3d.relabel(axes3d.relabel(f, l), axes3d.inverse(l)), f)
        assert np.array_equal(axes3d.relabel_vert(axes3d.relabel_vert(vert, l), axes3d.inverse(l)), vert)
        # the corner table follows the nodes: corner c = ir + 2 is + 4 it of the relabelled element is node [it, is, ir] * (n - 1)
        corners = np.arange(8).reshape(1, 2, 2, 2)
        assert np.array_equal(axes3d.relabel(corners, l).ravel(), axes3d.relabel_vert(np.arange(8)[None, :], l).ravel())
    c = axes3d.inplane_case()
    with pytest.raises(AssertionError):
        axes3d.transform_case(c, ((1, 0, 2), (1, 1, 1)), np.eye(3))            # improper: the Jacobian would change sign
    for A in range(3):
        for C in range(3):
            local, Q = axes3d.orientation(A, C, (1, -1, 1))
            t = axes3d.transform_case(c, local, Q)
            assert np.ptp((t.x, t.y, t.z)[C], axis=(1, 2, 3)[2 - A]).max() > 0.1            # the span runs along local axis A, coordinate C
            for a in range(3):
                if a != A:
                    assert np.ptp((t.x, t.y, t.z)[C], axis=(1, 2, 3)[2 - a]).max() == 0.0
    import dataclasses
    cm = dataclasses.replace(c, cmask=np.stack([c.mask, c.mask, np.ones_like(c.mask)]))
    with pytest.raises(ValueError):
        axes3d.transform_case(cm, axes3d.IDENTITY, axes3d.oblique())
    local, Q = axes3d.orientation(0, 1)
    t = axes3d.transform_case(cm, local, Q)
    assert np.array_equal(t.cmask[1], np.ones_like(c.mask)) and np.array_equal(t.cmask[0], axes3d.relabel(c.mask, local))


def test_oracle_is_covariant_under_relabelling_and_rotation():
    """The extruded, in-plane curved case with its two-dimensional base flow and a three-dimensional state: all 24 proper
    relabellings in the original frame, the three cyclic coordinate permutations (each with the cyclic relabelling of the same
    power, so the spanwise direction visits every local axis and every coordinate) and one oblique rotation."""
    c = _inplane_case()
    x, y, z = c.x, c.y, c.z
    kz = 2.0 * np.pi / 0.8
    q = [np.sin(1.3 * x + kz * z) * np.cos(2.0 * y) * c.mask, np.cos(0.7 * x + 0.2) * np.sin(3.0 * y - kz * z) * c.mask,
         np.sin(x + y) * np.cos(kz * z) * c.mask]
    J12 = LinNS3D(x=c.x, y=c.y, z=c.z, gid=c.gid, nglob=c.nglob, mask=c.mask, ub=c.ub, spng=c.spng, re=c.re, endtime=c.endtime,
                  has_outflow=True, build_solvers=False)._to2
    q.append(J12(0.3 * np.cos(x) * y * (1.0 + 0.5 * np.sin(kz * z)), -1))
    cyc = ((0, 1, 2), (1, 2, 0), (2, 0, 1))
    frames = [("relabelling %s %s" % l, l, np.eye(3)) for l in axes3d.proper_relabellings()]
    frames += [("cyclic %d" % k, (cyc[k], (1, 1, 1)), _CYCLIC[k]) for k in range(3)]
    frames += [("oblique", (cyc[1], (1, 1, 1)), axes3d.oblique())]
    worst = [0.0, 0.0]
    _check_steps_covariant(c, q, frames, worst)
    print("extruded case, 28 frames, four steps direct and adjoint: largest deviation velocity %.2e, pressure %.2e" % tuple(worst))


def test_oracle_is_covariant_on_a_warped_box_with_a_general_state():
    """The warped 3 x 2 x 2 outflow box of tests/test_3d_gpu.py with its fully three-dimensional base flow, sponge and state (every
    metric term, every base-flow gradient non-zero): one oblique rotation and two relabellings with flips, the operators
    (no solves) at the 1e-12 the GPU tests hold the kernels to, then four steps direct and adjoint."""
    from tests.test_3d_gpu import _case
    c = _case(6, True)
    c.spng = 0.4 * np.clip(c.x - 1.4, 0.0, None) ** 2
    x, y, z = c.x, c.y, c.z
    q = [np.sin(1.3 * x + z) * np.cos(2.0 * y) * c.mask, np.cos(0.7 * x + 0.2) * np.sin(3.0 * y - z) * c.mask,
         np.sin(x + y) * np.cos(2.0 * z) * c.mask]
    frames = [("oblique", axes3d.IDENTITY, axes3d.oblique()),
              ("x'=z y'=x z'=y, r<->s, t flipped", ((1, 0, 2), (1, 1, -1)), _CYCLIC[1]),
              ("oblique 11, s<->t, s flipped", ((0, 2, 1), (1, -1, 1)), axes3d.oblique(11))]
    o = _oracle(c, solvers=False)
    q.append(o._to2(0.3 * np.cos(x) * y + 0.2 * np.sin(z), -1))
    rng = np.random.default_rng(8)
    u = rng.standard_normal((3,) + c.x.shape)
    p = rng.standard_normal((c.nel, 4, 4, 4))
    rel = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max()
    worst = 0.0
    for name, local, Q in frames:
        ct = axes3d.transform_case(c, local, Q)
        ot = _oracle(ct, solvers=False)
        ut, pt = axes3d.to_frame(u, p, local, Q)
        vec = lambda w: np.stack(axes3d.to_frame(w, None, local, Q)[0])
        sca = lambda f: axes3d.relabel(f, local)
        errs = dict(axhelm=rel(ot.axhelm(sca(u[0]), 0.7, 1.3), sca(o.axhelm(u[0], 0.7, 1.3))),
                    opdiv=rel(ot.opdiv(ut), sca(o.opdiv(u))),
                    opgradt=rel(np.stack(ot.opgradt(pt)), vec(o.opgradt(p))),
                    convect=rel(ot.convect(ut, sca(u[1])), sca(o.convect(u, u[1]))),
                    convect_base=rel(np.stack([ot.convect(ot.ub, ut[k]) for k in range(3)]), vec([o.convect(o.ub, u[k]) for k in range(3)])),
                    convect_adj=rel(np.stack(ot.convect_adj(ut, ot.ub)), vec(o.convect_adj(u, o.ub))))
        print(name, {k: "%.1e" % v for k, v in errs.items()})
        worst = max(worst, max(errs.values()))
        assert max(errs.values()) < 1e-12, (name, errs)
    w2 = [0.0, 0.0]
    _check_steps_covariant(c, q, frames, w2)
    print("warped box: largest operator deviation %.2e; four steps: velocity %.2e, pressure %.2e" % (worst, w2[0], w2[1]))
