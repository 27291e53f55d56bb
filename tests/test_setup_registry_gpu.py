"""The record of the mutable solver state (dalloc_mut, nsk_ctx::mut): reset_solver_state zeroes it and nsk_clone allocates a
lane from it.  "A reset state equals a fresh context's" is pinned on quadrilaterals by
tests/test_errors_gpu.py::test_kernel_timing_hook_leaves_no_trace_in_the_next_map; here the same for hexahedra, element shards
and lanes, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _cyl6():
    from nekstab_amd import mesh
    case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6)
    m = np.load(os.path.join(GOLDEN, "cylinder_modes.npz"))
    u = m["dRe_u"].astype(np.float64)
    return case, (u[0], u[1], np.zeros((case.nel, 4, 4)))


def _ctx6(case, **kw):
    from nekstab_amd.capi import NekStabHip
    a = dict(tol_helm=1e-12, tol_pres=1e-6, tol_relative=1, nproj=8, max_helm_iter=120, max_pres_iter=192)
    a.update(kw)
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **a)
    h.set_nsteps(5)
    return h


def test_hexahedra_reset_state_equals_a_fresh_context():
    """box_case_3d(2, 2, 2, 6): a 5-step map, nsk_bench_kernel on two kernels of the step, the map again from the same input =
    the map of a fresh context (the record holds dpw, xc, rc_big, the totals and the coarse work vectors besides the core set)."""
    from nekstab_amd import mesh3d
    from nekstab_amd.capi import NekStabHip

    def ubf(x, y, z):
        return np.stack([1.0 - 0.3 * y * y + 0.1 * np.sin(x + z), 0.2 * np.cos(x) * y + 0.1 * z, 0.15 * np.sin(y + 0.5 * z) + 0.05 * x])
    c = mesh3d.box_case_3d(2, 2, 2, 6, lengths=(2.0, 1.0, 0.8), outflow_xmax=True, re=40.0, endtime=0.05, ub_func=ubf, warp=0.06)
    rng = np.random.default_rng(11)
    q = [c.mask * rng.standard_normal(c.x.shape) for _ in range(3)] + [np.zeros((c.nel, 4, 4, 4))]
    out = []
    for dirty in (False, True):
        h = NekStabHip(c, c.meta["vert"], c.meta["nvert"], tol_helm=1e-12, tol_pres=1e-8, tol_relative=1, max_helm_iter=200, max_pres_iter=48, nproj=8)
        try:
            h.set_nsteps(5)
            a, f = h.alloc(2)
            h.upload3(a, *q)
            if dirty:
                h.matvec(f, a, 0)
                for kn in ("helm", "schwarz"):
                    assert h.bench_kernel(kn, 20)["avg_us"] > 0
            h.matvec(f, a, 0)
            out.append(h.download3(f))
        finally:
            h.close()
    assert np.isfinite(out[0][0]).all() and np.abs(out[0][0]).max() > 0
    assert _equal(out[0][:3], out[1][:3])


def test_shards_reset_state_equals_a_freshly_cut_pair():
    """Two virtual ranks of the lx1 = 6 cylinder.  reset_solver_state is reached on shards behind a map that went non-finite
    (group_run_map; the timing hook's dirty flag is read by map_launch, which shards do not pass): a map, a map of a vector with
    a NaN (refused, NSK_ENAN), the first map again = the first map of a freshly cut pair.  The pressure projection space (nproj = 8)
    is kept from map to map, so a state that was not reset shows."""
    from nekstab_amd.capi import NskError
    from nekstab_amd.sharded import ShardGroup
    case, q = _cyl6()
    full = _ctx6(case)
    try:
        def pair():
            g = ShardGroup(full, case, 2)
            g.set_nsteps(5)
            return g
        g = pair()
        a, bad, f = g.alloc(3)
        g.upload(a, *q)
        g.matvec(f, a, 0)
        first = g.download(f)
        g.matvec(f, a, 0)
        warm = g.download(f)
        qx = q[0].copy(); qx[5, 2, 3] = np.nan
        g.upload(bad, qx, q[1], q[2])
        with pytest.raises(NskError) as ei:
            g.matvec(f, bad, 0)
        assert ei.value.code == -3
        g.matvec(f, a, 0)
        again = g.download(f)
        g.close()
        g = pair()
        a, f = g.alloc(2)
        g.upload(a, *q)
        g.matvec(f, a, 0)
        fresh = g.download(f)
        g.close()
        assert np.isfinite(fresh[0]).all()
        assert _equal(first[:2], fresh[:2])
        assert not _equal(warm[:2], fresh[:2])              # (the check can tell a kept state from a reset one)
        assert _equal(again[:2], fresh[:2])
    finally:
        full.close()


@pytest.mark.lanes
def test_lane_state_is_its_own():
    """A lane of an lx1 = 6 context gets its mutable arrays from its parent's record: its first map = a fresh context's first map
    bit for bit, and the parent's next map is what it is without a lane (nsk_clone sets the parent's `tail` to 0: compared with a
    parent of that setting that never had a lane)."""
    case, q = _cyl6()

    def first_map(h, ctx=None):
        a, f = h.alloc(2)
        h.upload(a, *q)
        if ctx is None:
            h.matvec(f, a, 0)
        else:
            h._chk(h.lib.nsk_matvec(ctx, 0, f, a))
        return h.download(f)
    h = _ctx6(case)
    try:
        fresh = first_map(h)
    finally:
        h.close()
    h = _ctx6(case)
    try:
        h.set_option("tail", 0)
        alone = first_map(h)
    finally:
        h.close()
    h = _ctx6(case)
    try:
        k = h.add_lane()
        lane = first_map(h, h._lanes[k])
        parent = first_map(h)
    finally:
        h.close()
    assert np.isfinite(fresh[0]).all()
    assert _equal(lane[:2], fresh[:2])
    assert _equal(parent[:2], alone[:2])
