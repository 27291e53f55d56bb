"""Option "idx_first": B_j of the quadrilateral pressure iteration on its compact argument block (k_divgs_t_l<.., true>) loads its
gather-table entry together with the convergence flag, issues the gathers through it first behind the flag test and stages the
coarse values behind the first contraction pass.  Only the order of the loads changes, no operation and no summation order:
every comparison here is np.array_equal, option 1 against option 0 in one build, on the cylinder fixture: the state after maps
of 6 time steps and the per-step iteration counts.  (A_j, k_schwarz_uc_l, keeps its order: the same change there measured
nothing.)"""
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

NSTEPS = 6
_CASES = {}


def _case(lx1, adjoint=False):
    key = (lx1, bool(adjoint))
    if key not in _CASES:
        from nekstab_amd import mesh
        _CASES[key] = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), lx1, adjoint=bool(adjoint))
    return _CASES[key]


def _seed(case):
    from nekstab_amd import seed
    qx, qy = seed.add_noise(case)
    m = case.lx1 - 2
    return qx, qy, np.zeros((case.nel, m, m))


def _maps(h, case, mode, nmaps):
    """nmaps consecutive maps of NSTEPS steps: every output, the per-step iteration counts of every map, the statistics"""
    h.set_nsteps(NSTEPS)
    v = h.alloc(nmaps + 1)
    h.upload(v[0], *_seed(case))
    h.scal(v[0], 1.0 / h.norm(v[0]))
    outs, iters = [], []
    for k in range(nmaps):
        h.matvec(v[k + 1], v[k], mode)
        outs.append(h.download(v[k + 1]))
        hh, pp = h.step_iters()
        iters.append((hh.copy(), pp.copy()))
    return dict(outs=outs, iters=iters, stats=h.stats())


def _run(case, mode, first, options=(), nmaps=1, **ctx):
    from nekstab_amd.settings import production_context
    h = production_context(case, **ctx)
    try:
        if first is not None:
            h.set_option("idx_first", first)
        for k, val in options:
            h.set_option(k, val)
        return _maps(h, case, mode, nmaps)
    finally:
        h.close()


def _bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _same(a, b):
    assert len(a["outs"]) == len(b["outs"])
    for fa, fb in zip(a["outs"], b["outs"]):
        assert np.abs(fa[0]).max() > 0 and np.all(np.isfinite(fa[0])) and _bits(fa, fb)
    for (ha, pa), (hb, pb) in zip(a["iters"], b["iters"]):
        assert ha[:NSTEPS].min() > 0 and pa[:NSTEPS].min() > 0                  # both solves iterated in every step
        assert np.array_equal(ha, hb) and np.array_equal(pa, pb)                # the same iteration counts, step by step


def _counts(off, on, nmaps=1):
    """the new order ran with 1 and not with 0 (a redone map counts again)"""
    assert off["stats"]["idxfirst_steps"] == 0
    if on["stats"]["retries"] == 0:
        assert on["stats"]["idxfirst_steps"] == nmaps * NSTEPS
    else:
        assert on["stats"]["idxfirst_steps"] >= (nmaps + 1) * NSTEPS


@pytest.mark.parametrize("lx1", [6, 8, 10, 12])
@pytest.mark.parametrize("mode", [0, 1])
def test_every_instantiation_bit_for_bit(lx1, mode):
    """k_divgs_t_l<N, false, false, true> of every lx1, direct and adjoint.  lx1 = 8 runs the instantiation of the benchmark;
    lx1 = 12 takes the new order with option 1 only."""
    case = _case(lx1, mode)
    off = _run(case, mode, 0)
    on = _run(case, mode, 1)
    print("lx1", lx1, "mode", mode, "idx_first steps", on["stats"]["idxfirst_steps"], "iterations", on["iters"][0][0][:NSTEPS].tolist(), on["iters"][0][1][:NSTEPS].tolist())
    _counts(off, on)
    assert on["stats"]["leanargs_steps"] == on["stats"]["idxfirst_steps"]        # exactly where the compact blocks run
    _same(off, on)


def test_component_masks():
    """nsk_init_masks, lx1 = 6: k_divgs_t_l<6, false, true, true> (the CM instantiation of B).  The second component gets a
    Dirichlet condition of its own on the nodes of the lowest grid line, so that the two masks differ."""
    from dataclasses import replace
    case = _case(6)
    m1 = case.mask * (case.y > case.y.min() + 1e-12)
    assert not np.array_equal(m1, case.mask)
    cm = replace(case, cmask=np.stack([case.mask, m1]))
    off = _run(cm, 0, 0)
    on = _run(cm, 0, 1)
    _counts(off, on)
    _same(off, on)
    assert not _bits(on["outs"][0], _run(case, 0, 1)["outs"][0])        # the second mask was used


def test_start_in_a0_and_projection_restart():
    """lx1 = 8, nproj = 3, two maps: every solve starts inside A_0 (uc_start: row 0 of the partials alone, the flag still the
    previous solve's), and the projection space fills and restarts within a map."""
    case = _case(8)
    off = _run(case, 0, 0, nmaps=2, nproj=3)
    on = _run(case, 0, 1, nmaps=2, nproj=3)
    assert on["stats"]["absorb_maps"] >= 2 and off["stats"]["absorb_maps"] == on["stats"]["absorb_maps"]
    _counts(off, on, nmaps=2)
    _same(off, on)


def test_tails_keep_the_old_order():
    """lx1 = 8, four maps, tail = 1 with the heads pushed far below the iteration counts: k_pres_tail2 runs most iterations on
    the shared body in today's order, behind heads in the new order -- bit-identical with option 0."""
    case = _case(8)
    opts = [("tail", 1), ("tail_off_h", -16), ("tail_off_p", -3)]
    off = _run(case, 0, 0, opts, nmaps=4)
    on = _run(case, 0, 1, opts, nmaps=4)
    print("tail maps", on["stats"]["tail_maps"], "heads per step %.2f / %.2f" % (on["stats"]["step_budget_helm_mean"], on["stats"]["step_budget_pres_mean"]),
          "retries", on["stats"]["retries"])
    assert on["stats"]["tail_maps"] >= 1 and off["stats"]["tail_maps"] == on["stats"]["tail_maps"]
    later_p = np.mean([pp[:NSTEPS].mean() for _, pp in on["iters"][1:]])
    print("pressure iterations per step of maps 2 to 4: %.2f" % later_p)
    assert on["stats"]["step_budget_pres_mean"] < later_p                # the pressure tail ran iterations
    _counts(off, on, nmaps=4)
    _same(off, on)


@pytest.mark.parametrize("what", ["eager", "hostcheck"])
def test_eager_steps(what):
    """Steps launched one by one (use_graph = 0) and host-checked steps take the new order too."""
    case = _case(8)
    opts = {"eager": [("use_graph", 0)], "hostcheck": [("hostcheck", 1)]}[what]
    off = _run(case, 0, 0, opts, nproj=3)
    on = _run(case, 0, 1, opts, nproj=3)
    _counts(off, on)
    _same(off, on)


def test_default_and_refused_values():
    """A fresh production context with nothing set takes the option (lx1 <= 10; lx1 = 12 keeps today's order unless the option
    is 1) and equals option 0; the value 2 is refused; without the compact blocks (lean_args = 0) the option does nothing."""
    from nekstab_amd.capi import NskError
    from nekstab_amd.settings import production_context
    case = _case(6)
    dflt = _run(case, 0, None)
    assert dflt["stats"]["idxfirst_steps"] > 0 and dflt["stats"]["idxfirst_steps"] == dflt["stats"]["leanargs_steps"]
    off = _run(case, 0, 0)
    _same(dflt, off)
    h = production_context(case)
    try:
        with pytest.raises(NskError) as e:
            h.set_option("idx_first", 2)
        assert e.value.code == -1
    finally:
        h.close()
    nolean = _run(case, 0, 1, [("lean_args", 0)])
    assert nolean["stats"]["idxfirst_steps"] == 0 and nolean["stats"]["leanargs_steps"] == 0
    _same(nolean, off)
    d12 = _run(_case(12), 0, None)
    assert d12["stats"]["idxfirst_steps"] == 0 and d12["stats"]["leanargs_steps"] > 0


def test_ignored_on_shards_and_hexahedra():
    """A two-rank ShardGroup and a 2 x 2 x 2 hexahedral box (both lx1 = 6) keep Dev and today's order whatever the option
    says: no step counted, identical bits for either value."""
    from nekstab_amd import mesh3d
    from nekstab_amd.capi import NekStabHip
    from nekstab_amd.settings import production_context
    from nekstab_amd.sharded import ShardGroup
    case = _case(6)
    res = []
    for first in (0, 1):
        full = production_context(case, nproj=3)
        full.set_option("idx_first", first)
        g = ShardGroup(full, case, 2)
        g.set_option("idx_first", first)
        g.set_nsteps(NSTEPS)
        q, f1 = g.alloc(2)
        g.upload(q, *_seed(case))
        g.scal(q, 1.0 / g.norm(q))
        g.matvec(f1, q, 0)
        res.append((g.download(f1), g.stats()))
        g.close()
        full.close()
    assert res[0][1]["idxfirst_steps"] == 0 and res[1][1]["idxfirst_steps"] == 0
    assert np.abs(res[0][0][0]).max() > 0 and _bits(res[0][0], res[1][0])
    ubf = lambda x, y, z: np.stack([1.0 - 0.3 * y * y + 0.1 * np.sin(x + z), 0.2 * np.cos(x) * y + 0.1 * z, 0.15 * np.sin(y + 0.5 * z)])
    c = mesh3d.box_case_3d(2, 2, 2, 6, lengths=(2.0, 1.0, 0.8), outflow_xmax=True, re=40.0, endtime=0.05, warp=0.06, ub_func=ubf)
    q = [np.sin(1.1 * c.x + 0.3) * np.cos(0.7 * c.y) * c.mask, np.cos(0.5 * c.x) * np.sin(1.3 * c.y + 0.2 * c.z) * c.mask, 0.3 * np.sin(c.y + c.z) * c.mask]
    res = []
    for first in (0, 1):
        h = NekStabHip(c, c.meta["vert"], c.meta["nvert"], tol_helm=1e-11, tol_pres=1e-6, tol_relative=1, nproj=3)
        h.set_option("idx_first", first)
        h.set_nsteps(NSTEPS)
        a, b = h.alloc(2)
        h.upload3(a, q[0], q[1], q[2], np.zeros(h.npres))
        h.matvec(b, a, 0)
        res.append((h.download3(b), h.stats()))
        h.close()
    assert res[0][1]["idxfirst_steps"] == 0 and res[1][1]["idxfirst_steps"] == 0
    assert np.abs(res[0][0][0]).max() > 0 and _bits(res[0][0], res[1][0])
