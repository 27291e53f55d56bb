"""Option "lean_args": the iteration kernels of the quadrilateral step (k_helm, k_schwarz_uc, k_divgs_t) on compact argument
blocks -- the head as leading, preloaded kernel parameters, the rest in one batch of argument loads -- against the same bodies on
Dev by value.  Only where the arguments come from changes, no operation and no order: every comparison here is np.array_equal,
option 1 against option 0 in one build, on the cylinder fixture: the state after a map of 6 time steps (step classes 1, 2, 3 and
4-6: launches it = 0 / 1 / >= 2 and all three BDF orders of the Jacobi diagonal) and the per-step iteration counts."""
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


def _run(case, mode, lean, options=(), nmaps=1, **ctx):
    from nekstab_amd.settings import production_context
    h = production_context(case, **ctx)
    try:
        if lean is not None:
            h.set_option("lean_args", lean)
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
    """the compact blocks ran with 1 and not with 0 (a redone map counts again)"""
    assert off["stats"]["leanargs_steps"] == 0
    if on["stats"]["retries"] == 0:
        assert on["stats"]["leanargs_steps"] == nmaps * NSTEPS
    else:
        assert on["stats"]["leanargs_steps"] >= (nmaps + 1) * NSTEPS


@pytest.mark.parametrize("lx1", [6, 8, 10, 12])
@pytest.mark.parametrize("mode", [0, 1])
def test_every_instantiation_bit_for_bit(lx1, mode):
    """lx1 = 6, 8, 10: k_helm_l<N, true> (packed), 12: the component-major k_helm_l<12, false>; k_schwarz_uc_l / k_divgs_t_l of
    every lx1; direct and adjoint.  lx1 = 8 runs the instantiations of the benchmark."""
    case = _case(lx1, mode)
    off = _run(case, mode, 0)
    on = _run(case, mode, 1)
    print("lx1", lx1, "mode", mode, "lean steps", on["stats"]["leanargs_steps"], "iterations", on["iters"][0][0][:NSTEPS].tolist(), on["iters"][0][1][:NSTEPS].tolist())
    _counts(off, on)
    assert (on["stats"]["helmpack_steps"] > 0) == (lx1 <= 10)
    _same(off, on)


def test_component_masks():
    """nsk_init_masks, lx1 = 6: k_helm_l<6, true, true> and k_divgs_t_l<6, false, true>.  The second component gets a Dirichlet
    condition of its own on the nodes of the lowest grid line, so that the two masks differ (equal masks take the shared-mask
    instantiations)."""
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


def test_tails_share_the_bodies():
    """lx1 = 8, four maps, tail = 1 with the heads pushed far below the iteration counts (as tests/test_persistent_gpu.py): from the second
    map on (the per-step budgets exist from then) k_helm_tail and k_pres_tail2 -- on Dev -- run most iterations behind heads
    on the compact blocks, the same body text in both."""
    case = _case(8)
    # (heads = the previous map's counts + offset; the counts of these short maps still fall by ~9 from the first map to the
    #  second, so the velocity offset is larger than the -6 of the longer maps there)
    opts = [("tail", 1), ("tail_off_h", -16), ("tail_off_p", -3)]
    off = _run(case, 0, 0, opts, nmaps=4)
    on = _run(case, 0, 1, opts, nmaps=4)
    print("tail maps", on["stats"]["tail_maps"], "heads per step %.2f / %.2f" % (on["stats"]["step_budget_helm_mean"], on["stats"]["step_budget_pres_mean"]),
          "iterations per step %.2f" % (on["stats"]["total_helm_iters"] / on["stats"]["total_steps"]), "retries", on["stats"]["retries"])
    assert on["stats"]["tail_maps"] >= 1 and off["stats"]["tail_maps"] == on["stats"]["tail_maps"]
    # the tails ran iterations: the heads (a mean over the maps that had per-step budgets, the second to the fourth) stay below
    # the iteration counts of those maps
    later_h = np.mean([hh[:NSTEPS].mean() for hh, _ in on["iters"][1:]]), np.mean([pp[:NSTEPS].mean() for _, pp in on["iters"][1:]])
    print("iterations per step of maps 2 to 4: %.2f / %.2f" % later_h)
    assert on["stats"]["step_budget_helm_mean"] < later_h[0]
    _counts(off, on, nmaps=4)
    _same(off, on)


def test_deferred_projection_update_across_a_restart():
    """nproj = 3: the projection space fills and restarts within the 6 steps of a map, its update deferred into the next step's
    readers (proj_absorb); A_0 starts every solve (uc_start) on the block k_proj_apply_e left."""
    case = _case(8)
    off = _run(case, 0, 0, nmaps=2, nproj=3)
    on = _run(case, 0, 1, nmaps=2, nproj=3)
    assert on["stats"]["absorb_maps"] >= 2 and off["stats"]["absorb_maps"] == on["stats"]["absorb_maps"]
    _counts(off, on, nmaps=2)
    _same(off, on)


@pytest.mark.parametrize("what", ["eager", "hostcheck"])
def test_eager_steps(what):
    """Steps launched one by one (use_graph = 0) and host-checked steps take the compact blocks too."""
    case = _case(8)
    opts = {"eager": [("use_graph", 0)], "hostcheck": [("hostcheck", 1)]}[what]
    off = _run(case, 0, 0, opts, nproj=3)
    on = _run(case, 0, 1, opts, nproj=3)
    _counts(off, on)
    _same(off, on)


def test_default_and_refused_values():
    """A fresh production context with nothing set takes the compact blocks and equals option 0; values other than -1, 0, 1
    are refused."""
    from nekstab_amd.capi import NskError
    from nekstab_amd.settings import production_context
    case = _case(6)
    dflt = _run(case, 0, None)
    assert dflt["stats"]["leanargs_steps"] > 0 and dflt["stats"]["helmpack_steps"] > 0 and dflt["stats"]["convfuse_steps"] > 0
    _same(dflt, _run(case, 0, 0))
    h = production_context(case)
    try:
        with pytest.raises(NskError) as e:
            h.set_option("lean_args", 2)
        assert e.value.code == -1
    finally:
        h.close()


def test_ignored_where_helm_pack_is():
    """Shards, hexahedra and the persistent velocity solve (k_helm_fused) keep Dev whatever the option says -- exactly where
    helm_pack is ignored."""
    from nekstab_amd import mesh3d
    from nekstab_amd.capi import NekStabHip
    from nekstab_amd.settings import production_context
    from nekstab_amd.sharded import ShardGroup
    case = _case(6)
    res = []
    for lean in (0, 1):
        full = production_context(case, nproj=3)
        full.set_option("lean_args", lean)
        g = ShardGroup(full, case, 2)
        g.set_option("lean_args", lean)
        g.set_nsteps(NSTEPS)
        q, f1 = g.alloc(2)
        g.upload(q, *_seed(case))
        g.scal(q, 1.0 / g.norm(q))
        g.matvec(f1, q, 0)
        res.append((g.download(f1), g.stats()))
        g.close()
        full.close()
    assert res[0][1]["leanargs_steps"] == 0 and res[1][1]["leanargs_steps"] == 0 and res[1][1]["helmpack_steps"] == 0
    assert _bits(res[0][0], res[1][0])
    fused = [_run(case, 0, lean, fused=1) for lean in (0, 1)]
    assert fused[0]["stats"]["leanargs_steps"] == 0 and fused[1]["stats"]["leanargs_steps"] == 0 and fused[1]["stats"]["helmpack_steps"] == 0
    assert _bits(fused[0]["outs"][0], fused[1]["outs"][0])
    ubf = lambda x, y, z: np.stack([1.0 - 0.3 * y * y + 0.1 * np.sin(x + z), 0.2 * np.cos(x) * y + 0.1 * z, 0.15 * np.sin(y + 0.5 * z)])
    c = mesh3d.box_case_3d(2, 2, 2, 6, lengths=(2.0, 1.0, 0.8), outflow_xmax=True, re=40.0, endtime=0.05, warp=0.06, ub_func=ubf)
    q = [np.sin(1.1 * c.x + 0.3) * np.cos(0.7 * c.y) * c.mask, np.cos(0.5 * c.x) * np.sin(1.3 * c.y + 0.2 * c.z) * c.mask, 0.3 * np.sin(c.y + c.z) * c.mask]
    res = []
    for lean in (0, 1):
        h = NekStabHip(c, c.meta["vert"], c.meta["nvert"], tol_helm=1e-11, tol_pres=1e-6, tol_relative=1, nproj=3)
        h.set_option("lean_args", lean)
        h.set_nsteps(NSTEPS)
        a, b = h.alloc(2)
        h.upload3(a, q[0], q[1], q[2], np.zeros(h.npres))
        h.matvec(b, a, 0)
        res.append((h.download3(b), h.stats()))
        h.close()
    assert res[0][1]["leanargs_steps"] == 0 and res[1][1]["leanargs_steps"] == 0 and res[1][1]["helmpack_steps"] == 0
    assert np.abs(res[0][0][0]).max() > 0 and _bits(res[0][0], res[1][0])
