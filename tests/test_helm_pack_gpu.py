"""Option "helm_pack": the quadrilateral velocity solve on packed scratch arrays (component-interleaved r, p, s, x and A z, the
partial sums as row pairs: 16-byte accesses in k_helm / k_helm_tail / k_pres_rhs) against the component-major layout.  The
arithmetic and its order are the same => the same bits: every comparison here is np.array_equal, option 0 against option 1."""
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

NSTEPS = 24            # short maps; two consecutive maps per context
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


def _maps(h, case, mode, nmaps=2, nsteps=NSTEPS):
    """nmaps consecutive maps f_k = map(f_{k-1}): every output, the per-step iteration counts of every map, the Hessenberg column
    of the last output against the vectors before it (nsk_orth), the statistics."""
    h.set_nsteps(nsteps)
    v = h.alloc(nmaps + 1)
    h.upload(v[0], *_seed(case))
    h.scal(v[0], 1.0 / h.norm(v[0]))
    outs, iters = [], []
    for k in range(nmaps):
        h.matvec(v[k + 1], v[k], mode)
        outs.append(h.download(v[k + 1]))
        hh, pp = h.step_iters()
        iters.append((hh.copy(), pp.copy()))
    col, beta = h.orth(v[nmaps], v[:nmaps])
    return dict(outs=outs, iters=iters, col=col, beta=beta, stats=h.stats())


def _run(case, mode, pack, options=(), nmaps=2, nsteps=NSTEPS, **ctx):
    from nekstab_amd.settings import production_context
    h = production_context(case, **ctx)              # production tolerances (tol_relative = 1)
    if pack is not None:
        h.set_option("helm_pack", pack)
    for k, val in options:
        h.set_option(k, val)
    r = _maps(h, case, mode, nmaps, nsteps)
    h.close()
    return r


def _bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _same(a, b):
    assert len(a["outs"]) == len(b["outs"])
    for fa, fb in zip(a["outs"], b["outs"]):
        assert np.abs(fa[0]).max() > 0 and _bits(fa, fb)
    for (ha, pa), (hb, pb) in zip(a["iters"], b["iters"]):
        assert np.array_equal(ha, hb) and np.array_equal(pa, pb)            # the same iteration counts, step by step
    assert np.array_equal(a["col"], b["col"]) and a["beta"] == b["beta"]


def _counts(off, on, nmaps=2, nsteps=NSTEPS):
    """the packed form ran with 1 and not with 0 (a redone map counts again)"""
    assert off["stats"]["helmpack_steps"] == 0
    if on["stats"]["retries"] == 0:
        assert on["stats"]["helmpack_steps"] == nmaps * nsteps
    else:
        assert on["stats"]["helmpack_steps"] >= (nmaps + 1) * nsteps


@pytest.mark.parametrize("lx1", [6, 8, 10, 12])
@pytest.mark.parametrize("mode", [0, 1])
def test_every_instantiation_bit_for_bit(lx1, mode):
    """lx1 = 6, 8, 10, 12: EPB = 7 / 4 / 2 / 1 elements per workgroup, 286 / 499 / 998 / 1996 workgroups on 256 / 256 / 256 / 144
    threads: one block of partial sums per thread in part of the threads, two, the loop behind 2 NT blocks, and the totals of
    k_tot2 (row layout of the partial sums kept, vectors packed); direct and adjoint."""
    case = _case(lx1, mode)
    nsteps = 12 if lx1 == 12 else NSTEPS
    off = _run(case, mode, 0, nsteps=nsteps)
    on = _run(case, mode, 1, nsteps=nsteps)
    print("lx1", lx1, "mode", mode, "packed steps", on["stats"]["helmpack_steps"], "helm iterations", on["stats"]["total_helm_iters"])
    _counts(off, on, nsteps=nsteps)
    _same(off, on)


def test_the_tail_on_packed_arrays():
    """lx1 = 8, tail = 1 with the heads pushed far below the iteration counts: k_helm_tail<8, true> runs most iterations of every
    solve from the second map on (the per-step budgets exist from then)."""
    case = _case(8)
    opts = [("tail", 1), ("tail_off_h", -6), ("tail_off_p", -3)]
    off = _run(case, 0, 0, opts, nmaps=4)
    on = _run(case, 0, 1, opts, nmaps=4)
    print("tail maps", on["stats"]["tail_maps"], "heads per step %.2f" % on["stats"]["step_budget_helm_mean"],
          "iterations per step %.2f" % (on["stats"]["total_helm_iters"] / on["stats"]["total_steps"]), "retries", on["stats"]["retries"])
    assert on["stats"]["tail_maps"] >= 2 and off["stats"]["tail_maps"] == on["stats"]["tail_maps"]
    assert on["stats"]["step_budget_helm_mean"] < on["stats"]["total_helm_iters"] / on["stats"]["total_steps"]      # the tails ran iterations
    _counts(off, on, nmaps=4)
    _same(off, on)


@pytest.mark.parametrize("what", ["eager", "hostcheck"])
def test_eager_steps(what):
    """Steps launched one by one (use_graph = 0) and host-checked steps (hostcheck = 1: the host reads the flags between
    launches) take the packed form too."""
    case = _case(8)
    opts = {"eager": [("use_graph", 0)], "hostcheck": [("hostcheck", 1)]}[what]
    off = _run(case, 0, 0, opts, nproj=3)
    on = _run(case, 0, 1, opts, nproj=3)
    _counts(off, on)
    _same(off, on)


@pytest.mark.parametrize("tol", [1e-3, 0.5, 1e3])
def test_finished_and_never_started_solves(tol):
    """Relative tolerances far above production's.  1e-3 and 0.5: solves of a few iterations whose components finish in
    different launches -- the finished component's half of every 16-byte store is the loaded value, the launches behind the end
    take the early exit.  1e3: the residual of the extrapolated guess and the right-hand side are of one order, so every solve is
    finished when launch 1 forms the reference norms from the (b, b) pair, the only launch that loads it: zero iterations."""
    case = _case(8)
    off = _run(case, 0, 0, tol_helm=tol)
    on = _run(case, 0, 1, tol_helm=tol)
    hh = on["iters"][-1][0]
    print("tol_helm", tol, "iterations per step of the last map", hh.tolist(), "retries", on["stats"]["retries"])
    if tol == 1e3:
        assert hh.max() == 0                 # never-started solves
    else:
        assert 0 < hh.max() < 10             # solves of a few iterations
    _counts(off, on)
    _same(off, on)


@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("absorb", [0, 1])
def test_the_four_forms_of_the_pressure_right_hand_side(fuse, absorb):
    """k_pres_rhs<N, AB, PK>: with and without the deferred update of the projection space, launched behind k_convect_rhs
    (it advances the step counter) or behind k_rhs.  nproj = 3: append, restart and flush all occur in 24 steps."""
    case = _case(8)
    opts = [("conv_fuse", fuse), ("proj_absorb", absorb)]
    off = _run(case, 0, 0, opts, nproj=3)
    on = _run(case, 0, 1, opts, nproj=3)
    assert (on["stats"]["absorb_maps"] >= 2) == bool(absorb) and (on["stats"]["convfuse_steps"] > 0) == bool(fuse)
    _counts(off, on)
    _same(off, on)


def test_shards_and_hexahedra_ignore_it():
    """Shards (their halo exchange and totals index rows) and hexahedra keep the component-major layout whatever the option says."""
    from nekstab_amd import mesh3d
    from nekstab_amd.capi import NekStabHip
    from nekstab_amd.settings import production_context
    from nekstab_amd.sharded import ShardGroup
    case = _case(6)
    res = []
    for pack in (0, 1):
        full = production_context(case, nproj=3)
        full.set_option("helm_pack", pack)
        g = ShardGroup(full, case, 2)
        g.set_option("helm_pack", pack)
        g.set_nsteps(NSTEPS)
        q, f1 = g.alloc(2)
        g.upload(q, *_seed(case))
        g.scal(q, 1.0 / g.norm(q))
        g.matvec(f1, q, 0)
        res.append((g.download(f1), g.stats()))
        g.close()
        full.close()
    assert res[0][1]["helmpack_steps"] == 0 and res[1][1]["helmpack_steps"] == 0
    assert _bits(res[0][0], res[1][0])
    ubf = lambda x, y, z: np.stack([1.0 - 0.3 * y * y + 0.1 * np.sin(x + z), 0.2 * np.cos(x) * y + 0.1 * z, 0.15 * np.sin(y + 0.5 * z)])
    c = mesh3d.box_case_3d(2, 2, 2, 6, lengths=(2.0, 1.0, 0.8), outflow_xmax=True, re=40.0, endtime=0.05, warp=0.06, ub_func=ubf)
    q = [np.sin(1.1 * c.x + 0.3) * np.cos(0.7 * c.y) * c.mask, np.cos(0.5 * c.x) * np.sin(1.3 * c.y + 0.2 * c.z) * c.mask, 0.3 * np.sin(c.y + c.z) * c.mask]
    res = []
    for pack in (0, 1):
        h = NekStabHip(c, c.meta["vert"], c.meta["nvert"], tol_helm=1e-11, tol_pres=1e-6, tol_relative=1, nproj=3)
        h.set_option("helm_pack", pack)
        h.set_nsteps(6)
        a, b = h.alloc(2)
        h.upload3(a, q[0], q[1], q[2], np.zeros(h.npres))
        h.matvec(b, a, 0)
        res.append((h.download3(b), h.stats()["helmpack_steps"]))
        h.close()
    assert res[0][1] == 0 and res[1][1] == 0
    assert np.abs(res[0][0][0]).max() > 0 and _bits(res[0][0], res[1][0])


def test_lx1_12_takes_it_only_when_asked():
    """k_helm<12, true> needs more registers than k_helm<12> (one wavefront per SIMD fewer): the default leaves lx1 = 12 on the
    component-major layout, option 1 packs it (test_every_instantiation_bit_for_bit)."""
    case = _case(12)
    dflt = _run(case, 0, None, nmaps=1, nsteps=4)
    assert dflt["stats"]["helmpack_steps"] == 0
    _same(dflt, _run(case, 0, 1, nmaps=1, nsteps=4))


def test_default_refused_values_and_the_bench_kernel():
    """A fresh production context with nothing set runs packed and equals option 0; values other than -1, 0, 1 are refused;
    nsk_bench_kernel("helm") times the instantiation the context runs and the map behind it equals a fresh context's."""
    from nekstab_amd.capi import NskError
    from nekstab_amd.settings import production_context
    case = _case(6)
    dflt = _run(case, 0, None, nmaps=1)
    assert dflt["stats"]["helmpack_steps"] > 0
    _same(dflt, _run(case, 0, 0, nmaps=1))
    h = production_context(case)
    try:
        with pytest.raises(NskError) as e:
            h.set_option("helm_pack", 2)
        assert e.value.code == -1
        for pack in (0, 1):
            h.set_option("helm_pack", pack)
            t = h.bench_kernel("helm", 20)["avg_us"]
            print("helm_pack", pack, "k_helm", t, "us")
            assert t > 0
        _same(dflt, _maps(h, case, 0, nmaps=1))
    finally:
        h.close()
