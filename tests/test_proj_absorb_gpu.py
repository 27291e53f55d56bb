"""Option "proj_absorb": the update of the pressure projection space of time step s applied by the first two readers of the
space in step s + 1 (k_pres_rhs: PX, k_proj_apply_e: PEX) instead of a k_proj_update launch per step, against the launch per
step.  Same operations on the same values in the same order => the same bits: every comparison here is np.array_equal."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NSTEPS = 24            # short maps; two consecutive maps per context: the map-end flush and the next map's first step
_CASES = {}


def _case(lx1, adjoint=False):
    """The small cylinder mesh at lx1 = 6 (what the case6 fixture loads) or 8 (the flagship kernel instantiation), direct or adjoint."""
    key = (lx1, bool(adjoint))
    if key not in _CASES:
        from nekstab_amd import mesh
        from tests.conftest import GOLDEN
        _CASES[key] = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), lx1, adjoint=bool(adjoint))
    return _CASES[key]


def _seed(case):
    from nekstab_amd import seed
    qx, qy = seed.add_noise(case)
    m = case.lx1 - 2
    return qx, qy, np.zeros((case.nel, m, m))


def _two_maps(h, case, mode, nmaps=2):
    """nmaps consecutive maps of NSTEPS time steps, f_k = map(f_{k-1}): every output, the per-step iteration counts of every map,
    the Hessenberg column of the last output against the vectors before it (nsk_orth), the statistics."""
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
    col, beta = h.orth(v[nmaps], v[:nmaps])
    st = h.stats()
    return dict(outs=outs, iters=iters, col=col, beta=beta, stats=st)


def _run(case, mode, absorb, options=(), **ctx):
    from nekstab_amd.settings import production_context
    h = production_context(case, **ctx)              # production tolerances (tol_relative = 1)
    h.set_option("proj_absorb", absorb)
    for k, val in options:
        h.set_option(k, val)
    r = _two_maps(h, case, mode)
    h.close()
    return r


def _same(a, b):
    assert len(a["outs"]) == len(b["outs"])
    for fa, fb in zip(a["outs"], b["outs"]):
        assert all(np.array_equal(x, y) for x, y in zip(fa, fb))
    for (ha, pa), (hb, pb) in zip(a["iters"], b["iters"]):
        assert np.array_equal(ha, hb) and np.array_equal(pa, pb)            # the same iteration counts, step by step
    assert np.array_equal(a["col"], b["col"]) and a["beta"] == b["beta"]


@pytest.mark.parametrize("lx1,mode,restart", [(6, 0, 1), (6, 1, 1), (6, 0, 0), (6, 1, 0), (8, 0, 1), (8, 1, 1), (8, 0, 0)])
def test_every_branch_bit_for_bit(lx1, mode, restart):
    """nproj = 3: the space fills after three steps, then restarts on the total solution every third step (proj_restart = 1) or
    merges into the oldest slot every step (proj_restart = 0): append, restart / merge, the flush at the end of a map and the
    first step of the next map (nothing pending), direct and adjoint."""
    case = _case(lx1, mode)
    off = _run(case, mode, 0, [("proj_restart", restart)], nproj=3)
    on = _run(case, mode, 1, [("proj_restart", restart)], nproj=3)
    print("lx1", lx1, "mode", mode, "restart", restart, "pressure iterations per step", off["iters"][1][1], "absorb maps", on["stats"]["absorb_maps"])
    assert off["stats"]["absorb_maps"] == 0 and on["stats"]["absorb_maps"] >= 2      # the option did what it says in both runs (a redone map counts again)
    _same(off, on)


def test_default_is_on_where_the_solve_starts_inside_its_first_launch():
    case = _case(6)
    dflt = _run(case, 0, -1, nproj=3)
    assert dflt["stats"]["absorb_maps"] >= 2
    _same(dflt, _run(case, 0, 0, nproj=3))


def test_no_update_branch():
    """Solves that end with zero GMRES iterations (the projection alone meets a loose tolerance; min_pres_iter = 0) leave
    nothing to absorb: k_vel_update_proj leaves no update pending and the next step's readers find none."""
    case = _case(6)
    opts = [("min_pres_iter", 0)]
    off = _run(case, 0, 0, opts, nproj=3, tol_pres=0.5)
    zeros = sum(int((pp == 0).sum()) for _, pp in off["iters"])
    print("pressure iterations per step, option off:", [pp.tolist() for _, pp in off["iters"]])
    assert zeros >= 1                                   # the branch is taken on this fixture at this setting
    on = _run(case, 0, 1, opts, nproj=3, tol_pres=0.5)
    assert on["stats"]["absorb_maps"] >= 2
    _same(off, on)


def test_tail_modes_agree_with_the_option_on():
    """Persistent tails (tail = 1: median heads; 2: budgets with the tail as a safety net) against launch budgets (0), option on:
    bit for bit the same maps, as tests/test_persistent_gpu.py asks of the launch-per-step update.  Four maps: the per-step
    budgets that the tails need exist from the second map on."""
    from nekstab_amd.settings import production_context
    case = _case(8)
    res = {}
    for tail in (0, 1, 2):
        h = production_context(case, nproj=3)
        h.set_option("proj_absorb", 1)
        h.set_option("tail", tail)
        if tail == 0:
            h.set_option("tail_off_h", 8); h.set_option("tail_off_p", 8)      # the reference run must not overflow a budget (a redone map starts from the space its failed attempt left)
        res[tail] = _two_maps(h, case, 0, nmaps=4)
        h.close()
        print("tail", tail, "tail maps", res[tail]["stats"]["tail_maps"], "retries", res[tail]["stats"]["retries"], "absorb maps", res[tail]["stats"]["absorb_maps"])
        assert res[tail]["stats"]["retries"] == 0 and res[tail]["stats"]["absorb_maps"] == 4
    assert res[0]["stats"]["tail_maps"] == 0 and res[1]["stats"]["tail_maps"] >= 2 and res[2]["stats"]["tail_maps"] >= 2
    _same(res[0], res[1])
    _same(res[0], res[2])


@pytest.mark.parametrize("what", ["fuse2_0", "nproj_0"])
def test_gating_contexts_run_the_launch_per_step(what):
    """Contexts whose pressure solve does not start inside its first launch (fuse2 = 0) or that have no projection space keep the
    k_proj_update launch per step: forcing the option on is ignored, not half-applied."""
    case = _case(6)
    opts = [("fuse2", 0)] if what == "fuse2_0" else []
    nproj = 0 if what == "nproj_0" else 3
    off = _run(case, 0, 0, opts, nproj=nproj)
    on = _run(case, 0, 1, opts, nproj=nproj)
    assert off["stats"]["absorb_maps"] == 0 and on["stats"]["absorb_maps"] == 0
    _same(off, on)


def test_gating_shards_run_the_launch_per_step():
    """Two shards of the same case: the sharded step keeps its sequence whatever the option says on the shards and on their parent."""
    from nekstab_amd.settings import production_context
    from nekstab_amd.sharded import ShardGroup
    case = _case(6)
    res = []
    for absorb in (0, 1):
        full = production_context(case, nproj=3)
        full.set_option("proj_absorb", absorb)
        g = ShardGroup(full, case, 2)
        g.set_option("proj_absorb", absorb)
        g.set_nsteps(NSTEPS)
        q, f1, f2 = g.alloc(3)
        g.upload(q, *_seed(case))
        g.scal(q, 1.0 / g.norm(q))
        g.matvec(f1, q, 0)
        g.matvec(f2, f1, 0)
        res.append((g.download(f1), g.download(f2), g.stats()))
        g.close()
        full.close()
    assert res[0][2]["absorb_maps"] == 0 and res[1][2]["absorb_maps"] == 0
    for k in (0, 1):
        assert all(np.array_equal(x, y) for x, y in zip(res[0][k], res[1][k]))


def test_bench_kernel_names_and_the_map_behind_them():
    """After a factorisation with the option on the timing hook still knows the three kernels; the map behind it starts from a
    reset state and equals a fresh context's map (as tests/test_errors_gpu.py asks of the launch-per-step update)."""
    from nekstab_amd import krylov
    from nekstab_amd.settings import production_context
    case = _case(6)
    qx, qy, zp = _seed(case)
    h0 = production_context(case, nproj=3)
    h0.set_option("proj_absorb", 1)
    h0.set_nsteps(NSTEPS)
    a, f = h0.alloc(2)
    h0.upload(a, qx, qy, zp)
    h0.scal(a, 1.0 / h0.norm(a))
    h0.matvec(f, a, 0)
    ref = h0.download(f)
    h0.close()
    h = production_context(case, nproj=3)
    h.set_option("proj_absorb", 1)
    h.set_nsteps(NSTEPS)
    K = 3
    Q = h.alloc(K + 1)
    h.upload(Q[0], qx, qy, zp)
    h.scal(Q[0], 1.0 / h.norm(Q[0]))
    H = np.zeros((K + 1, K))
    krylov.arnoldi_factorization(h, Q, H, 1, K, 0, stats={})
    assert h.stats()["absorb_maps"] >= K
    for kn in ("proj_update", "pres_rhs", "proj_apply_e"):
        assert h.bench_kernel(kn, 20)["avg_us"] > 0
    f = h.alloc(1)[0]
    h.matvec(f, Q[0], 0)
    got = h.download(f)
    h.close()
    assert all(np.array_equal(x, y) for x, y in zip(got[:2], ref[:2]))          # reset state = fresh context
