"""Option "conv_fuse": convection and the velocity right-hand side of a time step in one launch (k_convect_rhs) against the two
launches k_convect + k_rhs.  Both forms call the same bodies, the forcing goes from one half to the other in a register instead
of through memory => the same bits: every comparison here is np.array_equal, option 0 against option 1."""
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


def _run(case, mode, fuse, options=(), nmaps=2, **ctx):
    from nekstab_amd.settings import production_context
    h = production_context(case, **ctx)              # production tolerances (tol_relative = 1)
    if fuse is not None:
        h.set_option("conv_fuse", fuse)
    for k, val in options:
        h.set_option(k, val)
    r = _maps(h, case, mode, nmaps)
    h.close()
    return r


def _bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _same(a, b):
    assert len(a["outs"]) == len(b["outs"])
    for fa, fb in zip(a["outs"], b["outs"]):
        assert _bits(fa, fb)
    for (ha, pa), (hb, pb) in zip(a["iters"], b["iters"]):
        assert np.array_equal(ha, hb) and np.array_equal(pa, pb)            # the same iteration counts, step by step
    assert np.array_equal(a["col"], b["col"]) and a["beta"] == b["beta"]


def _counts(off, on, nmaps=2, nsteps=NSTEPS):
    """the option did what it says in both runs (a redone map counts again)"""
    assert off["stats"]["convfuse_steps"] == 0
    redone = on["stats"]["retries"]
    if redone == 0:
        assert on["stats"]["convfuse_steps"] == nmaps * nsteps
    else:
        assert on["stats"]["convfuse_steps"] >= (nmaps + 1) * nsteps


@pytest.mark.parametrize("lx1", [6, 8, 10])
@pytest.mark.parametrize("mode", [0, 1])
def test_every_instantiation_bit_for_bit(lx1, mode):
    """lx1 = 6, 8, 10: EPB = 7 / 4 / 2 elements per workgroup, 567 / 576 / 450 fine nodes on 256 threads, with (6, 10) and without
    (8) inactive lanes; direct and adjoint."""
    case = _case(lx1, mode)
    off = _run(case, mode, 0)
    on = _run(case, mode, 1)
    print("lx1", lx1, "mode", mode, "fused steps", on["stats"]["convfuse_steps"], "absorb maps", on["stats"]["absorb_maps"])
    _counts(off, on)
    _same(off, on)


@pytest.mark.parametrize("lx1", [6, 8])
@pytest.mark.parametrize("absorb", [0, 1])
def test_with_and_without_the_deferred_projection_update(lx1, absorb):
    """Both instantiations of the fused kernel: with the bookkeeping workgroup (proj_absorb = 1) and without.  nproj = 3: append,
    restart and the flush at the end of a map all occur in 24 steps."""
    case = _case(lx1)
    opts = [("proj_absorb", absorb)]
    off = _run(case, 0, 0, opts, nproj=3)
    on = _run(case, 0, 1, opts, nproj=3)
    assert (on["stats"]["absorb_maps"] >= 2) == bool(absorb) and off["stats"]["absorb_maps"] == on["stats"]["absorb_maps"]
    _counts(off, on)
    _same(off, on)


def _upo_case(endtime):
    from nekstab_amd import mesh
    from nekstab_amd.quadrature import gauss_legendre, gauss_lobatto_legendre, interp_matrix
    z = np.load(os.path.join(GOLDEN, "cylinder_upo.npz"))
    case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6, endtime=endtime)
    case.ub[:] = z["u"]
    J = interp_matrix(gauss_lobatto_legendre(6)[0], gauss_legendre(4)[0])
    return case, (z["u"][0], z["u"][1], J @ z["p"] @ J.T)


@pytest.mark.parametrize("kind", ["stored", "fourier"])
def test_periodic_base_flows_and_the_moved_step_counter(kind):
    """A stored periodic orbit (one set of base-flow constants per step, slot *bstep) and a Fourier orbit (trig row *bstep): the
    fused launch reads the counter in every workgroup, this step's k_pres_rhs advances it.  The orbit's own integration (full
    equations, eager steps) runs with the option too.  Three maps each, the second adjoint: a counter left one off by a map, or
    advanced twice or not at all in a step, moves every later step onto another base flow."""
    from nekstab_amd.settings import production_context
    case, q0 = _upo_case(0.15)
    res = []
    for fuse in (0, 1):
        h = production_context(case, nproj=3)
        h.set_option("conv_fuse", fuse)
        a0, ae = h.alloc(2)
        h.upload(a0, *q0)
        if kind == "stored":
            h.set_orbit(a0, spng_str=1.7, end=ae)
        else:
            h.set_orbit_fourier(a0, 3, spng_str=1.7, end=ae)
        n = h.nsteps
        assert n >= 16
        end = h.download(ae)
        v = h.alloc(4)
        h.upload(v[0], *_seed(case))
        h.scal(v[0], 1.0 / h.norm(v[0]))
        outs, iters = [end], []
        for k, mode in enumerate((0, 1, 0)):
            h.matvec(v[k + 1], v[k], mode)
            outs.append(h.download(v[k + 1]))
            hh, pp = h.step_iters()
            iters.append((hh.copy(), pp.copy()))
        col, beta = h.orth(v[3], v[:3])
        res.append(dict(outs=outs, iters=iters, col=col, beta=beta, stats=h.stats()))
        h.close()
    off, on = res
    print(kind, "orbit steps", n, "fused steps", on["stats"]["convfuse_steps"], "retries", on["stats"]["retries"])
    assert off["stats"]["convfuse_steps"] == 0 and on["stats"]["convfuse_steps"] >= 4 * n      # the integration + three maps
    _same(off, on)


def test_full_equations():
    """adjoint == 2 through the shared convection body: one nonlinear map (the metrics instead of the base-flow constants, the
    DNS sponge), set up as tests/test_newton_gpu.py does."""
    from nekstab_amd import mesh
    from nekstab_amd.capi import NekStabHip
    from nekstab_amd.quadrature import gauss_legendre, gauss_lobatto_legendre, interp_matrix
    case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6, spng_str=0.0)
    J = interp_matrix(gauss_lobatto_legendre(6)[0], gauss_legendre(4)[0])
    q = (case.ub[0] * (1 + 0.05 * np.sin(case.y)), case.ub[1] + 0.02 * np.cos(case.x) * case.mask, J @ case.meta["bf_p"] @ J.T)
    res = []
    for fuse in (0, 1):
        h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], tol_helm=1e-12, tol_pres=1e-8, tol_relative=1,
                       nproj=8, max_helm_iter=150, max_pres_iter=96)
        h.set_option("conv_fuse", fuse)
        vq, vf = h.alloc(2)
        h.upload(vq, *q)
        h.set_baseflow(vq)
        h.set_nsteps(NSTEPS)
        h.nonlinear_map(vf, vq)
        res.append((h.download(vf), h.stats()["convfuse_steps"]))
        h.close()
    assert res[0][1] == 0 and res[1][1] >= NSTEPS
    assert np.abs(res[0][0][0]).max() > 0 and _bits(res[0][0], res[1][0])


@pytest.mark.parametrize("what", ["budgets", "tails", "eager"])
def test_launch_modes(what):
    """lx1 = 8: launch budgets (tail = 0), safety-net tails (tail = 2) and host-checked eager steps (hostcheck = 1, which takes the
    fused kernel too) give the same bits with the option as without it, in the same mode.  Four maps: the per-step budgets exist
    from the second map on."""
    case = _case(8)
    opts = {"budgets": [("tail", 0), ("tail_off_h", 8), ("tail_off_p", 8)], "tails": [("tail", 2)], "eager": [("hostcheck", 1)]}[what]
    off = _run(case, 0, 0, opts, nmaps=4, nproj=3)
    on = _run(case, 0, 1, opts, nmaps=4, nproj=3)
    print(what, "tail maps", on["stats"]["tail_maps"], "retries", on["stats"]["retries"], "fused steps", on["stats"]["convfuse_steps"])
    if what == "tails":
        assert on["stats"]["tail_maps"] >= 2
    if what == "budgets":
        assert on["stats"]["tail_maps"] == 0
    _counts(off, on, nmaps=4)
    _same(off, on)


def test_forced_maps_ignore_it():
    """k_add_force sits between the two kernels: a forced map keeps the two launches whatever the option says."""
    from nekstab_amd.capi import NSK_ADJOINT, NSK_DIRECT
    from nekstab_amd.settings import production_context
    case = _case(6)
    force = np.load(os.path.join(GOLDEN, "cylinder_bf_sensitivity.npz"))["sr_u"].astype(np.float64)
    res = []
    for fuse in (0, 1):
        h = production_context(case, nproj=3)
        h.set_option("conv_fuse", fuse)
        h.set_nsteps(NSTEPS)
        a, b, fv = h.alloc(3)
        h.upload(a, *_seed(case))
        h.scal(a, 1.0 / h.norm(a))
        h.upload(fv, force[0], force[1], np.zeros(h.npres))
        out = []
        for mode in (NSK_DIRECT, NSK_ADJOINT):
            h.forced_map(b, a, fv, mode)
            out.append(h.download(b))
        res.append((out, h.stats()["convfuse_steps"]))
        h.close()
    assert res[0][1] == 0 and res[1][1] == 0
    assert _bits(res[0][0][0], res[1][0][0]) and _bits(res[0][0][1], res[1][0][1])


def test_hexahedra_ignore_it():
    from nekstab_amd import mesh3d
    from nekstab_amd.capi import NekStabHip
    ubf = lambda x, y, z: np.stack([1.0 - 0.3 * y * y + 0.1 * np.sin(x + z), 0.2 * np.cos(x) * y + 0.1 * z, 0.15 * np.sin(y + 0.5 * z)])
    c = mesh3d.box_case_3d(2, 2, 2, 6, lengths=(2.0, 1.0, 0.8), outflow_xmax=True, re=40.0, endtime=0.05, warp=0.06, ub_func=ubf)
    q = [np.sin(1.1 * c.x + 0.3) * np.cos(0.7 * c.y) * c.mask, np.cos(0.5 * c.x) * np.sin(1.3 * c.y + 0.2 * c.z) * c.mask, 0.3 * np.sin(c.y + c.z) * c.mask]
    res = []
    for fuse in (0, 1):
        h = NekStabHip(c, c.meta["vert"], c.meta["nvert"], tol_helm=1e-11, tol_pres=1e-6, tol_relative=1, nproj=3)
        h.set_option("conv_fuse", fuse)
        h.set_nsteps(6)
        a, b = h.alloc(2)
        h.upload3(a, q[0], q[1], q[2], np.zeros(h.npres))
        h.matvec(b, a, 0)
        res.append((h.download3(b), h.stats()["convfuse_steps"]))
        h.close()
    assert res[0][1] == 0 and res[1][1] == 0
    assert np.abs(res[0][0][0]).max() > 0 and _bits(res[0][0], res[1][0])


def test_shards_ignore_it():
    """Two shards of the same case on one device: the sharded step keeps its sequence whatever the option says on the shards and
    on their parent."""
    from nekstab_amd.settings import production_context
    from nekstab_amd.sharded import ShardGroup
    case = _case(6)
    res = []
    for fuse in (0, 1):
        full = production_context(case, nproj=3)
        full.set_option("conv_fuse", fuse)
        g = ShardGroup(full, case, 2)
        g.set_option("conv_fuse", fuse)
        g.set_nsteps(NSTEPS)
        q, f1, f2 = g.alloc(3)
        g.upload(q, *_seed(case))
        g.scal(q, 1.0 / g.norm(q))
        g.matvec(f1, q, 0)
        g.matvec(f2, f1, 0)
        res.append((g.download(f1), g.download(f2), g.stats()))
        g.close()
        full.close()
    assert res[0][2]["convfuse_steps"] == 0 and res[1][2]["convfuse_steps"] == 0
    for k in (0, 1):
        assert _bits(res[0][k], res[1][k])


def test_default_and_refused_values():
    """A fresh production context with nothing set runs fused and equals option 0; values other than -1, 0, 1 are refused."""
    from nekstab_amd.capi import NskError
    from nekstab_amd.settings import production_context
    case = _case(6)
    dflt = _run(case, 0, None)
    assert dflt["stats"]["convfuse_steps"] > 0
    _same(dflt, _run(case, 0, 0))
    h = production_context(case)
    try:
        with pytest.raises(NskError) as e:
            h.set_option("conv_fuse", 2)
        assert e.value.code == -1
    finally:
        h.close()


def test_bench_kernel_name_and_the_map_behind_it():
    """nsk_bench_kernel knows the fused kernel and the two it replaces; the map behind them starts from a reset state and equals
    a fresh context's map."""
    from nekstab_amd.settings import production_context
    case = _case(6)
    ref = _run(case, 0, 1, nmaps=1)
    h = production_context(case)
    h.set_option("conv_fuse", 1)
    first = _maps(h, case, 0, nmaps=1)
    for kn in ("convect_rhs", "convect", "rhs"):
        t = h.bench_kernel(kn, 20)["avg_us"]
        print(kn, t, "us")
        assert t > 0
    again = _maps(h, case, 0, nmaps=1)
    h.close()
    assert _bits(first["outs"][0], ref["outs"][0])
    assert _bits(again["outs"][0][:2], ref["outs"][0][:2])          # reset state = fresh context
