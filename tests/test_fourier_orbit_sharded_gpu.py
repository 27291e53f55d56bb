"""Fourier-compressed periodic base flows on element shards (nsk_group_set_orbit_fourier, nsk_group_set_orbit_modes,
nsk_group_get_orbit_modes; ShardGroup / ShardRank .set_orbit_fourier, .set_orbit_modes, .get_orbit_modes): every rank keeps the
modes of its own elements and the sharded step rebuilds the base-flow constants per rank (k_baseflow_fourier in group_step).
Held against the single-rank Fourier orbit and against the stored orbit on shards, with the bounds those comparisons already
have in tests/test_sharded_r3_gpu.py and tests/test_fourier_orbit_gpu.py: per element the reconstruction adds the same numbers
in the same order on a shard as on the full mesh, so a sharded Fourier map differs from the single-rank one only through the
rounding of halo sums and all-reduces and the solver tolerance -- what makes a sharded stored-orbit map differ.

The runs that several tests look at are done once per module (`shedding`: the integrations from the shedding state;
`loaded`: the single-rank maps over the synthetic modes) and left unchanged by the tests."""
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN
from tests.test_fourier_orbit_gpu import PERIOD, _synthetic_modes, _upload_modes2

pytestmark = pytest.mark.gpu

# the setting of test_time_periodic_base_flow_on_shards
KW1 = dict(tol_helm=1e-12, tol_pres=1e-6, tol_relative=1, nproj=8, max_helm_iter=150, max_pres_iter=48)
ENDTIME = 0.15


def _rel(w, got, ref, ncomp=2):
    num = np.sqrt(sum(np.sum(w * (a - b) ** 2) for a, b in zip(got[:ncomp], ref[:ncomp])))
    den = np.sqrt(sum(np.sum(w * b ** 2) for b in ref[:ncomp]))
    return num / den


def _max3(got, ref):
    """the max-norm measure of test_time_periodic_base_flow_on_hexahedral_shards"""
    sc = max(np.abs(ref[k]).max() for k in range(3))
    return max(np.abs(got[k] - ref[k]).max() for k in range(3)) / sc


def _bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _dev_rel(g, a, b):
    """|a - b| / |b| in the device's inner product; a is overwritten"""
    g.axpy(a, -1.0, b)
    return g.norm(a) / g.norm(b)


# ---------------------------------------------------------------------------------------------------------------------------
# 1, 2, the transitions of 7 and the single-rank side of 8: integrations from the shedding state, done once
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shedding():
    from nekstab_amd import mesh, seed
    from nekstab_amd.capi import NekStabHip, NskError
    from nekstab_amd.quadrature import gauss_legendre, gauss_lobatto_legendre, interp_matrix
    from nekstab_amd.sharded import ShardGroup
    z = np.load(os.path.join(GOLDEN, "cylinder_upo.npz"))
    case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6, endtime=ENDTIME)
    case.ub[:] = z["u"]
    J = interp_matrix(gauss_lobatto_legendre(6)[0], gauss_legendre(4)[0])
    q0 = (z["u"][0], z["u"][1], J @ z["p"] @ J.T)
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **KW1)
    R = {"case": case, "h": h, "q0": q0, "w": np.ones_like(case.x)}
    groups = []
    try:
        # ---- single rank, every harmonic
        a0, ae, vq, vf = h.alloc(4)
        h.upload(a0, *q0)
        qx, qy = seed.add_noise(case)
        h.upload(vq, qx, qy, np.zeros(h.npres)); h.scal(vq, 1.0 / h.norm(vq))
        R["seed"] = sd = h.download(vq)
        h.set_baseflow(a0)                                                        # nsteps of the orbit, before M is chosen
        n = R["n"] = h.nsteps
        M = R["M"] = n // 2
        R["amp_h"] = h.set_orbit_fourier(a0, M, spng_str=1.7, end=ae)
        R["dt_h"] = h.dt
        R["end_h"] = h.download(ae)
        R["map_h"] = []
        for mode in (0, 1):
            h.matvec(vf, vq, mode); R["map_h"].append(h.download(vf))
        # ---- two shards, the Fourier form
        g = ShardGroup(h, case, 2); groups.append(g)                              # (cut from a parent that holds a Fourier orbit: starts steady)
        R["g"] = g
        b0, be, sq, sf, st = g.alloc(5)
        g.upload(b0, *q0); g.upload(sq, *sd)
        try:
            g.get_orbit_modes(); R["fresh_shard_get"] = "no error"
        except NskError as e:
            R["fresh_shard_get"] = (e.code, str(e))
        try:
            g.set_orbit_fourier(b0, M + 1, spng_str=1.7); R["refusal"] = "no error"
        except NskError as e:
            R["refusal"] = (e.code, str(e))
        R["amp_g"] = g.set_orbit_fourier(b0, M, spng_str=1.7, end=be)
        R["n_g"], R["dt_g"] = g.nsteps, g.dt
        R["end_g"] = g.download(be)
        # asked for twice: of a second group in the state the first was in (same bits expected: integration and reduction add in a
        # fixed order), and of the same group again (its pressure projection space now holds the first integration's solutions --
        # kept from map to map by design -- so the second integration is another one within the solver tolerance)
        t = ShardGroup(h, case, 2); groups.append(t)
        t0 = t.alloc(1)[0]
        t.upload(t0, *q0)
        R["amp_t"] = t.set_orbit_fourier(t0, M, spng_str=1.7)
        R["amp_g2"] = g.set_orbit_fourier(b0, M, spng_str=1.7, end=be)
        R["get_g"] = g.get_orbit_modes()
        R["map_g"] = []
        for mode in (0, 1):
            g.matvec(sf, sq, mode); R["map_g"].append(g.download(sf))
        A, B = g.alloc(M + 1), g.alloc(M)
        R["get_g_AB"] = g.get_orbit_modes(A, B)
        R["norms_g"] = np.array([g.norm(A[0])] + [x for k in range(1, M + 1) for x in (g.norm(A[k]), g.norm(B[k - 1]))])
        g.free(A + B)
        g.set_nsteps(n + 5)
        g.matvec(st, sq, 0)
        R["long_g"] = g.download(st)
        g.set_nsteps(n)
        # ---- two shards, the stored form, on the same parent
        s = ShardGroup(h, case, 2); groups.append(s)
        c0, ce, tq, tf = s.alloc(4)
        s.upload(c0, *q0); s.upload(tq, *sd)
        s.set_orbit(c0, spng_str=1.7, end=ce)
        R["n_s"] = s.nsteps
        R["end_s"] = s.download(ce)
        R["stored_vs_fourier"] = []
        for mode in (0, 1):
            s.matvec(tf, tq, mode)
            g.upload(st, *s.download(tf)); g.upload(sf, *R["map_g"][mode])
            R["stored_vs_fourier"].append(_dev_rel(g, sf, st))
        s.set_nsteps(n + 5)
        try:
            s.matvec(tf, tq, 0); R["long_s"] = "no error"
        except NskError as e:
            R["long_s"] = (e.code, str(e))
        s.set_nsteps(n)
        # ---- transitions: Fourier after stored (s), stored after Fourier (g)
        s.set_orbit_fourier(c0, 2, spng_str=1.7)
        R["s_get_after_fourier"] = s.get_orbit_modes()
        s.matvec(tf, tq, 0)
        R["s_map_after_fourier"] = s.download(tf)
        g.set_orbit(b0, spng_str=1.7)
        try:
            g.get_orbit_modes(); R["g_get_after_stored"] = "no error"
        except NskError as e:
            R["g_get_after_stored"] = (e.code, str(e))
        g.matvec(sf, sq, 0)
        R["g_map_after_stored"] = g.download(sf)
        # ---- single rank, M = 2 (the yardstick of the one-rank communicator)
        R["amp_h2"] = h.set_orbit_fourier(a0, 2, spng_str=1.7)
        h.matvec(vf, vq, 0)
        R["map_h2"] = h.download(vf)
        yield R
    finally:
        for x in groups:
            x.close()
        h.close()


def test_integration_on_quadrilateral_shards(shedding):
    """1: g.set_orbit_fourier against h.set_orbit_fourier at M = nsteps // 2 from the shedding state, 2 shards."""
    R = shedding
    n, M = R["n"], R["M"]
    assert n >= 16, n
    assert R["fresh_shard_get"][0] == -1 and "no Fourier orbit" in R["fresh_shard_get"][1], R["fresh_shard_get"]
    assert R["refusal"][0] == -1 and "nmodes" in R["refusal"][1], R["refusal"]
    assert R["n_g"] == n and abs(R["dt_g"] - R["dt_h"]) < 1e-15
    r = _rel(R["w"], R["end_g"], R["end_h"])
    print("orbit end state, 2 shards vs single rank: rel diff", r)
    assert r < 1e-9
    for mode in (0, 1):
        r = _rel(R["w"], R["map_g"][mode], R["map_h"][mode])
        print("mode", mode, "map over the Fourier orbit, 2 shards vs single rank: rel diff", r)
        assert r < 1e-8
    assert R["get_g"] == (M, ENDTIME) and R["get_g_AB"] == (M, ENDTIME)


def test_fourier_equals_stored_orbit_on_shards(shedding):
    """1: the same integration (k_orbit_dft only reads the field), and maps that differ by the rounding of the reconstruction."""
    R = shedding
    assert R["n_s"] == R["n"]
    assert _bits(R["end_s"], R["end_g"])
    print("Fourier (full spectrum) vs stored orbit on 2 shards, direct / adjoint: relL2", R["stored_vs_fourier"])
    for e in R["stored_vs_fourier"]:
        assert e < 1e-9
    assert all(np.all(np.isfinite(x)) for x in R["long_g"]) and np.abs(R["long_g"][0]).max() > 0
    assert R["long_s"] != "no error" and "longer than the stored" in R["long_s"][1], R["long_s"]


def test_amplitudes(shedding):
    """2: amp[m] from the device reduction over the ranks against g.norm of the mode vectors (both fixed-order sums of the same
    1.4e5 non-negative terms: n eps = 1.6e-11 at worst), against the single rank's (integrations 1e-9 apart), and twice: a second
    fresh group returns the same bits; the same group asked again re-integrates with the projection space the first integration
    left (by design), so its amplitudes are those of another integration -- held to the bound of the line above."""
    R = shedding
    amp, nrm, ah = R["amp_g"], R["norms_g"], R["amp_h"]
    assert amp.shape == (2 * R["M"] + 1,) and np.all(np.isfinite(amp)) and amp[0] > 0
    d = np.abs(amp - nrm)
    print("amp vs norm of the mode vectors: worst relative", (d / np.maximum(nrm, 1e-300)).max(), "worst absolute / amp[0]", d.max() / amp[0])
    assert np.all((d <= 1e-10 * nrm) | (d <= 1e-10 * amp[0]))
    print("sharded vs single-rank amp: worst / amp[0]", np.abs(amp - ah).max() / ah[0])
    assert np.abs(amp - ah).max() <= 1e-8 * ah[0]
    assert np.array_equal(amp, R["amp_t"])
    print("the same group asked again: worst / amp[0]", np.abs(amp - R["amp_g2"]).max() / amp[0])
    assert np.abs(amp - R["amp_g2"]).max() <= 1e-8 * amp[0]             # (and not doubled: the mode arrays were zeroed again)


def test_transitions_between_stored_and_fourier(shedding):
    """7, second half: set_orbit_fourier after set_orbit and set_orbit after set_orbit_fourier both give working maps."""
    R = shedding
    assert R["s_get_after_fourier"] == (2, ENDTIME)
    assert R["g_get_after_stored"][0] == -1 and "no Fourier orbit" in R["g_get_after_stored"][1]
    for a in (R["g_map_after_stored"], R["s_map_after_fourier"]):
        assert all(np.all(np.isfinite(x)) for x in a) and np.abs(a[0]).max() > 0
    print("stored orbit after a Fourier one vs the full-spectrum Fourier map: rel diff", _rel(R["w"], R["g_map_after_stored"], R["map_g"][0]))
    # the M = 2 orbit that replaced the stored one is the single rank's M = 2 orbit: the sharded-vs-single-rank bound of the map
    r2 = _rel(R["w"], R["s_map_after_fourier"], R["map_h2"])
    print("M = 2 Fourier orbit after a stored one vs single rank at M = 2: rel diff", r2)
    assert r2 < 1e-8


def test_one_rank_rccl_communicator(shedding):
    """8: ShardRank with n = 1 and a communicator: the amplitude sum goes through nsk_allreduce_host."""
    from nekstab_amd.sharded import ShardRank
    R = shedding
    h, case = R["h"], R["case"]
    uid = ShardRank.new_unique_id(h.lib)
    s = ShardRank(h, case, 0, 1, uid)
    try:
        b0, sq, sf = s.alloc(3)
        s.upload(b0, *R["q0"]); s.upload(sq, *R["seed"])
        amp = s.set_orbit_fourier(b0, 2, spng_str=1.7)
        assert s.nsteps == R["n"] and s.get_orbit_modes() == (2, ENDTIME)
        print("one-rank communicator vs single-rank amp: worst / amp[0]", np.abs(amp - R["amp_h2"]).max() / R["amp_h2"][0])
        assert amp.shape == (5,) and np.abs(amp - R["amp_h2"]).max() <= 1e-8 * R["amp_h2"][0]
        s.matvec(sf, sq, 0)
        got = s.download_local(sf)
        r = _rel(np.ones_like(got[0]), got, [x[s.elems] for x in R["map_h2"]])
        print("direct map, one-rank communicator vs single rank: rel diff", r)
        assert r < 1e-8
        s.free([b0, sq, sf])
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 3, 6, 7, 9: modes loaded with set_orbit_modes; the single-rank maps are computed once
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loaded(case6, oracle6_nosolve, modes):
    from nekstab_amd.capi import NekStabHip
    from tests.test_matvec_gpu import _mode
    A, B = _synthetic_modes(case6.ub, case6.x)
    q = _mode(oracle6_nosolve, modes, "dRe")
    h = NekStabHip(case6, case6.meta["vert"], case6.meta["nvert"], **KW1)
    try:
        va, vb = _upload_modes2(h, A, B)
        h.set_orbit_modes(va, vb, PERIOD)
        R = {"h": h, "A": A, "B": B, "q": q, "dt": h.dt, "nsteps": h.nsteps, "bm1": oracle6_nosolve.bm1, "ref": {}}
        vq, vf = h.alloc(2)
        h.upload(vq, *q)
        h.set_nsteps(6)
        for phase in (0.0, 0.37):
            h.set_option("orbit_phase", phase)
            for mode in (0, 1):
                h.matvec(vf, vq, mode)
                R["ref"][(phase, mode)] = h.download(vf)
        yield R
    finally:
        h.close()


@pytest.mark.parametrize("nranks", [2, 3])
def test_modes_loaded_and_phase(case6, loaded, nranks):
    """3: modes that vary in space (a rank that reads another element's modes fails), phase 0 and 0.37, six steps."""
    from nekstab_amd.sharded import ShardGroup
    L = loaded
    g = ShardGroup(L["h"], case6, nranks)
    try:
        va, vb = _upload_modes2(g, L["A"], L["B"])
        g.set_orbit_modes(va, vb, PERIOD)
        assert g.get_orbit_modes() == (2, PERIOD)
        assert g.nsteps == L["nsteps"] and abs(g.dt - L["dt"]) < 1e-15, (g.nsteps, g.dt, L["nsteps"], L["dt"])
        g.set_nsteps(6)
        sq, sf = g.alloc(2)
        g.upload(sq, *L["q"])
        for phase in (0.0, 0.37):
            g.set_option("orbit_phase", phase)
            for mode in (0, 1):
                g.matvec(sf, sq, mode)
                r = _rel(L["bm1"], g.download(sf), L["ref"][(phase, mode)])
                print("nranks", nranks, "phase", phase, "mode", mode, "sharded vs single rank over the loaded modes: rel diff", r)
                assert r < 1e-8
        assert not _bits(L["ref"][(0.0, 0)], L["ref"][(0.37, 0)])
        g.free(va + vb + [sq, sf])
    finally:
        g.close()


def test_shards_of_rank_local_parents(case6, loaded):
    """6: shards cut from nsk_init_local parents against the full-mesh single rank."""
    from nekstab_amd.sharded import ShardGroup, local_parents, partition_rcb
    L = loaded
    part = partition_rcb(case6, 2)
    P = []
    g = None
    try:
        P, _ = local_parents(case6, 2, part, **KW1)
        g = ShardGroup(P, case6, 2, part)
        va, vb = _upload_modes2(g, L["A"], L["B"])
        g.set_orbit_modes(va, vb, PERIOD)
        assert g.nsteps == L["nsteps"] and abs(g.dt - L["dt"]) < 1e-15
        g.set_nsteps(6)
        g.set_option("orbit_phase", 0.37)
        sq, sf = g.alloc(2)
        g.upload(sq, *L["q"])
        g.matvec(sf, sq, 0)
        r = _rel(L["bm1"], g.download(sf), L["ref"][(0.37, 0)])
        print("shards of rank-local parents vs single rank: rel diff", r)
        assert r < 1e-8
    finally:
        if g is not None:
            g.close()
        for p in P:
            p.close()


def test_the_way_back(case6, hip6, loaded):
    """7, first half: set_baseflow ends the Fourier orbit; the group then maps as a fresh one, bit for bit.  On the context of
    test_refusals_and_the_way_back (the fixture hip6, no pressure projection space), where that claim is made for the single
    rank: with a projection space the solutions of the maps over the orbit stay in it, by design, and the next map is another
    one within the solver tolerance (measured with the settings of test 1: pressure differs at 1e-8 relative)."""
    from nekstab_amd.capi import NskError
    from nekstab_amd.sharded import ShardGroup
    L = loaded
    g = ShardGroup(hip6, case6, 2)
    f = ShardGroup(hip6, case6, 2)
    try:
        va, vb = _upload_modes2(g, L["A"], L["B"])
        g.set_orbit_modes(va, vb, PERIOD)
        sq, sf = g.alloc(2); fq, ff, fa = f.alloc(3)
        g.upload(sq, *L["q"]); f.upload(fq, *L["q"])
        f.upload(fa, L["A"][0][0], L["A"][0][1], np.zeros(f.npres))
        g.set_nsteps(3)
        g.matvec(sf, sq, 0)
        g.set_nsteps(5)
        g.matvec(sf, sq, 0)
        fourier_map = g.download(sf)
        g.set_baseflow(va[0]); f.set_baseflow(fa)                 # A_0 = the case's base flow
        with pytest.raises(NskError) as e:
            g.get_orbit_modes()
        assert e.value.code == -1 and "no Fourier orbit" in str(e.value)
        g.set_nsteps(5); f.set_nsteps(5)
        g.matvec(sf, sq, 0); f.matvec(ff, fq, 0)
        assert _bits(g.download(sf), f.download(ff))
        assert not _bits(fourier_map, f.download(ff))
    finally:
        g.close(); f.close()


def test_mode_files_on_shards(case6, loaded, tmp_path):
    """9: fourier.write_modes / read_modes with a ShardGroup as the context."""
    from nekstab_amd import fourier
    from nekstab_amd.sharded import ShardGroup
    L = loaded
    g = ShardGroup(L["h"], case6, 2)
    g2 = ShardGroup(L["h"], case6, 2)
    try:
        va, vb = _upload_modes2(g, L["A"], L["B"])
        g.set_orbit_modes(va, vb, PERIOD)
        files = fourier.write_modes(g, str(tmp_path))
        assert len(files) == 6
        M, period, amp = fourier.read_modes(g2, str(tmp_path))
        assert (M, period) == (2, PERIOD) and g2.get_orbit_modes() == g.get_orbit_modes() == (2, PERIOD)
        assert amp.shape == (5,) and amp[0] > 0
        A1, B1 = g.alloc(3), g.alloc(2)
        A2, B2 = g2.alloc(3), g2.alloc(2)
        g.get_orbit_modes(A1, B1); g2.get_orbit_modes(A2, B2)
        for x, y in zip(A1 + B1, A2 + B2):
            assert _bits(g.download(x), g2.download(y))
        assert np.array_equal(g.download(A1[1])[0], L["A"][1][0])   # and they are the modes that went in
    finally:
        g.close(); g2.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4, 5: hexahedra and the launch forms
# ---------------------------------------------------------------------------------------------------------------------------
def _box(lx1):
    """the 24-element box of test_host_checked_convergence_equals_budgeted_launches, its perturbation and settings"""
    from nekstab_amd import mesh3d
    ubf = lambda x, y, z: np.stack([1.0 - 0.3 * y * y + 0.1 * np.sin(x + z), 0.2 * np.cos(x) * y + 0.1 * z, 0.15 * np.sin(y + 0.5 * z)])
    case = mesh3d.box_case_3d(4, 3, 2, lx1, lengths=(2.0, 1.0, 0.8), outflow_xmax=True, re=40.0, endtime=0.05, ub_func=ubf, warp=0.05)
    x, y, z = case.x, case.y, case.z
    m = lx1 - 2
    q = (np.sin(1.3 * x + z) * np.cos(2.0 * y) * case.mask, np.cos(0.7 * x + 0.2) * np.sin(3.0 * y - z) * case.mask,
         np.sin(x + y) * np.cos(2.0 * z) * case.mask, np.zeros((case.nel, m, m, m)))
    kw = dict(tol_helm=1e-12, tol_pres=1e-7, tol_relative=1, max_helm_iter=200, max_pres_iter=48)
    return case, q, kw


def _box_modes(case):
    """three-component M = 2 modes: case.ub times the functions of x of _synthetic_modes"""
    ub, x = case.ub, case.x
    w = np.stack([ub[2], 0.3 * ub[2] * np.cos(0.1 * x), 0.2 * ub[2] * np.sin(0.07 * x), 0.1 * ub[2] * np.exp(-(x / 10.0) ** 2), np.zeros_like(x)])
    return _synthetic_modes(ub[:2], x, w)


def _upload_modes3(h, A, B):
    va, vb = h.alloc(len(A)), h.alloc(len(B))
    for v, m in zip(va + vb, list(A) + list(B)):
        h.upload3(v, m[0], m[1], m[2], np.zeros(h.npres))
    return va, vb


@pytest.mark.parametrize("lx1,ranks", [(6, (2, 3)), (8, (2,))])
def test_hexahedral_shards(lx1, ranks):
    """4: the 12-constant slot rebuilt per rank (lx1 = 8: read by the matrix-core convection kernel), phase 0.37, three steps."""
    from nekstab_amd.capi import NekStabHip
    from nekstab_amd.sharded import ShardGroup
    case, q, kw = _box(lx1)
    A, B = _box_modes(case)
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **kw)
    try:
        h.set_orbit_modes(*_upload_modes3(h, A, B), PERIOD)
        dt, ns = h.dt, h.nsteps
        h.set_option("orbit_phase", 0.37)
        h.set_nsteps(3)
        vq, vf = h.alloc(2)
        h.upload3(vq, *q)
        refs = []
        for mode in (0, 1):
            h.matvec(vf, vq, mode); refs.append(h.download3(vf))
        for nranks in ranks:
            g = ShardGroup(h, case, nranks)
            va, vb = _upload_modes3(g, A, B)
            g.set_orbit_modes(va, vb, PERIOD)
            assert g.get_orbit_modes() == (2, PERIOD) and g.nsteps == ns and abs(g.dt - dt) < 1e-15
            g.set_option("orbit_phase", 0.37)
            g.set_nsteps(3)
            sq, sf = g.alloc(2)
            g.upload3(sq, *q)
            for mode in (0, 1):
                g.matvec(sf, sq, mode)
                err = _max3(g.download3(sf), refs[mode])
                print("lx1", lx1, "mode", mode, "map over the Fourier orbit,", nranks, "hexahedral shards: max diff", err)
                assert err < 1e-6
            g.close()
    finally:
        h.close()


@pytest.mark.parametrize("dim", [2, 3])
def test_launch_forms(case6, oracle6_nosolve, modes, dim):
    """5: captured, eager and host-checked sharded steps over the Fourier orbit, two consecutive maps each: bit-identical, same
    iteration counts (the condition of test_host_checked_convergence_equals_budgeted_launches)."""
    from nekstab_amd.capi import NekStabHip
    from nekstab_amd.sharded import ShardGroup
    if dim == 2:
        case = case6
        u = modes["dRe_u"].astype(np.float64)
        q = (u[0], u[1], oracle6_nosolve.J12 @ modes["dRe_p"].astype(np.float64) @ oracle6_nosolve.J12.T)
        kw = dict(tol_helm=1e-12, tol_pres=1e-6, tol_relative=1, nproj=8, max_helm_iter=120, max_pres_iter=48)
        nst, R = 14, 3
        A, B = _synthetic_modes(case.ub, case.x)
        up = _upload_modes2
    else:
        case, q, kw = _box(6)
        nst, R = 4, 2
        A, B = _box_modes(case)
        up = _upload_modes3
    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **kw)
    try:
        out, its = {}, {}
        for name, opts in (("graph", {}), ("eager", {"shard_graph": 0}), ("hostcheck", {"shard_hostcheck": 1})):
            g = ShardGroup(h, case, R)
            for k, v in opts.items():
                g.set_option(k, v)
            g.set_orbit_modes(*up(g, A, B), PERIOD)
            g.set_option("orbit_phase", 0.37)
            g.set_nsteps(nst)
            a, b = g.alloc(2)
            (g.upload if dim == 2 else g.upload3)(a, *q)
            res = []
            for rep in range(2):
                g.matvec(b, a, 0)
                res.append((g.download if dim == 2 else g.download3)(b))
                g.copy(a, b)
            out[name] = res
            st = g.stats()
            its[name] = (st["helm_iters"], st["pres_iters"])
            g.close()
        print("iterations of the last map (velocity, pressure):", its)
        for name in ("eager", "hostcheck"):
            for rep in range(2):
                for x0, x1 in zip(out["graph"][rep], out[name][rep]):
                    assert np.array_equal(x0, x1), (name, rep)
            assert its[name] == its["graph"]
    finally:
        h.close()
