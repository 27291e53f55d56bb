"""CPU-side checks: the C-ABI library loads and exports every declared symbol, file formats,
case preparation, the seed, and the multi-process timing reduction used by bench.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import GOLDEN, ROOT


def test_capi_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()
    from nekstab_amd import capi
    lib = capi.load_library()
    hdr = open(os.path.join(ROOT, "include", "nekstab_hip.h")).read()
    declared = set(re.findall(r"\b(nsk_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/nekstab_hip.h but not exported"
    assert declared == set(capi.SYMBOLS), (declared ^ set(capi.SYMBOLS))


def test_no_cpu_fallback_without_gpu(case6):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from nekstab_amd.capi import NekStabHip, NskError
    with pytest.raises(NskError):
        NekStabHip(case6, case6.meta["vert"], case6.meta["nvert"])


def test_product_never_imports_oracle():
    for root, _, files in os.walk(os.path.join(ROOT, "nekstab_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp")):
                txt = open(os.path.join(root, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f


def test_fld_roundtrip(tmp_path):
    from nekstab_amd import nekio
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 7, 1, 6, 6)); u = rng.standard_normal((2, 7, 1, 6, 6)); p = rng.standard_normal((7, 1, 6, 6))
    f = str(tmp_path / "tst0.f00001")
    nekio.write_fld(f, x=x, u=u, p=p, time=1.0, istep=101)
    r = nekio.read_fld(f)
    assert r.istep == 101 and r.rdcode == "XUP" and r.nx == 6
    assert np.array_equal(r.x, x) and np.array_equal(r.u, u) and np.array_equal(r.p, p)


def test_spectre_writer_format(tmp_path, spectre):
    from nekstab_amd import nekio
    H = spectre["Hd"][:12]
    f = str(tmp_path / "Spectre_Hd.dat")
    nekio.write_spectre(f, H[:, 0] + 1j * H[:, 1], H[:, 2])
    back = nekio.read_spectre(f)
    assert np.allclose(back, H, rtol=2e-7, atol=1e-30)
    line = open(f).readline()
    assert len(line.rstrip("\n")) == 45 and "E" in line           # (3E15.7)


def test_case_numbering_and_masks(case6):
    c = case6
    assert c.nel == 1996 and c.nglob == c.gid.max() + 1
    gx = np.zeros(c.nglob); gx[c.gid.ravel()] = c.x.ravel()
    assert np.abs(gx[c.gid] - c.x).max() < 2e-6                   # copies of a node coincide (fp32 mesh file)
    gy = np.zeros(c.nglob); gy[c.gid.ravel()] = c.y.ravel()
    dy = np.abs(gy[c.gid] - c.y)
    assert set(np.unique(np.round(dy[dy > 1e-5]))) <= {32.0}       # only the periodic y pair differs
    r = np.hypot(c.x, c.y)
    assert np.all(c.mask[r < 0.5 + 1e-6] == 0) and np.all(c.ub[:, r < 0.5 + 1e-6] == 0)   # wall nodes
    assert np.all(c.mask[np.abs(c.x + 16) < 1e-9] == 0)           # inflow 'v'
    assert np.all(c.mask[np.abs(c.x - 50) < 1e-9] == 1)           # outflow 'O' stays free (direct)
    assert c.spng.max() == 1.0 and np.all(c.spng[(c.x > -12.6) & (c.x < 46.6)] == 0)


def test_seed_is_deterministic_and_continuous(case6):
    from nekstab_amd import seed
    a = seed.add_noise(case6); b = seed.add_noise(case6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    g = np.zeros(case6.nglob); g[case6.gid.ravel()] = a[0].ravel()
    assert np.abs(g[case6.gid] - a[0]).max() == 0.0               # single-valued on shared nodes
    assert np.all(a[0][case6.mask == 0] == 0)


def test_two_rank_gloo_host_transport_and_timing(tmp_path):
    """The N>1 host protocol on two CPU processes (gloo): the product's host-staged halo transport
    (nekstab_amd.sharded.HostTransport: per-peer exchange + all-reduce, what nsk_comm_init_host calls back into) and
    bench.py's timing reduction (barrier, max-over-ranks time, aggregate = sum of units / max time)."""
    script = tmp_path / "w.py"
    script.write_text(
        "import sys, time, numpy as np, torch, torch.distributed as dist\n"
        "sys.path.insert(0, %r)\n"
        "from nekstab_amd.sharded import HostTransport\n"
        "dist.init_process_group('gloo')\n"
        "r = dist.get_rank(); tr = HostTransport(dist)\n"
        "got = tr.exchange([1 - r], [np.arange(5, dtype=np.float64) + 10 * r])\n"
        "assert np.array_equal(got[0], np.arange(5) + 10 * (1 - r))\n"
        "# through the ctypes callbacks, as the C library calls them\n"
        "import ctypes as C\n"
        "send = (np.ones(3) * (r + 1)); recv = np.zeros(3); dp = C.POINTER(C.c_double)\n"
        "peers = (C.c_int * 1)(1 - r); cnt = (C.c_int * 1)(3)\n"
        "sp = (dp * 1)(send.ctypes.data_as(dp)); rp = (dp * 1)(recv.ctypes.data_as(dp))\n"
        "assert tr.xf(None, 1, peers, cnt, sp, rp) == 0 and np.all(recv == 2 - r)\n"
        "buf = np.array([1.0 + r, 2.0]); assert tr.af(None, buf.ctypes.data_as(dp), 2) == 0 and np.all(buf == [3.0, 4.0])\n"
        "dist.barrier(); t0 = time.perf_counter(); time.sleep(0.05 * (r + 1)); dist.barrier()\n"
        "t = torch.tensor([0.05 * (r + 1)], dtype=torch.float64); dist.all_reduce(t, op=dist.ReduceOp.MAX)\n"
        "units = torch.tensor([10.0]); dist.all_reduce(units)\n"
        "assert abs(t.item() - 0.1) < 1e-12 and units.item() == 20.0\n"
        # (leave together, as test_local_setup_exchange_over_gloo does: a rank that exits with the group still open closes its
        #  sockets under the other rank's gloo threads, which then abort that process -- SIGABRT on rank 1, now and then)
        "dist.barrier(); dist.destroy_process_group()\n"
        "print('ok', r)\n" % ROOT)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29611", str(script)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2000:]
    assert out.stdout.count("ok") == 2


def test_bench_spawns_its_ranks(tmp_path):
    """`python bench.py --gpus N` without a launcher starts N child processes with RANK / WORLD_SIZE set (checked without
    a GPU: the children stop at 'needs a GPU'), and a launcher / --gpus mismatch is an error."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the GPU runs")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and out.stderr.count("bench.py needs a GPU") == 2, out.stderr[-1500:]
    env = dict(os.environ, WORLD_SIZE="1", RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0 and "launcher started 1 ranks" in out.stderr


def test_bench_retries_after_a_stalled_attempt():
    """A stalled first attempt (watchdog exit, STALL_EXIT) must lead to the eager retry in fresh processes; only the unique
    'no GPU' code stops the attempts (both used exit code 3, so a stall ended the run without the retry)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the retry would run the whole sharded bench")
    env = dict(os.environ, NSK_BENCH_TEST_STALL="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode != 0
    assert out.stderr.count("forced stall (test hook)") == 2, out.stderr[-1500:]
    assert "attempt 0 (captured step graphs) failed with code 5: retrying with eager launches in fresh processes" in out.stderr, out.stderr[-1500:]
    assert out.stderr.count("bench.py needs a GPU") == 2, out.stderr[-1500:]        # attempt 1 ran (and ended on the unique no-GPU code)
    assert "attempt 1" not in out.stderr
    rec = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(rec) == 1 and '"value": null' in rec[0]


@pytest.mark.parametrize("nranks", [2, 3, 8])
def test_partition_rcb(case6, nranks):
    """Element partition for sharded runs: every element owned once, balanced, deterministic, and
    spatially compact (few interface nodes compared with a random partition)."""
    from nekstab_amd.sharded import partition_rcb
    p = partition_rcb(case6, nranks)
    assert p.shape == (case6.nel,) and p.min() == 0 and p.max() == nranks - 1
    cnt = np.bincount(p, minlength=nranks)
    assert cnt.max() - cnt.min() <= 1
    assert np.array_equal(p, partition_rcb(case6, nranks))

    def interface_nodes(part):
        owners = np.zeros(case6.nglob, dtype=np.int64)
        np.bitwise_or.at(owners, case6.gid.ravel(), np.repeat(1 << part, case6.lx1 ** 2))
        return int(np.sum((owners & (owners - 1)) != 0))
    rng = np.random.default_rng(0)
    assert interface_nodes(p) < 0.2 * interface_nodes(rng.permutation(p))


def test_spectre_info_manifest(tmp_path, case6):
    """Spectre_<op>.info (core/eigensolvers.f:664-717): same keys, order and edit descriptors as the reference."""
    from types import SimpleNamespace
    from nekstab_amd import outpost
    be = SimpleNamespace(nsteps=100, dt=0.01)
    res = SimpleNamespace(H=np.zeros((201, 200)), schur_cnt=3)
    f = str(tmp_path / "Spectre_d.info")
    outpost.write_info(f, be, case6, res, evop="d", sampling_period=1.0, eigen_tol=1e-6, schur_tgt=2, schur_del=0.1,
                       outposted=10, uparam=[3.1, 0, 0, 5.0, 5.0, 1.7], tol_pres=1e-7, tol_vel=1e-9, nranks=4)
    lines = open(f).read().splitlines()
    assert lines[2] == "[mesh]" and lines[3] == "lx1=             " + "%16d" % 6
    assert lines[5] == "tot elemts=      " + "%16d" % 1996 and lines[8] == "e/rank=          " + "%16d" % 499
    assert lines[9] == "[userParams]" and lines[10] == "uparam01=        " + "  3.100000000000"
    assert lines[20] == "[solver]" and lines[23] == "dt=              " + "  0.1000000E-01"       # (A,E15.7)
    assert lines[25] == "residualTol PRE= " + "   0.1000E-06"                                      # (A,E13.4)
    assert lines[27] == "[eigensolver]" and lines[29] == "k_dim=           " + "%16d" % 200
    assert lines[-1] == "outposted=       " + "%16d" % 10 and len(lines) == 35
    info = outpost.read_info(f)
    assert int(info["schur iterations"]) == 3 and float(info["Re"]) == 50.0 and int(info["nsteps"]) == 100


def test_seed_hexahedral_branch():
    """mth_rand's IF3D branch (core/utils.f:463) in the host mirror: deterministic, single-valued on shared nodes,
    masked, and different from the planar formula."""
    from types import SimpleNamespace
    from nekstab_amd import seed
    n, nel = 4, 2
    z1 = np.linspace(0.0, 1.0, n)
    x = np.zeros((nel, n, n, n)); y = np.zeros_like(x); z = np.zeros_like(x)
    for e in range(nel):
        x[e] = e + z1[None, None, :]; y[e] = z1[None, :, None]; z[e] = z1[:, None, None]
    key = np.round(x * 3).astype(np.int64) * 100 + np.round(y * 3).astype(np.int64) * 10 + np.round(z * 3).astype(np.int64)
    _, gid = np.unique(key, return_inverse=True)
    gid = gid.reshape(x.shape)
    mask = np.ones_like(x); mask[x == 0.0] = 0.0
    c = SimpleNamespace(ndim=3, nel=nel, lx1=n, x=x, y=y, z=z, gid=gid, nglob=int(gid.max()) + 1, mask=mask)
    a = seed.add_noise(c); b = seed.add_noise(c)
    assert len(a) == 3 and all(np.array_equal(p, q) for p, q in zip(a, b))
    g = np.zeros(c.nglob); g[gid.ravel()] = a[2].ravel()
    assert np.array_equal(g[gid], a[2]) and np.all(a[0][mask == 0] == 0)
    r2 = seed._mth_rand(1.0, 2.0, None, 1.0, (0.3, 0.4), seed.FCOEFF[0])
    r3 = seed._mth_rand(1.0, 2.0, 3.0, 1.0, (0.3, 0.4, 0.5), seed.FCOEFF[0])
    assert abs(r2) <= 1 and abs(r3) <= 1 and r2 != r3


def test_scripts_compile():
    """scripts/ holds the measurement drivers DESIGN.md cites (scripts/README.md): keep them syntactically alive."""
    import py_compile
    sdir = os.path.join(ROOT, "scripts")
    names = [f for f in os.listdir(sdir) if f.endswith(".py")]
    assert len(names) >= 15
    for f in names:
        py_compile.compile(os.path.join(sdir, f), doraise=True)
    listed = open(os.path.join(sdir, "README.md")).read()
    for f in names:
        assert f in listed, f + " is not described in scripts/README.md"


def test_fortran_module_binds_every_header_entry():
    """host/nekstab_hip_mod.f90 (the iso_c_binding block INTEGRATION.md hands to a nekStab maintainer) binds EVERY function
    include/nekstab_hip.h declares -- VERDICT r2, row n2."""
    import re
    hdr = open(os.path.join(ROOT, "include", "nekstab_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char\*)\s+(nsk_\w+)\s*\(", hdr, flags=re.M))
    mod = open(os.path.join(ROOT, "host", "nekstab_hip_mod.f90")).read()
    bound = set(re.findall(r"bind\(c, name='(nsk_\w+)'\)", mod))
    assert declared and not (declared - bound), sorted(declared - bound)
    assert not (bound - declared), sorted(bound - declared)


def test_fortran_dense_restart_equals_python_host(tmp_path):
    """The Fortran host's eig / schur / select_eigenvalues / ordschur / truncation (host/krylov_host.f90, the host part of
    schur_condensation, core/eigensolvers.f:395-499) against nekstab_amd/krylov.py on the same Hessenberg matrix: same
    eigenvalues in the same order, same number of kept vectors, same truncated H and basis rotation Z."""
    import shutil
    import subprocess
    exe = os.path.join(ROOT, "host", "dense_check")
    if not os.path.exists(exe):
        if shutil.which("flang") is None:
            pytest.skip("flang not available and host/dense_check not prebuilt")
        subprocess.run(["make", "-C", os.path.join(ROOT, "host"), "dense_check"], check=True, stdout=subprocess.DEVNULL)
    from nekstab_amd import krylov
    from tests.dense_backend import DenseBackend, Vec
    rng = np.random.default_rng(11)
    k, tgt, delta = 30, 3, 0.10
    # a Hessenberg matrix with a few eigenvalues outside the circle of radius 0.9 (what a restart is asked to keep)
    blocks, i = np.zeros((k, k)), 0
    for z in (1.02 * np.exp(0.7j), 0.95 + 0j, 0.93 * np.exp(0.3j)):
        if z.imag == 0:
            blocks[i, i] = z.real; i += 1
        else:
            blocks[i:i + 2, i:i + 2] = [[z.real, z.imag], [-z.imag, z.real]]; i += 2
    while i + 1 < k:
        z = 0.85 * rng.random() * np.exp(2j * np.pi * rng.random())
        blocks[i:i + 2, i:i + 2] = [[z.real, z.imag], [-z.imag, z.real]]; i += 2
    if i < k:
        blocks[i, i] = 0.4
    X = rng.standard_normal((k, k))
    A = X @ blocks @ np.linalg.inv(X)
    import scipy.linalg as sla
    Hk, _ = sla.hessenberg(A, calc_q=True)
    H = np.zeros((k + 1, k))
    H[:k] = Hk
    H[k, k - 1] = 0.37
    fin, fout = str(tmp_path / "H.bin"), str(tmp_path / "out.bin")
    np.asfortranarray(H).T.ravel().tofile(fin)          # column-major stream
    out = subprocess.run([exe, fin, fout, str(k), str(tgt), str(delta)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(fout)
    vals_f = raw[:2 * k:2] + 1j * raw[1:2 * k:2]
    o = 2 * k
    vecs_f = (raw[o:o + 2 * k * k:2] + 1j * raw[o + 1:o + 2 * k * k:2]).reshape(k, k).T
    o += 2 * k * k
    ms_f = int(raw[o]); o += 1
    Hn_f = raw[o:o + (k + 1) * k].reshape(k, k + 1).T; o += (k + 1) * k
    Z_f = raw[o:o + k * k].reshape(k, k).T
    # eig: same values, same order (decreasing modulus; conjugates may swap within a pair of equal modulus)
    vals_p, vecs_p = krylov.eig_sorted(H[:k, :k])
    assert np.abs(np.abs(vals_f) - np.abs(vals_p)).max() < 1e-12
    assert np.abs(np.sort_complex(vals_f) - np.sort_complex(vals_p)).max() < 1e-11
    res_f = np.abs(H[k, k - 1] * vecs_f[k - 1, :]) / np.linalg.norm(vecs_f, axis=0)
    res_p = np.abs(H[k, k - 1] * vecs_p[k - 1, :]) / np.linalg.norm(vecs_p, axis=0)
    assert np.abs(np.sort(res_f) - np.sort(res_p)).max() < 1e-11
    # restart: python host on an identity 'basis' => its rotated basis IS Z
    be = DenseBackend(np.eye(k + 1))
    Q = [Vec(k + 1) for _ in range(k + 1)]
    for j in range(k + 1):
        Q[j].a[j] = 1.0
    Hp = H.copy()
    mstart = krylov.schur_condensation(be, Q, Hp, k, 1, delta, tgt)
    assert mstart == ms_f + 1 and ms_f >= tgt + 4
    Z_p = np.stack([q.a[:k] for q in Q[:k]], axis=1)
    assert np.abs(Hn_f - Hp).max() < 1e-11 * np.abs(H).max()
    assert np.abs(Z_f[:, :ms_f] - Z_p[:, :ms_f]).max() < 1e-11
    # and the restarted factorisation is still a Krylov decomposition:  A Z_1 = Z_1 T + z_{k+1} b^T Z
    T = Hn_f[:ms_f, :ms_f]
    assert np.abs(H[:k, :k] @ Z_f[:, :ms_f] - Z_f[:, :ms_f] @ T).max() < 1e-11


def test_rank_submesh_and_subset_case():
    """Rank-local set-up, host side: the sub-mesh of a rank = its own elements + two rings of node-sharing neighbours, in
    ascending global order, with global node / vertex ids kept."""
    from nekstab_amd import mesh
    from nekstab_amd.sharded import partition_rcb, rank_submesh, subset_case
    case = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 6)
    part = partition_rcb(case, 3)
    gid = case.gid.reshape(case.nel, -1)
    seen = np.zeros(case.nel, dtype=int)
    for r in range(3):
        sub = rank_submesh(case, part, r)
        own = np.where(part == r)[0]
        assert np.all(np.diff(sub) > 0) and np.isin(own, sub).all() and len(sub) < 0.6 * case.nel
        # ring 1 = every element touching a node of an owned element; ring 2 = the same once more
        ring1 = np.where(np.isin(gid, np.unique(gid[own])).any(axis=1))[0]
        ring2 = np.where(np.isin(gid, np.unique(gid[ring1])).any(axis=1))[0]
        assert np.array_equal(sub, ring2)
        assert len(rank_submesh(case, part, r, rings=1)) == len(ring1)
        sc = subset_case(case, sub)
        assert sc.nel == len(sub) and sc.nglob == case.nglob and sc.meta["nvert"] == case.meta["nvert"]
        assert np.array_equal(sc.gid, case.gid[sub]) and np.array_equal(sc.ub, case.ub[:, sub]) and np.array_equal(sc.meta["vert"], np.asarray(case.meta["vert"]).reshape(case.nel, -1)[sub])
        assert sc.x.shape == (len(sub), 6, 6) and case.nel == 1996           # (the whole-mesh case is untouched)
        seen[own] += 1
    assert np.all(seen == 1)


def test_eight_rank_submeshes_and_halo_plans_are_mutually_consistent():
    """Eight ranks before the node arrives, host side, no GPU: on a small extruded hexahedral case every
    rank's sub-mesh (own elements + two rings) gives (i) the SAME dssum interface as the whole mesh -- per peer, the ascending
    list of shared global nodes, which is what fixes message sizes and entry order on both sides --, (ii) lists that agree
    pairwise (what r sends to p is what p expects from r, node for node), (iii) the complete multiplicity / assembled-mass
    stencil of every node of the own and ring-1 elements, which ONE ring does not give."""
    from nekstab_amd import mesh, mesh3d
    from nekstab_amd.sharded import partition_rcb, rank_submesh, velocity_halo_plan
    c2 = mesh.load_case_npz(os.path.join(GOLDEN, "cylinder_case.npz"), 4)
    case = mesh3d.extrude_case(c2, 3, 0.6, periodic=True)
    R = 8
    part = partition_rcb(case, R)
    gid = np.asarray(case.gid).reshape(case.nel, -1)
    mult = np.bincount(gid.ravel(), minlength=int(case.nglob))              # elements' node copies per global node (whole mesh)
    plans, one_ring_short = {}, 0
    for r in range(R):
        sub = rank_submesh(case, part, r)
        assert np.isin(np.where(part == r)[0], sub).all() and len(sub) < 0.7 * case.nel
        whole = velocity_halo_plan(gid, part, r)
        local = velocity_halo_plan(gid[sub], part[sub], r)
        assert sorted(whole) == sorted(local) and all(np.array_equal(whole[p], local[p]) for p in whole), r
        plans[r] = local
        # two rings: multiplicity of every node of the own + ring-1 elements, counted inside the sub-mesh, is the whole-mesh one
        own = np.where(part == r)[0]
        ring1 = rank_submesh(case, part, r, rings=1)
        m2 = np.bincount(gid[sub].ravel(), minlength=int(case.nglob))
        nodes1 = np.unique(gid[ring1])
        assert np.array_equal(m2[nodes1], mult[nodes1]), r
        m1 = np.bincount(gid[ring1].ravel(), minlength=int(case.nglob))
        one_ring_short += int((m1[nodes1] != mult[nodes1]).sum())
        assert np.array_equal(m1[np.unique(gid[own])], mult[np.unique(gid[own])])      # (one ring is enough for the OWN nodes only)
    assert one_ring_short > 0
    npairs = 0
    for r in range(R):
        for p, nodes in plans[r].items():
            assert r in plans[p] and np.array_equal(plans[p][r], nodes), (r, p)        # send list of r -> p == receive list of p <- r
            npairs += 1
    assert npairs >= 2 * (R - 1) and max(len(v) for pl in plans.values() for v in pl.values()) > 0
    print("8 ranks: %d directed neighbour pairs, messages of %d .. %d nodes" % (npairs, min(len(v) for pl in plans.values() for v in pl.values()),
                                                                                   max(len(v) for pl in plans.values() for v in pl.values())))


def test_local_setup_exchange_over_gloo(tmp_path):
    """The exchange of the rank-local set-up (sharded.exchange_local) between two processes: sums, maxima, and every rank's
    coarse rows concatenated in rank order."""
    script = tmp_path / "w.py"
    script.write_text(
        "import sys, numpy as np, torch.distributed as dist\n"
        "sys.path.insert(0, %r)\n"
        "from nekstab_amd.sharded import exchange_local\n"
        "dist.init_process_group('gloo')\n"
        "r = dist.get_rank()\n"
        "n = 3 + 2 * r\n"
        "u = np.arange(n, dtype=np.int32) + 100 * r; v = u[::-1].copy(); a = np.linspace(0.5, 1.5, n) * (r + 1)\n"
        "vol, ct, lm, npr, U, V, A = exchange_local(dist, 1.25 + r, 160 * (r + 1), 3.0 - r, 7.0 + 2 * r, u, v, a)\n"
        "assert vol == 3.5 and npr == 480 and ct == 3.0 and lm == 9.0\n"
        "eu = np.concatenate([np.arange(3), np.arange(5) + 100]); ea = np.concatenate([np.linspace(0.5, 1.5, 3), 2 * np.linspace(0.5, 1.5, 5)])\n"
        "assert U.dtype == np.int32 and np.array_equal(U, eu) and np.array_equal(V, np.concatenate([np.arange(3)[::-1], (np.arange(5) + 100)[::-1]]))\n"
        "assert np.array_equal(A, ea)\n"
        "dist.barrier(); dist.destroy_process_group()\n"
        "print('ok', r)\n" % ROOT)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29617", str(script)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2000:]
    assert out.stdout.count("ok") == 2


def test_lds_stride_table_of_the_matrix_core_passes_is_conflict_free_in_the_bank_model():
    """PadLay<8> (nekstab_amd/csrc/nsk3_mfma_ops.hpp): the per-stage LDS strides of the wavefront-per-element Schwarz kernel,
    checked against the bank model they were searched with (scripts/lds_bank_search.py: ds_read_b64 in two 32-lane groups over
    64 banks, ds_write_b64 in four 16-lane groups over 32 banks).  Every stage of the fast-diagonalisation tile costs its ideal
    cycle count or one group more; the compact strides cost 2-4 times as much."""
    import importlib.util, re
    spec = importlib.util.spec_from_file_location("lds_bank_search", os.path.join(ROOT, "scripts", "lds_bank_search.py"))
    bank = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bank)
    src = open(os.path.join(ROOT, "nekstab_amd", "csrc", "nsk3_mfma_ops.hpp")).read()
    blk = src[src.index("template <> struct PadLay<8>"):]
    F = re.search(r"F\[7\]\[3\] = \{(.*?)\};", blk, re.S).group(1)
    strides = [tuple(int(x) for x in t.split(",")) for t in re.findall(r"\{([^{}]+)\}", F)]
    assert len(strides) == 7
    T, M = (8, 8, 8), 6
    def cost(s, wkind, rkind, sub=None):
        c = 0
        if wkind == "lin": c += bank.lin_w(bank.lin_addr(T, s))
        else:
            cols, ms, MR = bank.cols_for(wkind, T, s); c += bank.wr(MR, cols, ms)
        if rkind == "lin": c += bank.lin_r(bank.lin_addr(T, s, sub))
        else:
            cols, ks, K = bank.cols_for(rkind, T, s); c += bank.rd(K, cols, ks)
        return c
    stages = [("lin", "r"), ("r", "s"), ("s", "t"), ("t", "t"), ("t", "s"), ("s", "r"), ("r", "lin")]
    compact = (64, 8, 1)
    tot_pad = tot_cmp = 0
    for st, (w, r) in zip(strides, stages):
        assert bank.injective(T, st, 640)
        sub = (1, (M, M, M)) if r == "lin" else None
        tot_pad += cost(st, w, r, sub); tot_cmp += cost(compact, w, r, sub)
    print("LDS cycles of one fast-diagonalisation solve in the bank model: padded", tot_pad, "compact", tot_cmp)
    assert tot_pad <= 370 and tot_cmp >= 2.5 * tot_pad


def test_reference_logfile_ingestion(tmp_path):
    """bench.py --ref-logfile: the reference's own per-iteration timing (core/krylov_decomposition.f:75, :92-98) and Nek5000's
    step lines -> matvecs/s of the reference run; without step lines the whole-minute lines give a lower bound."""
    import bench
    lines = [" iteration current and total:           1 /          32"]
    for i in range(1, 184):
        lines.append("Step %6d, t= %.7E, DT= 5.4644809E-03, C=  0.494 %.4E 2.0000E-02" % (i, i * 5.4644809e-3, 0.02 * i))
    lines += [" Time per iteration/remaining:  0h  1min /  0h  1min", "", " iteration current and total:           2 /          32"]
    for i in range(1, 184):
        lines.append("Step %6d, t= %.7E, DT= 5.4644809E-03, C=  0.494 %.4E 3.0000E-02" % (i, i * 5.4644809e-3, 3.66 + 0.03 * i))
    lines += [" Time per iteration/remaining:  0h  1min /  0h  1min", " iteration current and total:           3 /          32", "Step      1, t= 5.4644809E-03, DT= 5.4644809E-03, C=  0.494 9.0000E+00 1.0000E+00"]
    f = tmp_path / "logfile"
    f.write_text("\n".join(lines) + "\n")
    r = bench.parse_reference_logfile(str(f))
    assert r["iterations"] == 2 and r["k_dim"] == 32 and r["time_steps_per_iteration"] == 183.0
    assert abs(r["s_per_iteration"] - 183 * 0.025) < 1e-9 and abs(r["matvecs_per_s"] - 1.0 / (183 * 0.025)) < 1e-12
    f.write_text("\n".join(l for l in lines if not l.startswith("Step")) + "\n")
    r = bench.parse_reference_logfile(str(f))
    assert r["iterations"] == 2 and r["s_per_iteration_upper_bound"] == 60.0 and "matvecs_per_s" not in r
    f.write_text("nothing here\n")
    assert "error" in bench.parse_reference_logfile(str(f))
