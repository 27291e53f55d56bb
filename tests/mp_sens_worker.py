"""Worker of tests/test_sensitivity_sharded_gpu.py: one rank of the sharded eigenmode post-processing whose ranks are separate
PROCESSES sharing one GPU.  Rank-local set-up (LocalParent), the shard cut from it, the parent released; halos of the gradient
and divergence fields and the sums of norms and integrals travel through torch.distributed (gloo) on the host.  Every rank
compares its own elements and the integrals with the numpy restatement on the whole mesh."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from nekstab_amd import mesh
    from nekstab_amd import sensitivity as S
    from nekstab_amd.sharded import LocalParent, ShardRank, attach_host_transport, partition_rcb
    golden = os.path.join(ROOT, "tests", "golden")
    lx1 = 6
    case = mesh.load_case_npz(os.path.join(golden, "cylinder_case.npz"), lx1)
    m = np.load(os.path.join(golden, "cylinder_modes.npz"))
    raw = [S.interp_gll(m[k + "_u"].astype(np.float64), lx1) for k in ("dRe", "dIm", "aRe", "aIm")]
    geom = S.NpGeom(case)
    bio = S.np_biorthogonalize(geom, *raw)
    ref_s = S.np_bf_sensitivity(geom, *bio[:4])
    ref_b = S.np_energy_budget(geom, case.ub, raw[0], raw[1], 1.0 / case.re)

    part = partition_rcb(case, world)
    lp = LocalParent(case, part, rank, tol_helm=1e-12, tol_pres=1e-6, tol_relative=1, max_helm_iter=120, max_pres_iter=48)
    lp.finish_dist(dist)
    sh = ShardRank(lp, case, rank, world, None, part)
    tr = attach_host_transport(sh, dist)
    sh.release_parent()
    e = sh.elems
    zp = np.zeros((case.nel, lx1 - 2, lx1 - 2))
    rel = lambda a, b: np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b))
    errs = {}

    # biorthogonalisation of the raw modes: norms and <a, d> summed over the ranks
    v = sh.alloc(4)
    for vec, u in zip(v, raw):
        sh.upload(vec, u[0], u[1], zp)
    gamma, delta = sh.biorthogonalize(*v)
    errs["gamma"] = abs(gamma - bio[4]) / abs(bio[4])
    errs["delta"] = abs(delta - bio[5]) / abs(bio[5])
    for vec, u in zip(v, bio[:4]):                                  # the references' modes from here on, as the single-rank tests
        sh.upload(vec, u[0], u[1], zp)
    outs = sh.alloc(6)
    sh.bf_sensitivity(*v, outs[0], outs[1], parts=outs[2:])
    for k, o in zip(("sr", "si", "tr", "ti", "pr", "pi"), outs):
        a, b, p = sh.download_local(o)
        errs[k] = rel(np.array([a, b]), ref_s[k][:, e])
        errs[k + "_p"] = float(np.abs(p).max())

    ub, dRe, dIm = sh.alloc(3)
    sh.upload(ub, case.ub[0], case.ub[1], zp)
    sh.upload(dRe, raw[0][0], raw[0][1], zp)
    sh.upload(dIm, raw[1][0], raw[1][1], zp)
    integrals = sh.energy_budget(ub, dRe, dIm, prod=outs[:2], diss=outs[2])
    for c in range(2):
        a, b, _ = sh.download_local(outs[c])
        errs["prod%d" % c] = rel(np.array([a, b]), ref_b["prod"][c][:, e])
    d, d1, dp = sh.download_local(outs[2])
    errs["diss"] = rel(d, ref_b["diss"][e])
    errs["diss_rest"] = float(max(np.abs(d1).max(), np.abs(dp).max()))
    errs["integrals"] = np.max(np.abs(integrals - ref_b["integrals"])) / np.max(np.abs(ref_b["integrals"]))

    both = [torch.zeros(10, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(both, torch.from_numpy(integrals.copy()))
    same = all(np.array_equal(b.numpy(), integrals) for b in both)  # every rank holds the same bits
    worst = max(errs.values())
    print("MPSENS rank %d of %d: %d elements, worst error %.2e (%s), integrals identical on all ranks: %s, exchanges %d allreduces %d"
          % (rank, world, len(e), worst, max(errs, key=errs.get), same, tr.n_exchange, tr.n_allreduce), flush=True)
    ok = worst <= 1e-12 and same and tr.n_exchange > 0 and tr.n_allreduce > 0 and lp.nel < 0.8 * case.nel
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    sh.close(); lp.close()
    dist.destroy_process_group()
    sys.exit(0 if flag.item() == 1.0 else 1)


if __name__ == "__main__":
    main()
