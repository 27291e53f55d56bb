"""Worker of tests/test_boostconv_gpu.py: one rank of nsk_group_boostconv_map whose ranks are separate PROCESSES sharing one
GPU (rank-local set-up, the shard cut from it, halos and sums over torch.distributed / gloo on the host).  The 2 snp + 1 sums of
every call go through the transport's all-reduce inside the map, then every rank solves the small system on its own: every
rank must hold the same bits of residu, they must be the sums over ALL ranks, and the coefficients must have been the same --
a whole-mesh context in the same process gives the residu to compare with; the residu of the calls behind the first carry
the coefficients of the calls before them (1e-6 is far above what the solver tolerances leave)."""
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
    from nekstab_amd.capi import NekStabHip
    from nekstab_amd.sharded import LocalParent, ShardRank, attach_host_transport, partition_rcb
    golden = os.path.join(ROOT, "tests", "golden")
    lx1, nst, snp, skip = 6, 6, 3, 2
    case = mesh.load_case_npz(os.path.join(golden, "cylinder_case.npz"), lx1, spng_str=0.0)
    kw = dict(tol_helm=1e-14, tol_pres=1e-10, tol_relative=1, max_helm_iter=150, max_pres_iter=96, nproj=8)     # (those of the oracle test: residu to 6.5e-10 of itself there)
    zp = np.zeros((case.nel, lx1 - 2, lx1 - 2))
    q0 = (case.ub[0] * (1 + 0.05 * np.sin(case.y)), case.ub[1] + 0.02 * np.cos(case.x) * case.mask, zp)

    part = partition_rcb(case, world)
    lp = LocalParent(case, part, rank, **kw)
    lp.finish_dist(dist)
    sh = ShardRank(lp, case, rank, world, None, part)
    attach_host_transport(sh, dist)
    sh.release_parent()
    q, f = sh.alloc(2)
    sh.upload(q, *q0)
    sh.set_nsteps(nst)
    sh.boostconv_init(snp)
    res = sh.boostconv_map(f, q, skip, 0)
    assert len(res) == 4, res

    both = [torch.zeros(len(res), dtype=torch.float64) for _ in range(world)]
    dist.all_gather(both, torch.from_numpy(res.copy()))
    same = all(np.array_equal(b.numpy(), res) for b in both)

    h = NekStabHip(case, case.meta["vert"], case.meta["nvert"], **kw)
    a, b = h.alloc(2)
    h.upload(a, *q0)
    h.set_nsteps(nst)
    h.boostconv_init(snp)
    one = h.boostconv_map(b, a, skip, 0)
    err = float(np.abs(res / one - 1.0).max())
    print("MPBCV rank %d of %d: %d elements, residu identical on every rank: %s, against the single rank %.2e, residu of call 1 %.4e"
          % (rank, world, len(sh.elems), same, err, res[1]), flush=True)
    ok = same and err <= 1e-6 and np.all(res > 0) and lp.nel < 0.8 * case.nel
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    h.close(); sh.close(); lp.close()
    dist.destroy_process_group()
    sys.exit(0 if flag.item() == 1.0 else 1)


if __name__ == "__main__":
    main()
