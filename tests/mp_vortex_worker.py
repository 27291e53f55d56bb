"""Worker of tests/test_vortex_gpu.py: one rank of nsk_group_vortex_criteria whose ranks are separate PROCESSES sharing one GPU.
Rank-local set-up (LocalParent), the shard cut from it, the parent released.  The criteria are element-local: the transport is
attached as every sharded run has it, and must carry nothing.  Every rank compares its own elements with the numpy restatement
on the whole mesh."""
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
    u = np.load(os.path.join(golden, "cylinder_modes.npz"))["dRe_u"].astype(np.float64)
    ref = S.np_vortex_criteria(S.NpGeom(case), u, 0.5)

    part = partition_rcb(case, world)
    lp = LocalParent(case, part, rank, tol_helm=1e-12, tol_pres=1e-6, tol_relative=1, max_helm_iter=120, max_pres_iter=48)
    lp.finish_dist(dist)
    sh = ShardRank(lp, case, rank, world, None, part)
    tr = attach_host_transport(sh, dist)
    sh.release_parent()
    e = sh.elems
    zp = np.zeros((case.nel, lx1 - 2, lx1 - 2))
    rel = lambda a, b: np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b))

    q, w, om, w2, om2 = sh.alloc(5)
    sh.upload(q, u[0], u[1], zp)
    n0 = tr.n_exchange
    sh.vortex_criteria(w, q, 0.5, omega=om)
    sh.vortex_criteria(w2, q, 0.5, omega=om2)
    n1 = tr.n_exchange
    lam, qq, p = sh.download_local(w)
    ox, oy, op = sh.download_local(om)
    qa, qb, _ = sh.download_local(q)
    errs = [rel(a, b[e]) for a, b in zip((lam, qq, ox), ref)]
    rest = float(max(np.abs(p).max(), np.abs(oy).max(), np.abs(op).max()))
    same = all(np.array_equal(a, b) for a, b in zip(sh.download_local(w) + sh.download_local(om), sh.download_local(w2) + sh.download_local(om2)))
    same = same and np.array_equal(qa, u[0][e]) and np.array_equal(qb, u[1][e])
    print("MPVOX rank %d of %d: %d elements, lambda2 / Q / Omega against whole-mesh numpy %.2e %.2e %.2e, other slots %.1e, two calls "
          "identical and q untouched: %s, exchanges %d" % (rank, world, len(e), errs[0], errs[1], errs[2], rest, same, n1 - n0), flush=True)
    ok = max(errs) <= 1e-12 and rest == 0.0 and same and n1 == n0 and lp.nel < 0.8 * case.nel
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    sh.close(); lp.close()
    dist.destroy_process_group()
    sys.exit(0 if flag.item() == 1.0 else 1)


if __name__ == "__main__":
    main()
