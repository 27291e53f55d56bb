"""Worker of tests/test_vorticity_gpu.py: one rank of nsk_group_vorticity whose ranks are separate PROCESSES sharing one GPU.
Rank-local set-up (LocalParent), the shard cut from it, the parent released; the halo of the mass-weighted curl (and, once, of
the mass) travels through torch.distributed (gloo) on the host.  Every rank compares its own elements with the numpy
restatement on the whole mesh."""
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
    ref = S.np_vorticity(S.NpGeom(case), u)[0]

    part = partition_rcb(case, world)
    lp = LocalParent(case, part, rank, tol_helm=1e-12, tol_pres=1e-6, tol_relative=1, max_helm_iter=120, max_pres_iter=48)
    lp.finish_dist(dist)
    sh = ShardRank(lp, case, rank, world, None, part)
    tr = attach_host_transport(sh, dist)
    sh.release_parent()
    e = sh.elems
    zp = np.zeros((case.nel, lx1 - 2, lx1 - 2))
    rel = lambda a, b: np.linalg.norm(np.ravel(a - b)) / np.linalg.norm(np.ravel(b))

    q, w, w2 = sh.alloc(3)
    sh.upload(q, u[0], u[1], zp)
    sh.vorticity(w, q)
    n1 = tr.n_exchange                                              # first call: the mass, then the curl
    sh.vorticity(w2, q)
    n2 = tr.n_exchange                                              # every later call: ONE exchange
    a, b, p = sh.download_local(w)
    a2, b2, p2 = sh.download_local(w2)
    qa, qb, _ = sh.download_local(q)
    err = rel(a, ref[e])
    rest = float(max(np.abs(b).max(), np.abs(p).max()))
    same = np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(qa, u[0][e]) and np.array_equal(qb, u[1][e])
    print("MPVORT rank %d of %d: %d elements, error against whole-mesh numpy %.2e, other slots %.1e, two calls identical and q untouched: %s, "
          "exchanges %d then %d" % (rank, world, len(e), err, rest, same, n1, n2 - n1), flush=True)
    ok = err <= 1e-12 and rest == 0.0 and same and n1 == 2 and n2 - n1 == 1 and lp.nel < 0.8 * case.nel
    flag = torch.tensor([1.0 if ok else 0.0])
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    sh.close(); lp.close()
    dist.destroy_process_group()
    sys.exit(0 if flag.item() == 1.0 else 1)


if __name__ == "__main__":
    main()
