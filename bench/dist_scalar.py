"""The cost of the row-partitioned cycle of a scalar (CSR) hierarchy (DESIGN.md
section 6.5): the 3D-1D system (problems.emi_3d1d, n = 48, radius 1,
parameters_metric_3d1d) on P = 1, 2, 4, 8 virtual ranks of one GPU.

    python bench/dist_scalar.py                    # this tree's library
    MAMG_LIB=<parent build>/libmamg.so python bench/dist_scalar.py --one-gpu

Per P, one JSON line per rank: owned rows and ghosts per level, what one apply
issues (kernels, send / receive groups, messages, all-reduces, side-stream
forks: mamg_dist_apply_launches) and the rank-local compute per apply, eager
and replayed from the graph, with the exchanges skipped (MAMG_DIST_TEST=dry:
timing only, the results are meaningless); then one line with the distributed
PCG's iteration count on real virtual ranks.  --one-gpu prints the one-GPU
apply time and PCG count instead (any library: the parent commit's via
MAMG_LIB, for the comparison column).  No speed-up is claimed: at 117,716 rows
the cycle is latency-bound; the table records what the partition costs.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def system(n, gamma, radius):
    import metric_amg_examples_amd as M
    s = M.problems.emi_3d1d(n, gamma, radius)
    return M, s, s.scipy(), M.problems.seeded_rhs(s.N), dict(M.parameters.parameters_metric_3d1d)


def one_gpu(args):
    import numpy as np
    import torch
    M, s, A, b, prm = system(args.n, args.gamma, args.radius)
    B = M.MetricAMG(A, s.W, idofs=s.idofs, parameters=prm)
    cg = M.ConjGrad(A, precond=B, tolerance=1e-6, maxiter=1000, stop_type=1)
    cg * b
    r = torch.as_tensor(np.asarray(b, np.float64)).cuda()
    z = torch.empty_like(r)
    B.time_apply(r, z, 5)
    eager = [round(B.time_apply(r, z, args.reps)[0], 4) for _ in range(3)]
    B.apply_device(r, z)
    torch.cuda.synchronize()
    graph = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            B.apply_device(r, z, torch.cuda.current_stream())
        e1.record()
        e1.synchronize()
        graph.append(round(e0.elapsed_time(e1) / args.reps, 4))
    print(json.dumps(dict(one_gpu=True, lib=os.environ.get('MAMG_LIB', 'tree'), ndofs=int(s.N), levels=B.num_levels,
                          niters=len(cg.residuals) - 1, ms_per_apply_eager=eager, ms_per_apply_graph=graph,
                          apply_bytes=B.apply_bytes)), flush=True)
    B.close()


def ranks(args, P, dry):
    import torch
    M, s, A, b, prm = system(args.n, args.gamma, args.radius)
    M._lib.set_option('MAMG_DIST_TEST', 'dry' if dry else None)
    hs = [M.DistMetricAMG(A, s.W, idofs=s.idofs, parameters=prm, rank=p, nranks=P, comm_id=None,
                          rep_nodes=args.rep_nodes) for p in range(P)]
    M._lib.set_option('MAMG_DIST_TEST', None)
    return M, s, A, b, prm, hs, torch


def dist(args, P):
    import numpy as np
    M, s, A, b, prm, hs, torch = ranks(args, P, True)
    H = M.HostHierarchy(A, idofs=s.idofs, parameters=prm)
    for p, h in enumerate(hs):
        plan = M.DistPlan(H, p, P, args.rep_nodes)
        lv = [plan.level(l) for l in range(plan.num_levels)]
        r = torch.as_tensor(np.ascontiguousarray(h.local_slice(b))).cuda()
        z = torch.empty_like(r)
        h.time_apply(r, z, 5)
        eager = [round(h.time_apply(r, z, args.reps)[0], 4) for _ in range(3)]
        graph = [round(h.time_apply(r, z, args.reps, mode=2)[0], 4) for _ in range(3)]
        print(json.dumps(dict(P=P, rank=p, owned=[x['nloc'] for x in lv], ghosts=[len(x['ghosts']) for x in lv],
                              replicated=[x['replicated'] for x in lv], launches=h.apply_launches,
                              compute_ms_eager=eager, compute_ms_graph=graph, apply_bytes=h.apply_bytes)), flush=True)
        plan.close()
    for h in hs:
        h.close()
    H.close()
    M, s, A, b, prm, hs, torch = ranks(args, P, False)
    cg = M.DistConjGrad.for_handles(hs if P > 1 else hs[0], tolerance=1e-6, maxiter=1000, stop_type=1)
    xs = cg.solve([torch.as_tensor(np.ascontiguousarray(h.local_slice(b))).cuda() for h in hs])
    x = np.concatenate([v.cpu().numpy() for v in xs])
    print(json.dumps(dict(P=P, niters=len(cg.residuals) - 1,
                          relres=float(np.linalg.norm(b - A @ x) / np.linalg.norm(b)))), flush=True)
    for h in hs:
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=48)
    ap.add_argument('--gamma', type=float, default=1e4)
    ap.add_argument('--radius', type=float, default=1.0)
    ap.add_argument('--ranks', type=int, nargs='*', default=[1, 2, 4, 8])
    ap.add_argument('--rep-nodes', type=int, default=32768)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--one-gpu', action='store_true')
    args = ap.parse_args()
    if args.one_gpu:
        one_gpu(args)
        return
    for P in args.ranks:
        dist(args, P)


if __name__ == '__main__':
    main()
