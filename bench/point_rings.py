"""The 3D-1D solve (problems.emi_3d1d, BASELINE config 5) with the reference's
own level-0 smoother -- the seed rings on the CSR layout with point-wise GS on
the rest (-schwarz rings) -- next to the additive
preset: PCG iterations, setup and setup + PCG seconds, ms per apply (eager,
mamg_time_apply, and replayed from the apply graph) and, with the diagnosis
build, the launches per apply.

    python bench/point_rings.py --schwarz rings                       # the DESIGN table
    MAMG_LIB=<parent build>/libmamg.so python bench/point_rings.py --schwarz additive
    MAMG_LIB=.../libmamg_diag.so MAMG_OP_PROFILE=1 python bench/point_rings.py --schwarz rings --ops \
        --radii 1.0 --gammas 1e4

One JSON line per (radius, gamma) on stdout.  --ops makes the library print its
per-kind launch counts to stderr (diagnosis build, MAMG_OP_PROFILE).  The
additive column of the table is timed with the parent commit's library
(MAMG_LIB), which does not know the rings.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(n, radius, gamma, schwarz, reps, ops=False):
    import numpy as np
    import torch
    import metric_amg_examples_amd as M
    from metric_amg_examples_amd import drivers as D
    s = M.problems.emi_3d1d(n, gamma, radius)
    A = s.scipy()
    b = M.problems.seeded_rhs(s.N)
    torch.cuda.synchronize()
    t0 = time.time()
    B = D._metric_amg_3d1d(A, s.W, s.idofs, D._params_3d1d(schwarz))
    torch.cuda.synchronize()
    t1 = time.time()
    cg = M.ConjGrad(A, precond=B, tolerance=1e-6, maxiter=1000, stop_type=1)      # the driver's solve
    x = cg * b
    torch.cuda.synchronize()
    t2 = time.time()
    xs = x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)
    relres = float(np.linalg.norm(b - A @ xs) / np.linalg.norm(b))
    r = torch.as_tensor(np.asarray(b, np.float64)).cuda()
    z = torch.empty_like(r)
    B.time_apply(r, z, 5)                               # warm-up
    eager = [B.time_apply(r, z, reps)[0] for _ in range(3)]
    B.apply_device(r, z)                                # captures the graph
    torch.cuda.synchronize()
    graph = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            B.apply_device(r, z, torch.cuda.current_stream())
        e1.record()
        e1.synchronize()
        graph.append(e0.elapsed_time(e1) / reps)
    ms1, kms, cb = B.time_apply(r, z, reps, mode=1)
    if ops:
        print('[point_rings] op profile: %s radius %g gamma %g' % (schwarz, radius, gamma), file=sys.stderr, flush=True)
        B.time_apply(r, z, 1, mode=1)
    out = dict(schwarz=schwarz, n=n, radius=radius, gamma=gamma, ndofs=int(s.N), seeds=int(len(s.idofs)),
               levels=B.num_levels, setup_path=B.setup_path, niters=len(cg.residuals) - 1, relres=relres,
               setup_s=round(t1 - t0, 4), pcg_s=round(t2 - t1, 4), timeKSP=round(t2 - t0, 4),
               ms_per_apply_eager=[round(v, 4) for v in eager], ms_per_apply_graph=[round(v, 4) for v in graph],
               l0_smooth_ms=round(kms[1], 4), l0_smooth_bytes=cb[1], apply_bytes=B.apply_bytes,
               lib=os.environ.get('MAMG_LIB', 'libmamg.so'))
    B.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--schwarz', default='rings', choices=('rings', 'additive'))
    ap.add_argument('--n', type=int, default=48)
    ap.add_argument('--radii', default='0,1.0,5.0')
    ap.add_argument('--gammas', default='1,1e4,1e8')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--ops', action='store_true')
    args = ap.parse_args()
    for radius in (float(v) for v in args.radii.split(',')):
        for gamma in (float(v) for v in args.gammas.split(',')):
            print(json.dumps(measure(args.n, radius, gamma, args.schwarz, args.reps, args.ops)), flush=True)


if __name__ == '__main__':
    main()
