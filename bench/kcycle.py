"""The reference's family (UA + pairwise HEM + SGS + coarse scaling, DESIGN.md
section 2.13) with the W-cycle against the nonlinear AMLI cycle (K-cycle) on
the bidomain_3d driver's meshes: setup time, ms per apply (graph replays),
PCG iterations to 1e-8, time to solution, ops (launches) per apply.

    python bench/kcycle.py --nrefs 4,5 --degrees 2,3                 # the DESIGN table
    python bench/kcycle.py --nrefs 4,5 --degrees 2 --tail 0,1        # ... with the K ops in the coarse tail
    MAMG_LIB=.../libmamg_diag.so MAMG_OP_PROFILE=1 python bench/kcycle.py --nrefs 4 --ops

One JSON line per (mesh, profile) on stdout.  ms per apply: the median of
--trials windows of --reps replays of the apply graph, timed with device
events after a warm-up window.  Time to solution: the device-resident PCG,
warmed by one solve, median of three.  --ops (diagnosis build with
MAMG_OP_PROFILE): the per-kind launch counts the library prints are summed
into ops_per_apply (a coarse-tail program counts as one).  launches_per_apply
is the same count from the handle's op list (mamg_apply_launches), which needs
no diagnosis build.  --tail: the K profiles run once per listed state of
MetricAMG.set_kcycle_tail (0: the inner CG's steps as launches, 1: inside the
coarse tail; tagged "K(m)+tail"); W runs once.
"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def profiles(degrees):
    import metric_amg_examples_amd as M
    P = M.parameters
    out = [('W', P.to_gpu_profile(P.parameters_metric)[0])]
    for m in degrees:
        out.append(('K(%d)' % m, P.to_gpu_profile(dict(P.parameters_metric_kcycle, amli_degree=m))[0]))
    return out


def count_ops(B, r, z):
    """launches per apply from the diagnosis build's MAMG_OP_PROFILE lines (stderr of one instrumented apply)"""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode='w+') as f:
        saved = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            B.time_apply(r, z, 1, mode=1)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read()
    counts = [float(v) for v in re.findall(r'\[mamg op\].*launches/apply ([0-9.]+)', text)]
    return int(round(sum(counts))) if counts else None


def measure(nrefs, tag, prm, reps, trials, ops, ktail=False):
    import numpy as np
    import torch
    import metric_amg_examples_amd as M
    n = M.problems.finest_n(3, nrefs)
    s = M.problems.bidomain(3, n, 1e6)
    b = M.problems.bidomain_mms_rhs(3, n, 1e6)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    B = M.MetricAMG(s, s.W, idofs=s.idofs, parameters=prm, kcycle_tail=ktail)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    r = torch.as_tensor(np.asarray(b, np.float64)).cuda()
    z = torch.empty_like(r)
    for _ in range(max(3, reps // 4)):                  # graph capture and warm-up
        B.apply_device(r, z)
    torch.cuda.synchronize()
    ms = []
    for _ in range(trials):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            B.apply_device(r, z)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    solver = M.ConjGrad(s, precond=B, tolerance=1e-8, maxiter=500, device=True)
    x = torch.zeros_like(r)
    solve_s = []
    for k in range(4):                                  # the first solve warms the iteration graph
        x.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        solver.solve_device(r, x)
        torch.cuda.synchronize()
        if k:
            solve_s.append(time.perf_counter() - t0)
    out = dict(profile=tag, nrefs=nrefs, n=n, ndofs=int(s.N), levels=B.num_levels,
               setup_s=round(setup_s, 4), ms_per_apply=round(statistics.median(ms), 4),
               ms_per_apply_trials=[round(v, 4) for v in ms], niters=len(solver.residuals) - 1,
               solve_s=round(statistics.median(solve_s), 4), apply_bytes=B.apply_bytes,
               tail=B.tail_info().get('tail_level'), kcycle_tail=int(B.kcycle_tail),
               tail_programs=len(B.tail_info()['programs']), launches_per_apply=B.apply_launches(),
               ops_per_apply=count_ops(B, r, z) if ops else None)
    B.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nrefs', default='4,5')
    ap.add_argument('--degrees', default='2,3')
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--ops', action='store_true')
    ap.add_argument('--tail', default='0', help="states of set_kcycle_tail for the K profiles, e.g. 0,1")
    args = ap.parse_args()
    degrees = [int(v) for v in args.degrees.split(',') if v]
    tails = [int(v) for v in args.tail.split(',') if v]
    if not tails or any(v not in (0, 1) for v in tails):
        ap.error('--tail takes 0, 1 or 0,1')
    for nrefs in (int(v) for v in args.nrefs.split(',')):
        for tag, prm in profiles(degrees):
            for kt in ([0] if tag == 'W' else tails):
                print(json.dumps(measure(nrefs, tag + ('+tail' if kt else ''), prm, args.reps, args.trials, args.ops,
                                         bool(kt))), flush=True)


if __name__ == '__main__':
    main()
