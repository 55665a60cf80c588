#!/usr/bin/env python3
"""Host loop against the device-resident loop of DistConjGrad.

    python bench/dist_pcg.py [--cases rccl1_bidomain,rccl1_3d1d,virtual2] [--rounds 3] [--out FILE]

In one process, on the same handles and the same b: one warm-up solve of
each loop, then `rounds` timed solves of each, alternating host / device.
A solve's wall time is read between two torch.cuda.synchronize() calls and
divided by its iteration count.  Cases:

  rccl1_bidomain  one rank over a one-rank RCCL communicator, bidomain 3-D
                  n = 128, default profile (4.3 M dofs: one rank's share of
                  the north-star size at N = 8), cbc.block rule, 1e-8
  rccl1_3d1d      the same on 3D-1D n = 48, parameters_metric_3d1d, stop type
                  1 (||r|| <= 1e-6 ||b||)
  virtual2        two virtual ranks, bidomain 3-D n = 64; the device loop
                  eager and as one captured lockstep iteration

Prints one JSON line per case (ms per iteration of every round, iteration
counts -- which must be equal --, the pcg_launches table) and a table.  No
run on two or more GPUs: a one-rank communicator exchanges nothing.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, solve):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = solve()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, n


def run_case(M, torch, name, handles, bs, loops, rounds, **kw):
    """loops: {label: dict of for_handles keywords}; the first is the host loop"""
    solvers = {k: M.DistConjGrad.for_handles(handles, **dict(kw, **v)) for k, v in loops.items()}
    xs = [torch.zeros_like(b) for b in bs]

    def solve(label):
        cg = solvers[label]
        if cg._device is None:
            cg.solve(bs)
        else:
            for x in xs:
                x.zero_()
            cg.solve(bs, xs)
        return len(cg.residuals) - 1

    iters = {k: timed(torch, lambda k=k: solve(k))[1] for k in loops}      # warm-up (graph capture, allocations)
    ms = {k: [] for k in loops}
    for _ in range(rounds):
        for k in loops:
            t, n = timed(torch, lambda k=k: solve(k))
            assert n == iters[k]
            ms[k].append(round(t / max(n, 1), 4))
    hs = handles if isinstance(handles, list) else [handles]
    stop = kw.get('stop_type')
    out = {'case': name, 'ranks': len(hs), 'local_dofs': [h.local_size for h in hs], 'iterations': iters,
           'ms_per_iteration': ms, 'apply_launches': hs[0].apply_launches,
           'pcg_launches': hs[0].pcg_launches(stop), 'tolerance': kw['tolerance'], 'stop_type': stop or 0}
    assert len(set(iters.values())) == 1, iters
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='rccl1_bidomain,rccl1_3d1d,virtual2')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--n-bidomain', type=int, default=128)
    ap.add_argument('--n-3d1d', type=int, default=48)
    ap.add_argument('--n-virtual', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import metric_amg_examples_amd as M
    torch.cuda.init()
    st = torch.cuda.current_stream()
    host, dev = dict(stream=st), dict(stream=st, device=True)
    rows = []
    for case in args.cases.split(','):
        if case == 'rccl1_bidomain':
            n = args.n_bidomain
            A = M.problems.bidomain_device(3, n, 1e6)
            s = M.problems.bidomain_meta(3, n, A[1].numel())
            h = M.DistMetricAMG(A, s.W, idofs=s.idofs, rank=0, nranks=1, comm_id=M.DistMetricAMG.unique_id(),
                                num_functions=2)
            bs = [torch.as_tensor(h.local_slice(M.problems.seeded_rhs(s.N))).cuda()]
            row = run_case(M, torch, '%s_n%d' % (case, n), h, bs, {'host': host, 'device': dev}, args.rounds,
                           tolerance=1e-8, maxiter=500)
            h.close()
            del A
        elif case == 'rccl1_3d1d':
            n = args.n_3d1d
            s = M.problems.emi_3d1d(n, 1e4, 1.0)
            h = M.DistMetricAMG(s.scipy(), None, idofs=s.idofs, parameters=M.parameters.parameters_metric_3d1d,
                                rank=0, nranks=1, comm_id=M.DistMetricAMG.unique_id())
            b = np.ascontiguousarray(h.local_slice(M.problems.seeded_rhs(s.N)))
            row = run_case(M, torch, '%s_n%d' % (case, n), h, [torch.as_tensor(b).cuda()],
                           {'host': host, 'device': dev}, args.rounds, tolerance=1e-6, maxiter=1000, stop_type=1)
            h.close()
        elif case == 'virtual2':
            n = args.n_virtual
            A = M.problems.bidomain_device(3, n, 1e6)
            s = M.problems.bidomain_meta(3, n, A[1].numel())
            hs = [M.DistMetricAMG(A, s.W, idofs=s.idofs, rank=p, nranks=2, comm_id=None, num_functions=2)
                  for p in range(2)]
            r = M.problems.seeded_rhs(s.N)
            bs = [torch.as_tensor(h.local_slice(r)).cuda() for h in hs]
            row = run_case(M, torch, '%s_n%d' % (case, n), hs, bs,
                           {'host': host, 'device_eager': dev, 'device_graph': dict(dev, graph=True)},
                           args.rounds, tolerance=1e-8, maxiter=500)
            for h in hs:
                h.close()
            del A
        else:
            raise SystemExit('unknown case ' + case)
        rows.append(row)
        print(json.dumps(row), flush=True)
    print('%-24s %-14s %5s  %s' % ('case', 'loop', 'iters', 'ms / iteration per round'))
    for row in rows:
        for k, v in row['ms_per_iteration'].items():
            print('%-24s %-14s %5d  %s' % (row['case'], k, row['iterations'][k], ' '.join('%.4f' % t for t in v)))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
