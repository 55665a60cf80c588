"""The hazmath preset (point-wise multicolour SGS) on the
bidomain drivers' meshes: PCG iterations, ms per apply (mamg_time_apply) and,
with the diagnosis build, the launches per apply and the row threshold of the
one-workgroup smoothing kernel.

    python bench/point_gs.py --tags hazmath,amg                      # the DESIGN table
    MAMG_LIB=.../libmamg_diag.so MAMG_OP_PROFILE=1 python bench/point_gs.py --tags hazmath --ops
    MAMG_LIB=.../libmamg_diag.so python bench/point_gs.py --small-sweep 0,1024,2048,4096,8192 [--sweep-case 3,32]

One JSON line per measurement on stdout.  --ops makes the library print its
per-kind launch counts to stderr (diagnosis build, MAMG_OP_PROFILE); the
sweep sets MAMG_CSR_GS_SMALL before each setup (diagnosis build; 0 = every
level launched colour by colour).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(dim, n, tag, reps, ops=False):
    import numpy as np
    import torch
    import metric_amg_examples_amd as M
    from metric_amg_examples_amd import drivers as D
    s = M.problems.bidomain(dim, n, 1.0)
    b = M.problems.bidomain_mms_rhs(dim, n, 1.0, 2, 3)
    prm = D._profile_params('reference', tag)
    t0 = time.time()
    x, niters, cond, dt, res, B = D._solve(s, s.W, b, tag, s.idofs, 1e-8, 500, prm)
    torch.cuda.synchronize()
    wall = time.time() - t0
    r = torch.as_tensor(np.asarray(b, np.float64)).cuda()
    z = torch.empty_like(r)
    B.time_apply(r, z, 5)                               # warm-up
    ms = [B.time_apply(r, z, reps)[0] for _ in range(3)]
    if ops:
        print('[point_gs] op profile: %s %d-D n=%d' % (tag, dim, n), file=sys.stderr, flush=True)
        B.time_apply(r, z, 1, mode=1)
    out = dict(tag=tag, dim=dim, n=n, ndofs=int(s.N), levels=B.num_levels, layout=B.layout, niters=niters,
               cond=round(cond, 3), timeKSP=round(wall, 4), ms_per_apply=[round(v, 4) for v in ms],
               apply_bytes=B.apply_bytes, small_rows=os.environ.get('MAMG_CSR_GS_SMALL', 'default'))
    B.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tags', default='hazmath')
    ap.add_argument('--dims', default='2,3')
    ap.add_argument('--nrefs', type=int, default=3)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--ops', action='store_true')
    ap.add_argument('--small-sweep', default='')
    ap.add_argument('--sweep-case', default='2,128', help='dim,n of the threshold sweep')
    args = ap.parse_args()
    if args.small_sweep:                                # alternating, three rounds
        dim, n = (int(v) for v in args.sweep_case.split(','))
        for rnd in range(3):
            for v in args.small_sweep.split(','):
                os.environ['MAMG_CSR_GS_SMALL'] = v
                print(json.dumps(dict(measure(dim, n, 'hazmath', args.reps, args.ops and rnd == 0), round=rnd)),
                      flush=True)
        return
    for tag in args.tags.split(','):
        for dim in (int(d) for d in args.dims.split(',')):
            i0 = 5 if dim == 2 else 3
            for n in (2 ** i for i in range(i0, i0 + args.nrefs)):
                print(json.dumps(measure(dim, n, tag, args.reps, args.ops)), flush=True)


if __name__ == '__main__':
    main()
