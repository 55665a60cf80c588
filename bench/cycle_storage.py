"""fp64 against fp32 cycle storage on one GPU.

One process sets up two handles of the same hierarchy (A_0 generated in HBM,
GPU setup, as bench.py), narrows one with mamg_set_cycle_storage and times the
two alternately:

  python bench/cycle_storage.py [--nrefs 6] [--dim 3] [--gamma 1e6] [--smoother jacobi|poly]
                                [--rounds 3] [--steps 20] [--out FILE]

Per handle and round: ms per apply of the eager launches (mamg_time_apply
mode 0, with events around the level-0 residual and K) and of the hipGraph
replays (events around `steps` mamg_apply_device calls), the algorithmic
bytes and TB/s of class 0 (residual), class 1 (K) and class 3 (restriction;
its time from one all-ops run, mode 1).  Once per handle: the device PCG to
1e-8 (iterations, seconds of a second, warm solve, the residual history when
the counts differ), the HBM the handle holds (free-memory difference with the
setup cache released) and the wall time of the narrowing call itself.
One JSON object per line; the last line is the summary.

  --trace f32|f64   build one handle, apply `steps` times and exit: the run to
                    put under `rocprofv3 --kernel-trace --stats -- python ...`
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C_RESID, C_K, C_R = 0, 1, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nrefs', type=int, default=6)
    ap.add_argument('--dim', type=int, default=3)
    ap.add_argument('--gamma', type=float, default=1e6)
    ap.add_argument('--smoother', choices=('jacobi', 'poly'), default='jacobi')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace', choices=('f32', 'f64'), default=None)
    args = ap.parse_args()

    import torch
    import metric_amg_examples_amd as M
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev)
    L = M._lib.lib()
    prof = dict(smoother={'jacobi': 3, 'poly': 12}[args.smoother], poly_degree=2)
    n = M.problems.finest_n(args.dim, args.nrefs, 'bidomain')
    out = open(args.out, 'w') if args.out else None

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    def free_bytes():
        torch.cuda.synchronize(dev)
        L.mamg_release_setup_cache()
        return torch.cuda.mem_get_info(dev)[0]

    def build():
        A0 = M.problems.bidomain_device(args.dim, n, args.gamma, device=dev)
        meta = M.problems.bidomain_meta(args.dim, n, int(A0[1].numel()))
        B = M.MetricAMG(A0, meta.W, idofs=meta.idofs, num_functions=2, setup='gpu', **prof)
        del A0
        torch.cuda.empty_cache()
        return B, meta

    if args.trace:
        B, meta = build()
        if args.trace == 'f32':
            B.set_cycle_storage('f32')
        r = torch.as_tensor(M.problems.seeded_rhs(meta.N)).to(dev)
        z = torch.zeros_like(r)
        for _ in range(args.steps + 3):
            B.apply_device(r, z, stream)
        torch.cuda.synchronize(dev)
        B.close()
        return

    f0 = free_bytes()
    B64, meta = build()
    f1 = free_bytes()
    B32, _ = build()
    f2 = free_bytes()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    B32.set_cycle_storage('f32')
    torch.cuda.synchronize(dev)
    t_narrow = time.perf_counter() - t0
    f3 = free_bytes()
    handles = {'f64': B64, 'f32': B32}
    emit({'what': 'setup', 'dim': args.dim, 'n': n, 'N': meta.N, 'smoother': args.smoother, 'gamma': args.gamma,
          'levels': B64.num_levels, 'level_storage_f32': [B32.level_storage(l) for l in range(B32.num_levels)],
          'level0_format': B32.level_format(0), 'handle_bytes_f64': f0 - f1, 'handle_bytes_f32_before_narrowing': f1 - f2,
          'handle_bytes_f32': f1 - f3, 'set_cycle_storage_s': round(t_narrow, 4),
          'apply_bytes': {k: B.apply_bytes for k, B in handles.items()}, 'kregion_f64': B64.kregion})

    r = torch.as_tensor(M.problems.seeded_rhs(meta.N)).to(dev)
    zs = {k: torch.zeros_like(r) for k in handles}
    for k, B in handles.items():                     # warm-up: graph capture and eager launches
        for _ in range(3):
            B.apply_device(r, zs[k], stream)
        B.time_apply(r, zs[k], 3, 0, stream)
    torch.cuda.synchronize(dev)
    d = (zs['f32'] - zs['f64']).norm().item() / zs['f64'].norm().item()
    emit({'what': 'apply_difference', 'rel_f32_vs_f64': d})

    rows = {k: [] for k in handles}
    for rnd in range(args.rounds):
        for k, B in handles.items():                 # alternating
            ms, kms, cb = B.time_apply(r, zs[k], args.steps, 0, stream)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.steps):
                B.apply_device(r, zs[k], stream)
            e1.record(stream)
            torch.cuda.synchronize(dev)
            gms = e0.elapsed_time(e1) / args.steps
            _, kall, _ = B.time_apply(r, zs[k], max(3, args.steps // 4), 1, stream)
            row = {'what': 'round', 'round': rnd, 'storage': k, 'eager_ms': round(ms, 4), 'graph_ms': round(gms, 4),
                   'applies_per_s_graph': round(1e3 / gms, 2)}
            for name, c, t in (('resid', C_RESID, kms[C_RESID]), ('k', C_K, kms[C_K]), ('restrict', C_R, kall[C_R])):
                row[name + '_ms'] = round(t, 4)
                row[name + '_bytes'] = cb[c]
                row[name + '_TBps'] = round(cb[c] / (t * 1e-3) / 1e12, 3) if t > 0 else None
            rows[k].append(row)
            emit(row)

    pcg = {}
    hist = {}
    for k, B in handles.items():
        maxiter = 500
        res = (C.c_double * (maxiter + 1))()
        al = (C.c_double * maxiter)()
        be = (C.c_double * maxiter)()
        nit = C.c_int32()
        secs = []
        for _ in range(2):                           # the second solve replays the cached iteration graph
            x = torch.zeros_like(r)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            M._lib.check(L.mamg_pcg_device(B.handle, C.c_void_p(r.data_ptr()), C.c_void_p(x.data_ptr()), 1e-8, maxiter,
                                           0, res, al, be, C.byref(nit), C.c_void_p(stream.cuda_stream)))
            torch.cuda.synchronize(dev)
            secs.append(round(time.perf_counter() - t0, 4))
        hist[k] = [res[i] for i in range(nit.value + 1)]
        pcg[k] = {'niters': nit.value, 'seconds_first': secs[0], 'seconds_warm': secs[1], 'residual': hist[k][-1],
                  'x': x}
    dx = (pcg['f32']['x'] - pcg['f64']['x']).norm().item() / pcg['f64']['x'].norm().item()
    for k in pcg:
        del pcg[k]['x']
    row = {'what': 'pcg', 'f64': pcg['f64'], 'f32': pcg['f32'], 'rel_solution_difference': dx}
    if pcg['f64']['niters'] != pcg['f32']['niters']:
        row['residuals_f64'], row['residuals_f32'] = hist['f64'], hist['f32']
    emit(row)

    def med(k, key):
        v = sorted(x[key] for x in rows[k])
        return v[len(v) // 2]

    keys = ('eager_ms', 'graph_ms', 'resid_ms', 'k_ms', 'restrict_ms')
    emit({'what': 'summary', 'median': {k: {q: med(k, q) for q in keys} for k in handles},
          'range': {k: {q: [min(x[q] for x in rows[k]), max(x[q] for x in rows[k])] for q in keys} for k in handles},
          'speedup_graph': round(med('f64', 'graph_ms') / med('f32', 'graph_ms'), 4),
          'pcg_iters': {k: pcg[k]['niters'] for k in pcg}})
    for B in handles.values():
        B.close()


if __name__ == '__main__':
    main()
