#!/usr/bin/env python3
"""VMB aggregation of the GPU setup: the parent commit's library (the strong
graph goes to the host and the sequential loop runs there) against this
tree's (worklist rounds on the device), in
alternating child processes of one session.

    python bench/vmb_setup.py --parent-lib <parent build>/libmamg.so \
        [--nrefs 4 5 6] [--rounds 3] [--entries host device] [--out FILE]

Profiles on bidomain_3d: parameters_standard on the nodal system (gamma 1e6)
and the hazmath point-wise preset (num_functions 1, gamma 1).  Entry points:
mamg_setup_gpu (A on the host) and mamg_setup_gpu_device (A generated in HBM,
never on the host).  Every child runs one warming setup, then one setup per
profile and size, smallest first, and prints one JSON line per setup: the
aggregation phase (mamg_setup_timings[0]), the setup wall, the process's
peak RSS so far and, with this tree's library, mamg_test_vmb_info per level.
Variants: `parent`; `new`, this tree's default (the device path from the size
threshold up, the host path below); `new_device`, mamg_test_set_vmb(2) and no
round cap: the device path on every level; `new_host`, mamg_test_set_vmb(0): the host path on
every level.  The last two give the two paths' time per level side by side,
which the threshold and the round cap of DESIGN.md section 2.10 come from.
`process_peak_rss_mb` is the child's ru_maxrss so far: it includes the torch
import and the warming setups, so it compares variants and is no absolute
footprint of the setup.

The parent prints every line, then per (profile, nrefs, entry, variant) the
medians over the rounds.
"""
import argparse
import json
import os
import resource
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW_SYMBOLS = ('mamg_test_set_vmb', 'mamg_test_vmb_info')


def child(args):
    import metric_amg_examples_amd as M
    if args.variant == 'parent':                 # the parent's library has no VMB hooks
        for k in NEW_SYMBOLS:
            M._lib.SIGNATURES.pop(k, None)
    import torch
    P = M.parameters
    if args.variant != 'parent':
        # new_device: no round cap either, so that every level's rounds run to their end
        M._lib.set_vmb({'new': 1, 'new_device': 2, 'new_host': 0}[args.variant], (1 << 40) if args.variant == 'new_device' else -1)

    def setup(profile, n):
        gamma = 1e6 if profile == 'standard_nodal' else 1.0
        dev = M.problems.bidomain_device(3, n, gamma)
        torch.cuda.synchronize()
        nv = (n + 1) ** 3
        if args.entry == 'host':
            A = tuple(t.cpu().numpy() for t in dev)
            del dev
            torch.cuda.empty_cache()
        else:
            A = dev
        t = time.perf_counter()
        if profile == 'standard_nodal':
            B = M.MetricAMG(A, [nv, nv], parameters=P.parameters_standard, setup='gpu')
        else:
            params, _ = M.precond.amg_pointwise_parameters(P.parameters_standard)
            B = M.MetricAMG(A, None, parameters=params, setup='gpu')
        torch.cuda.synchronize()
        wall = time.perf_counter() - t
        out = dict(variant=args.variant, entry=args.entry, profile=profile, n=n, N=2 * nv,
                   aggregate_ms=B.setup_timings['aggregate'], setup_total_ms=B.setup_timings['setup_total'],
                   wall_ms=round(1e3 * wall, 2), levels=B.num_levels,
                   process_peak_rss_mb=round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, 1))
        if args.variant != 'parent':
            lv = []
            while M._lib.vmb_info(len(lv)) is not None:
                lv.append(M._lib.vmb_info(len(lv)))
            out['vmb'] = lv
        B.close()
        return out

    setup('standard_nodal', 8)                   # HIP context and code objects before any timing
    setup('hazmath_pointwise', 8)
    for nrefs in args.nrefs:
        for profile in args.profiles:
            print(json.dumps(setup(profile, M.problems.finest_n(3, nrefs))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib')
    ap.add_argument('--nrefs', type=int, nargs='+', default=[4, 5, 6])
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--entries', nargs='+', default=['host', 'device'])
    ap.add_argument('--profiles', nargs='+', default=['standard_nodal', 'hazmath_pointwise'])
    ap.add_argument('--variants', nargs='+', default=['parent', 'new', 'new_device', 'new_host'])
    ap.add_argument('--timeout', type=int, default=900)
    ap.add_argument('--out')
    ap.add_argument('--variant')                 # child
    ap.add_argument('--entry')
    args = ap.parse_args()
    if args.variant:
        return child(args)
    if 'parent' in args.variants and not (args.parent_lib and os.path.exists(args.parent_lib)):
        sys.exit('--parent-lib: the parent commit\'s libmamg.so is needed for the variant "parent"')
    rows = []
    sink = open(args.out, 'a') if args.out else None
    for rnd in range(args.rounds):
        for entry in args.entries:
            for variant in args.variants:
                env = dict(os.environ)
                env.pop('MAMG_LIB', None)
                if variant == 'parent':
                    env['MAMG_LIB'] = os.path.abspath(args.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), '--variant', variant, '--entry', entry,
                       '--nrefs', *map(str, args.nrefs), '--profiles', *args.profiles]
                p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
                for line in p.stdout.splitlines():
                    if line.startswith('{'):
                        r = dict(json.loads(line), round=rnd)
                        rows.append(r)
                        print(json.dumps(r), flush=True)
                        if sink:
                            sink.write(json.dumps(r) + '\n')
                            sink.flush()
                if p.returncode:                       # a fault or a time limit: nothing more on the GPU
                    sys.exit('child %s/%s ended with status %d' % (variant, entry, p.returncode))
    keys = sorted({(r['profile'], r['n'], r['entry'], r['variant']) for r in rows})
    for k in keys:
        g = [r for r in rows if (r['profile'], r['n'], r['entry'], r['variant']) == k]
        s = dict(summary='median over rounds', profile=k[0], n=k[1], entry=k[2], variant=k[3], rounds=len(g),
                 aggregate_ms=statistics.median(r['aggregate_ms'] for r in g),
                 wall_ms=statistics.median(r['wall_ms'] for r in g),
                 process_peak_rss_mb=max(r['process_peak_rss_mb'] for r in g))
        print(json.dumps(s), flush=True)
        if sink:
            sink.write(json.dumps(s) + '\n')


if __name__ == '__main__':
    main()
