"""Inputs and CPU references for the edges of the PCG loops (nonzero x0,
relative tolerance, breakdown, maxiter 0, b = 0) -- TEST INFRASTRUCTURE ONLY.

The reference is never the code under test: mamg_oracle.pcg around the
oracle's apply for the cbc.block rule, and for stop type 1 the host loop
krylov.ConjGrad(device=False, stop_type=1) around the oracle's apply (as
tests/test_gpu_dist_pcg.py).  A preconditioner that is not positive comes from
the public parameters: over-relaxed Jacobi (relaxation > 2) makes the V-cycle
indefinite on the high frequencies, the setup accepts it, and the GPU
hierarchy stays the oracle's, so the oracle's breakdown and restore are an
independent reference for every branch of the device state machines.

tests/test_pcg_edges_ref.py pins, with the reference alone, that every input
below does what the GPU tests (tests/test_gpu_pcg_edges.py) rely on.
"""
import numpy as np

import mamg_oracle as mo

# name -> (dim, n, gamma, num_functions) of problems.bidomain
SYSTEMS = {'b3': (3, 16, 1e4, 2), 'b2': (2, 32, 1e4, 2), 'c2': (2, 16, 1e4, 1), 'c3': (3, 16, 1.0, 1)}


def _case(system, relaxation=None, b='seeded', x0=None, tol=1e-8, relativeconv=False, stop=0, outcome='converged',
          k=None):
    return dict(system=system, relaxation=relaxation, b=b, x0=x0, tol=tol, relativeconv=relativeconv, stop=stop,
                outcome=outcome, k=k)


# outcome / k: what the reference does (k: completed iterations; None: not tabulated, the reference decides).
# rz_neg at k means <r,Br> < 0 in iteration k: k completed iterations, k + 1 residuals, x = x_k restored.
CASES = {
    # breakdown and rejection
    'neg2': _case('b3', 3.0, outcome='rz_neg', k=2),
    'neg1x': _case('b3', 3.0, x0='x7', outcome='rz_neg', k=1),
    'neg0': _case('b3', 4.0, outcome='rz_neg', k=0),
    'neg0_x7': _case('b3', 4.0, x0='x7', outcome='rz_neg', k=0),
    'neg1': _case('b2', 2.5, outcome='rz_neg', k=1),
    'neg1_x7': _case('b2', 2.5, x0='x7', outcome='rz_neg', k=1),
    'notpos': _case('b2', 4.0, b='checker', outcome='not_pos', k=0),
    'notpos_x7': _case('b2', 4.0, b='checker', x0='x7', outcome='not_pos', k=0),
    'ok3': _case('b3', 3.0, b='checker', k=11),
    'csr0': _case('c2', 4.0, outcome='rz_neg', k=0),
    'neg2_s1': _case('b3', 3.0, tol=1e-6, stop=1, outcome='rz_neg', k=2),
    # healthy parameters, default relaxation
    'h3': _case('b3', k=35),
    'h3_x7': _case('b3', x0='x7', k=35),
    'h3_rel': _case('b3', x0='x7', tol=1e-6, relativeconv=True, k=21),
    'h3_b0': _case('b3', b='zero', x0='x7', k=33),
    'h2': _case('b2', k=26),
    'h2_x7': _case('b2', x0='x7', k=26),
    'h2_rel': _case('b2', x0='x7', tol=1e-6, relativeconv=True, k=16),
    'h2_b0': _case('b2', b='zero', x0='x7', k=26),
    'c3_x7': _case('c3', x0='x7'),
    # stop type 1 (||r|| <= tol ||b||, ||b|| = 0 taken as 1)
    'h3_x7_s1': _case('b3', x0='x7', tol=1e-6, stop=1),
    'h2_x7_s1': _case('b2', x0='x7', tol=1e-6, stop=1),
    'h3_b0_s1': _case('b3', b='zero', x0='x7', tol=1e-6, stop=1),
    'h2_b0_s1': _case('b2', b='zero', x0='x7', tol=1e-6, stop=1),
}
MAXITER = 500
_cache = {}


def checker(dim, n):
    """+-1 by the parity of the vertex's index sum on the (n+1)^dim grid: v on
    field 1 and -v on field 2 (the highest frequency the mesh carries)"""
    idx = np.indices((n + 1,) * dim).sum(axis=0).ravel()
    v = np.where(idx % 2 == 0, 1.0, -1.0)
    return np.concatenate([v, -v])


def system(name):
    """(A, nodal system): built once, shared, read-only"""
    k = ('sys', name)
    if k not in _cache:
        import metric_amg_examples_amd as M
        dim, n, gamma, _ = SYSTEMS[name]
        s = M.problems.bidomain(dim, n, gamma)
        _cache[k] = (s.scipy(), s)
    return _cache[k]


def param_kw(case):
    """the keywords both mo.Params and MetricAMG / DistMetricAMG take for this case"""
    c = CASES[case]
    kw = dict(num_functions=SYSTEMS[c['system']][3])
    if c['relaxation'] is not None:
        kw['relaxation'] = c['relaxation']
    return kw


def handle(case):
    """the oracle hierarchy of the case's (system, relaxation), shared"""
    c = CASES[case]
    k = ('h', c['system'], c['relaxation'])
    if k not in _cache:
        A, s = system(c['system'])
        _cache[k] = mo.setup(A, mo.Params(**param_kw(case)), idofs=s.idofs)
    return _cache[k]


def vectors(case):
    """(b, x0): x0 is zeros when the case starts from 0; read-only"""
    c = CASES[case]
    k = ('v', c['system'], c['b'], c['x0'])
    if k not in _cache:
        dim, n, _, _ = SYSTEMS[c['system']]
        N = system(c['system'])[0].shape[0]
        b = {'seeded': lambda: mo.seeded_rhs(N), 'checker': lambda: checker(dim, n),
             'zero': lambda: np.zeros(N)}[c['b']]()
        x0 = mo.seeded_rhs(N, 7) if c['x0'] == 'x7' else np.zeros(N)
        b.setflags(write=False)
        x0.setflags(write=False)
        _cache[k] = (b, x0)
    return _cache[k]


class _OracleB:
    """the oracle's apply behind the `B * r` the host ConjGrad calls"""

    def __init__(self, apply):
        self.apply = apply

    def __mul__(self, r):
        return self.apply(r)


def _run(case, apply):
    import warnings
    c = CASES[case]
    A = system(c['system'])[0]
    b, x0 = vectors(case)
    tol = c['tol']
    if c['stop'] == 0:
        try:
            ref = mo.pcg(A, apply, np.array(b), tol, MAXITER, x0=np.array(x0), relativeconv=c['relativeconv'])
        except ValueError as e:
            assert 'not positive' in str(e)
            return 'not_pos', 0, np.array(x0), np.zeros(0), np.zeros(0), np.zeros(0), None
        res = np.array(ref.residuals)
        k = len(res) - 1
        thr = tol * res[0] if c['relativeconv'] else tol
        outcome = 'rz_neg' if (k < MAXITER and res[-1] > thr) else 'converged'
        return outcome, k, np.array(ref.x), res, np.array(ref.alphas), np.array(ref.betas), None
    import metric_amg_examples_amd as M
    cg = M.ConjGrad(A, precond=_OracleB(apply), tolerance=tol, maxiter=MAXITER, device=False, stop_type=1,
                    relativeconv=c['relativeconv'], initial_guess=np.array(x0))
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            x = cg * np.array(b)
    except ValueError as e:
        assert 'not positive' in str(e)
        return 'not_pos', 0, np.array(x0), np.zeros(0), np.zeros(0), np.zeros(0), None
    res = np.array(cg.residuals)
    return ('rz_neg' if cg.breakdown else 'converged', len(res) - 1, np.array(x), res, np.array(cg.alphas),
            np.array(cg.betas), np.array(cg.residual_norms))


def reference(case):
    """(outcome, k, x, residuals, alphas, betas) of the reference solve:
    outcome 'converged' | 'rz_neg' | 'not_pos' (the ValueError; x = x0, empty
    histories), k completed iterations.  Computed once per case, read-only."""
    k = ('ref', case)
    if k not in _cache:
        out = _run(case, handle(case).apply)
        for a in out[2:]:
            if a is not None:
                a.setflags(write=False)
        _cache[k] = out
    return _cache[k][:6]


def reference_norms(case):
    """the ||r||_2 history of a stop type 1 case's reference solve"""
    reference(case)
    return _cache[('ref', case)][6]


def margins(case):
    """What makes the case decisive, from the reference's own vectors:
    not_pos: (<r0,Br0>, ||r0||^2);
    rz_neg:  (<r,Br> before the break, the negative <r,Br>, ||alpha d||,
              ||x_k + alpha d||) with d rebuilt from the z the oracle returned
              (d_0 = z_0, d_j+1 = z_j+1 + beta_j d_j)."""
    c = CASES[case]
    A = system(c['system'])[0]
    b, x0 = vectors(case)
    h = handle(case)
    if c['outcome'] == 'not_pos':
        r0 = b - A @ x0
        return float(np.dot(r0, h.apply(r0))), float(np.dot(r0, r0))
    rs, zs = [], []

    def traced(r):
        z = h.apply(r)
        rs.append(np.array(r))
        zs.append(np.array(z))
        return z
    outcome, k, x, res, al, be = _run(case, traced)[:6]
    assert outcome == 'rz_neg' and len(zs) == k + 2
    rz = [float(np.dot(r, z)) for r, z in zip(rs, zs)]
    d = zs[0].copy()
    for j in range(k):
        d = zs[j + 1] + be[j] * d
    alpha = rz[k] / float(np.dot(d, A @ d))
    return rz[k], rz[k + 1], float(np.linalg.norm(alpha * d)), float(np.linalg.norm(x + alpha * d))
