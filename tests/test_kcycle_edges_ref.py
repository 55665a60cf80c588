"""The conditions tests/test_gpu_kcycle_edges.py relies on, established on the
CPU reference alone (tests/kcycle_ref.py, oracle/mamg_oracle.py), for every
(case, seed) it runs.  These are conditions on the inputs, not measurements of
the library: an input that misses one is replaced (another sigma of
tests/kcycle_edge_cases.py's range), the condition is not relaxed.

1. One apply of a K case meets a visit with a kept step followed by a dropped
   one, and a visit with every step dropped; a coarse-scaling case meets a
   denominator <= 0 and one > 0.

   A dropped step followed by a *kept* one cannot occur, whatever the system:
   a dropped step has alpha = 0 and leaves r as it was, so the next step's
   z = M(r) and w = A z are the same vectors, the dead direction's beta is 0
   and the live ones' are the same numbers, p and q come out the same and so
   does d <= 0.  The test asserts exactly that (every step after a dropped one
   repeats its d bit for bit), which is also where beta_i = 0 of a dead
   direction runs on non-zero data: <z, q_i> = d_i < 0 there.
2. Every |d| / (||p|| ||q||) and every scaling cosine |den| / (||e|| ||A_c e||)
   is at least 1e-3, so a rounding difference cannot flip a decision; a zero
   product occurs only as the scaling of an e that an all-dropped visit left
   exactly zero.
3. A relative 1e-13 perturbation of the right-hand side moves the apply by at
   most 1e-11 (the factor 100 of tests/test_kcycle_ref.py), which entitles the
   GPU cases to the project's 1e-10.
4. The restatement without the guards (always dividing) is more than 1e-3 away
   from the guarded one or not finite, and so is the restatement without one
   guard alone, where that guard can decide anything: alpha's in every K case,
   the scaling's in every scaling case, and the beta's from degree 3 on (at
   degree 2 the stale beta_0 = <p_0, q_0> / d_0 = 1 makes p_1 = 0 and d_1 = 0,
   which alpha's guard drops as well).

Census of the cases as chosen (both seeds): smallest margin 1.1e-2, largest
amplification of the 1e-13 perturbation 2.3e-12.
"""
import numpy as np
import pytest

import kcycle_cases as kc
import kcycle_edge_cases as ke
import mamg_oracle as mo

CASE_SEEDS = [(n, s) for n in ke.INDEFINITE for s in ke.SEEDS]


def _M():
    import metric_amg_examples_amd as M
    return M


def pattern(steps):
    return ''.join('k' if d > 0 else 'D' for d, _ in steps)


@pytest.mark.parametrize('name,seed', CASE_SEEDS)
def test_conditions_of_the_gpu_cases(name, seed):
    kind, sigma, kw, m, visit = ke.INDEFINITE[name]
    c = ke.census(name, seed)
    pats = [pattern(steps) for _, steps in c['visits']]
    dens = [d for d, _ in c['scalings']]
    print('%s sigma %g seed %d: visits %s, scalings %d <= 0 and %d > 0, margin %.2e, 1e-13 in -> %.2e out, '
          'without guards %s' % (name, sigma, seed, {p: pats.count(p) for p in sorted(set(pats))},
                                 sum(d <= 0 for d in dens), sum(d > 0 for d in dens), c['margin'], c['moved'],
                                 {k: '%.1e' % v for k, v in c['unguarded'].items()}))
    assert np.isfinite(ke.reference(name)[seed]).all()
    # 1
    if visit == 'K':
        assert any('kD' in p for p in pats), pats
        assert any(set(p) == {'D'} for p in pats), pats
        assert not any('Dk' in p for p in pats), pats
        for _, steps in c['visits']:
            assert len(steps) == m
            dead = [d for d, _ in steps if not d > 0]
            assert all(d == dead[0] and d < 0 for d in dead), steps
    else:
        assert pats == []
    if kw.get('coarse_scaling'):
        assert any(d <= 0 for d in dens) and any(d > 0 for d in dens), dens
    else:
        assert dens == []
    # 2
    assert c['margin'] >= 1e-3, c['margin']
    assert all(pq > 0 for _, steps in c['visits'] for _, pq in steps)
    alldead = sum(set(p) == {'D'} for p in pats)
    assert c['zeros'] == sum(1 for d, eq in c['scalings'] if eq == 0 and d == 0) <= alldead
    # 3
    assert c['moved'] <= 1e-11, c['moved']
    # 4
    u = c['unguarded']
    assert u[()] > 1e-3
    if visit == 'K':
        assert u[('beta', 'scale')] > 1e-3
        if m >= 3:
            assert u[('alpha', 'scale')] > 1e-3
    if kw.get('coarse_scaling'):
        assert u[('alpha', 'beta')] > 1e-3


def test_trace_and_wrapper_leave_the_arithmetic_alone():
    """the traced restatement, and the oracle under the recording wrapper, give
    the bits of the plain ones; the wrapper is gone afterwards"""
    name = 'sgs_scaling_m2'
    r = ke.rhs(name, 7)
    before = mo.coarse_scale
    trace, log = [], []
    with ke.scaling_recorded(log):
        z = ke.restatement(name, trace).apply(r)
    assert mo.coarse_scale is before
    assert np.array_equal(z, ke.reference(name)[7]) and trace and log
    assert [(lv, j) for lv, j, _, _ in trace if lv == 1] == [(1, 0), (1, 1)]
    # on an SPD system nothing is dropped and the unguarded cycle is the guarded one bit for bit
    spd = 'ua3d_sgs_scaling_m2'
    ref = kc.restatement(spd)
    t = []
    zt = ke.kr.KCycle(ref.h, ref.degree, 'K', trace=t).apply(kc.rhs(spd, 7))
    zu = ke.kr.KCycle(ref.h, ref.degree, 'K', guards=False).apply(kc.rhs(spd, 7))
    assert np.array_equal(zt, kc.reference(spd)[7]) and np.array_equal(zu, zt)
    assert all(d > 0 for _, _, d, _ in t)


@pytest.mark.parametrize('kind', ['nodal', 'scalar'])
def test_host_setup_accepts_what_the_oracle_accepts(lib_built, kind):
    """setup.cpp's pivot rule is the oracle's: the shifts of the cases build the
    oracle's levels, and the first refused shift (a non-positive pivot of the
    coarsest Gauss-Jordan) is refused by both"""
    M = _M()
    name = 'sgs_m3' if kind == 'nodal' else 'scalar_jacobi_m2'
    prm = ke.c_params(name)
    for sigma in sorted({c[1] for c in ke.INDEFINITE.values() if c[0] == kind}) + [ke.SIGMA_REFUSED]:
        A, _, idofs = ke.shifted(kind, sigma)
        assert A.diagonal().min() > 0.9
        try:
            h = mo.setup(A, ke.oracle_params(name), idofs=idofs)
        except np.linalg.LinAlgError as e:
            assert 'non-positive pivot' in str(e)
            h = None
        assert (h is None) == (sigma == ke.SIGMA_REFUSED)
        if h is None:
            with pytest.raises(M._lib.MamgError) as ei:
                M.HostHierarchy(A, idofs=idofs, **prm)
            assert ei.value.code == -3 and 'not SPD' in str(ei.value), str(ei.value)      # MAMG_ERR_SETUP
        else:
            H = M.HostHierarchy(A, idofs=idofs, **prm)
            assert [H.sizes(l)['n'] for l in range(H.num_levels)] == [lv.A.shape[0] for lv in h.levels]
            H.close()
