"""Vanek-Mandel-Brezina aggregation of the GPU setup on the device
(csrc/gsetup.hip, the vmb_* kernels).

The sequential loop's phase 1 is the lexicographically first maximal
independent set of the squared strong graph; the device reaches it by
worklist rounds whose count and work tests/vmb_ref.py restates.  So the
hierarchy is the host setup's bit for bit, the rounds and evaluations equal
the restatement's exactly, and the strong graph never travels to the host.
"""
import functools

import numpy as np
import pytest

import vmb_cases
import vmb_ref
from conftest import set_opt

pytestmark = pytest.mark.gpu


def _mamg():
    import metric_amg_examples_amd as M
    return M


@pytest.fixture(autouse=True)
def _vmb_default():
    yield
    _mamg()._lib.set_vmb(1, -1)


def hierarchies_equal(Hh, Hg):
    """tests/test_gpu_setup.py hierarchies_equal, restated"""
    assert Hh.num_levels == Hg.num_levels
    for l in range(Hh.num_levels):
        a, b = Hh.level(l, with_A=(l > 0)), Hg.level(l, with_A=(l > 0))
        assert a.keys() == b.keys(), (l, a.keys(), b.keys())
        for k in a:
            if k == 'n':
                assert a[k] == b[k]
                continue
            x, y = a[k], b[k]
            if isinstance(x, tuple):
                for u, v in zip(x[:3], y[:3]):
                    assert np.array_equal(u, v), (l, k)
                assert x[3] == y[3]
            else:
                assert np.array_equal(x, y), (l, k)


DEVICE = 2          # mamg_test_set_vmb mode: the device path whatever the level's size
NO_CAP = 1 << 40    # max_rounds that no level reaches


def gpu_hierarchy(name, mode=DEVICE, max_rounds=NO_CAP):
    """(hierarchy of the GPU setup, vmb_info of its levels until None);
    by default the device path on every level, however small, and no cap"""
    M = _mamg()
    A, idofs, kw = vmb_cases.system(name)
    M._lib.set_vmb(mode, max_rounds)
    Hg = M.HostHierarchy(A, idofs=idofs, gpu=True, **kw)
    infos = []
    while True:
        v = M._lib.vmb_info(len(infos))
        if v is None:
            break
        infos.append(v)
    return Hg, infos


@functools.lru_cache(maxsize=None)
def host_side(name):
    """The host setup's hierarchy and, per aggregated level, the restatement's
    result, the graph's entries, and the counts read off the host's agg."""
    M = _mamg()
    A, idofs, kw = vmb_cases.system(name)
    Hh = M.HostHierarchy(A, idofs=idofs, **kw)
    nf, theta, measure = Hh.params.num_functions, Hh.params.strong_coupled, Hh.params.strength_measure
    levels = []
    for l, Al, agg in vmb_cases.level_systems(Hh):
        S, W = vmb_ref.level_graph(Al, nf, theta, measure)
        r = vmb_ref.vmb_schedule(S, W)
        assert np.array_equal(r.agg, agg)
        # phase 1 of the sequential loop, to tell its members from the joiners
        agg1 = np.full(S.shape[0], -1)
        for i in np.flatnonzero(r.roots):
            agg1[i] = agg[i]
            agg1[S.indices[S.indptr[i]:S.indptr[i + 1]]] = agg[i]
        levels.append(dict(ref=r, entries=W.nnz, roots=int(agg.max()) + 1,
                           joiners=int(((agg >= 0) & (agg1 < 0)).sum())))
    return Hh, levels


@pytest.mark.parametrize('name', vmb_cases.NAMES)
def test_device_vmb_hierarchy_bitwise_and_schedule(lib_built, name):
    """The device path's hierarchy equals the host setup's in every level
    array; every aggregated level reports the device path, the restatement's
    rounds and evaluations exactly, the host agg's roots and joiners, and at
    most 64 + 32 * rounds bytes copied to the host."""
    Hh, levels = host_side(name)
    Hg, infos = gpu_hierarchy(name)
    hierarchies_equal(Hh, Hg)
    Hg.close()
    assert len(infos) == len(levels) > 0
    for l, (v, h) in enumerate(zip(infos, levels)):
        r = h['ref']
        print(name, 'level', l, v)
        assert v['path'] == 1, (l, v)
        assert (v['rounds'], v['evaluations']) == (r.rounds, r.evaluations), (l, v, r.rounds, r.evaluations)
        assert v['nonisolated'] == r.nonisolated
        assert v['roots'] == h['roots'] == r.nagg
        assert v['joiners'] == h['joiners'] == r.joiners
        assert v['host_bytes'] <= 64 + 32 * v['rounds'], (l, v)


@pytest.mark.parametrize('name', ['3d16_nodal_ua', '3d16_scalar_ua', 'rows_257'])
def test_host_path_by_request(lib_built, name):
    """mode 0: path 0 on every level, the strong graph downloaded (13 bytes
    per entry at least), the hierarchy bitwise the host's."""
    Hh, levels = host_side(name)
    Hg, infos = gpu_hierarchy(name, mode=0)
    hierarchies_equal(Hh, Hg)
    Hg.close()
    assert len(infos) == len(levels)
    for v, h in zip(infos, levels):
        assert v['path'] == 0 and v['rounds'] == 0
        assert v['host_bytes'] >= 13 * h['entries'], (v, h['entries'])


@pytest.mark.parametrize('name,abandons', [('3d16_nodal_ua', True), ('laplace1d_3000', True),
                                           ('permuted_2d24', False), ('rows_65', True)])
def test_round_cap_falls_back_to_the_host_path(lib_built, name, abandons):
    """max_rounds 3: a level that needs more rounds is abandoned after three
    and aggregated by the host path from scratch (path 2), the others stay on
    the device (the permuted system's level 0 needs exactly three: the cap
    itself is no reason to leave); the hierarchy is bitwise the host's."""
    Hh, levels = host_side(name)
    Hg, infos = gpu_hierarchy(name, max_rounds=3)
    hierarchies_equal(Hh, Hg)
    Hg.close()
    assert len(infos) == len(levels)
    assert any(h['ref'].rounds > 3 for h in levels) == abandons
    assert abandons or max(h['ref'].rounds for h in levels) == 3
    for l, (v, h) in enumerate(zip(infos, levels)):
        if h['ref'].rounds > 3:
            capped = vmb_ref.vmb_schedule(*_graph(name, l), max_rounds=3)
            assert v['path'] == 2 and v['rounds'] == 3 and v['evaluations'] == capped.evaluations, v
            assert v['host_bytes'] >= 13 * h['entries']
        else:
            assert v['path'] == 1 and v['rounds'] == h['ref'].rounds, v


def _graph(name, level):
    Hh, _ = host_side(name)
    l, Al, agg = vmb_cases.level_systems(Hh)[level]
    return vmb_ref.level_graph(Al, Hh.params.num_functions, Hh.params.strong_coupled, Hh.params.strength_measure)


@pytest.mark.parametrize('preset', ['standard_nodal', 'hazmath_pointwise'])
def test_handles_apply_bitwise_equal(lib_built, preset):
    """parameters_standard (nodal) and the hazmath point-wise preset: the
    handle of the GPU setup (VMB on the device) and the handle of the host
    setup apply identically on two seeded right-hand sides."""
    M = _mamg()
    P = M.parameters
    s = M.problems.bidomain(3, 16, 1e6 if preset == 'standard_nodal' else 1.0)
    A = s.scipy()
    out = {}
    M._lib.set_vmb(DEVICE, NO_CAP)
    for setup in ('gpu', 'host'):
        if preset == 'standard_nodal':
            B = M.metricAMG(A, s.W, idofs=s.idofs, parameters=P.parameters_standard, setup=setup)
        else:
            B = M.precond.get_hazmath_amg_precond(A, parameters=P.parameters_standard, pointwise=True, setup=setup)
        assert B.setup_path == setup and B.effective_params['aggregation_type'] == P.VMB
        if setup == 'gpu':
            v = M._lib.vmb_info(0)
            assert v is not None and v['path'] == 1 and v['host_bytes'] <= 64 + 32 * v['rounds'], v
        out[setup] = [B * M.problems.seeded_rhs(s.N, seed) for seed in (1234, 99)]
        B.close()
    for zg, zh in zip(out['gpu'], out['host']):
        assert np.isfinite(zg).all() and np.array_equal(zg, zh)


@pytest.mark.parametrize('poison', ['0', '1'])
def test_device_vmb_repeats(lib_built, poison):
    """Two device-path setups give equal agg, rounds and evaluations, also
    when new device arrays start as NaN bytes (nothing read before written)."""
    set_opt('MAMG_POISON', poison)
    runs = []
    for _ in range(2):
        Hg, infos = gpu_hierarchy('3d16_nodal_ua')
        aggs = [Hg.level(l, with_A=False)['agg'] for l in range(len(infos))]
        Hg.close()
        runs.append((aggs, [(v['path'], v['rounds'], v['evaluations'], v['roots'], v['joiners']) for v in infos]))
    assert runs[0][1] == runs[1][1] and all(p[0] == 1 for p in runs[0][1])
    for a, b in zip(runs[0][0], runs[1][0]):
        assert np.array_equal(a, b)
    Hh, levels = host_side('3d16_nodal_ua')
    assert [p[1] for p in runs[0][1]] == [h['ref'].rounds for h in levels]


@pytest.mark.parametrize('mode', [DEVICE, 0])
def test_unassigned_node_is_a_setup_error(lib_built, mode):
    """A stored zero opposite a nonzero mirror: row 29's only strong entry
    (flagged as the mirror of (28, 29)) has weight 0.0, which phase 2 skips,
    so node 29 joins nothing: MAMG_ERR_SETUP with the host path's message on
    either path."""
    M = _mamg()
    A = vmb_cases.unassignable()
    M._lib.set_vmb(mode, NO_CAP)
    for gpu in (True, False):
        with pytest.raises(M._lib.MamgError) as ei:
            M.HostHierarchy(A, gpu=gpu, num_functions=1, aggregation_type=vmb_cases.VMB, coarse_dof=10)
        assert ei.value.code == -3      # MAMG_ERR_SETUP
        assert 'VMB aggregation left a non-isolated node unassigned' in str(ei.value)


# the default mode's two decisions (gsetup.hip VMB_MIN_NODES, vmb_round_cap)
MIN_NODES = 1 << 17


def default_cap(entries):
    """rounds that cost what the host path would: 60 us a round, 5 ns an entry"""
    return max(1, int(entries * 5.0 / (1e3 * 60.0)))


@pytest.mark.parametrize('name', ['3d16_nodal_ua', '3d16_scalar_ua', 'rows_257'])
def test_default_mode_small_levels_take_the_host_path(lib_built, name):
    """Default mode: levels below the size threshold, where the rounds
    measured slower than the round trip, report path 3 and run no round; the
    hierarchy is bitwise the host's."""
    Hh, levels = host_side(name)
    Hg, infos = gpu_hierarchy(name, mode=1, max_rounds=-1)
    hierarchies_equal(Hh, Hg)
    Hg.close()
    assert len(infos) == len(levels)
    for v, h in zip(infos, levels):
        assert v['path'] == 3 and v['rounds'] == 0 and v['host_bytes'] >= 13 * h['entries'], v


@pytest.mark.parametrize('n', [MIN_NODES - 1, MIN_NODES])
def test_default_mode_threshold_and_cap_on_a_chain(lib_built, n):
    """laplace1d at the size threshold, default mode and cap.  One node
    below: the host path, untried (path 3).  At the threshold: the device is
    tried, the chain needs n / 3 rounds, and the level is abandoned at the
    default cap (path 2), the rounds that cost what the host path would.  The
    coarser levels are below the threshold.  Bitwise the host hierarchy."""
    import mamg_oracle as mo
    M = _mamg()
    A = mo.laplace1d(n)
    kw = dict(num_functions=1, aggregation_type=vmb_cases.VMB, AMG_type=vmb_cases.UA, max_levels=20)
    Hh = M.HostHierarchy(A, **kw)
    M._lib.set_vmb(1, -1)
    Hg = M.HostHierarchy(A, gpu=True, **kw)
    hierarchies_equal(Hh, Hg)
    v0, v1 = M._lib.vmb_info(0), M._lib.vmb_info(1)
    Hh.close()
    Hg.close()
    if n < MIN_NODES:
        assert v0['path'] == 3 and v0['rounds'] == 0, v0
    else:
        assert v0['path'] == 2 and v0['rounds'] == default_cap(A.nnz) < n // 3, v0
    assert v1['path'] == 3, v1
