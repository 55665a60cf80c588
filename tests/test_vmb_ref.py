"""The restatement of the GPU setup's VMB schedule (tests/vmb_ref.py) against
the sequential loop (oracle aggregate_vmb), on the CPU: the same aggregates
on every level of every system of tests/test_gpu_vmb.py, and work that stays
a small multiple of the node count whatever the round count."""
import numpy as np
import pytest

import mamg_oracle as mo
import vmb_cases
import vmb_ref


def _levels(name):
    """(l, S, Wabs, host agg) per aggregated level of the host hierarchy."""
    import metric_amg_examples_amd as M
    A, idofs, kw = vmb_cases.system(name)
    H = M.HostHierarchy(A, idofs=idofs, **kw)
    nf, theta, measure = H.params.num_functions, H.params.strong_coupled, H.params.strength_measure
    out = [(l, *vmb_ref.level_graph(Al, nf, theta, measure), agg) for l, Al, agg in vmb_cases.level_systems(H)]
    H.close()
    assert out, 'no aggregated level'
    return out


@pytest.mark.parametrize('name', vmb_cases.NAMES)
def test_restatement_equals_sequential_loop(lib_built, name):
    for l, S, W, hagg in _levels(name):
        agg, nagg = mo.aggregate_vmb(W, S, l)
        r = vmb_ref.vmb_schedule(S, W)
        assert r.nagg == nagg, (name, l)
        assert np.array_equal(r.agg, agg), (name, l)
        assert np.array_equal(r.agg, hagg), (name, l)
        # a schedule that degenerates into full sweeps evaluates every
        # undecided node every round: 7.7 to 69 per node on grids, not <= 4
        assert r.evaluations <= 4 * r.nonisolated, (name, l, r.evaluations, r.nonisolated, r.rounds)


def test_chain_takes_a_round_per_aggregate():
    """laplace1d in index order is one chain: aggregates of three nodes, one
    per round (the case behind the round cap)."""
    S = mo.strength(mo.laplace1d(300), 0.1)
    r = vmb_ref.vmb_schedule(S)
    assert r.nagg == 100 and r.rounds == 100 and r.evaluations <= 4 * 300


def test_work_per_node_does_not_grow_with_the_rounds():
    """2-D bidomain as a scalar system at theta 0.1: n = 128 takes four times
    the rounds of n = 32, and the evaluations per node stay within 1.1 x (a
    schedule whose work scales with the round count gives 4 x)."""
    per_node, rounds = {}, {}
    for n in (32, 128):
        A = mo.bidomain_system(2, n, 1.0)['A'].tocsr()
        S = mo.strength(A, 0.1)
        r = vmb_ref.vmb_schedule(S)
        assert r.nagg == mo.aggregate_vmb(abs(A), S, 0)[1]
        per_node[n], rounds[n] = r.evaluations / r.nonisolated, r.rounds
        print('2-D n=%d: rounds %d, evaluations per non-isolated node %.3f' % (n, r.rounds, per_node[n]))
    assert rounds[128] > 3 * rounds[32]
    assert per_node[128] <= 1.1 * per_node[32], per_node
    assert per_node[128] <= 4.0
