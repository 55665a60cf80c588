"""A handle keeps the internal layout switches (mamg_set_option,
include/mamg_test.h) it was set up with: every setup call snapshots the
process-wide table once at its entry, and the layout builders, the first
apply (which builds the coarse-tail program) and the launch path read that
snapshot from the handle.  A switch set or reset afterwards, or while another
thread's setup runs, reaches only the handles set up after it."""
import os
import threading

import numpy as np
import pytest

import dist_csr_ref as dc
import mamg_oracle as mo
from conftest import set_opt

pytestmark = pytest.mark.gpu


def _M():
    import metric_amg_examples_amd as M
    return M


TAIL = {'MAMG_TAIL_RES': '0', 'MAMG_TAIL_LDS': '0', 'MAMG_TAIL_PROG_LDS': '1'}
TAIL_DEFAULT = {'MAMG_TAIL_RES': '1', 'MAMG_TAIL_LDS': '1', 'MAMG_TAIL_PROG_LDS': '0'}


def _pick(opts, keys):
    return {k: opts[k] for k in keys}


# n = 8 has two levels: the coarse level is the coarsest, which stays a
# launch, so the handle has no coarse tail and the three switches select
# nothing there; n = 16 has three levels and runs level 1 in the tail
@pytest.mark.parametrize('n', [8, 16])
def test_tail_switches_snapshot_at_setup_not_first_apply(lib_built, n):
    """The coarse-tail program is planned at a handle's first apply
    (tail_res_plan, tail_lds_plan, the program's place): it takes the switches
    of the handle's setup, not those set when the apply comes.  Each apply is
    bitwise that of a handle built and applied entirely under its settings
    (this test compares no variant with another or with a reference:
    tests/test_gpu_tail.py runs every tail switch against the oracle and the
    launch path and asserts the plan each one selects)."""
    M = _M()
    s = M.problems.bidomain(3, n, 1e6)
    A = s.scipy()
    r = mo.seeded_rhs(s.N)
    kw = dict(idofs=s.idofs, num_functions=2, smoother=11, Schwarz_type=7)   # SGS on the seed blocks

    def build_apply():
        B = M.MetricAMG(A, s.W, **kw)
        z = B * r
        B.close()
        return z
    for k, v in TAIL.items():
        set_opt(k, v)
    want1 = build_apply()                       # built and applied under the three set values
    B1 = M.MetricAMG(A, s.W, **kw)              # built under them, not applied yet
    for k in TAIL:
        set_opt(k, None)
    want2 = build_apply()                       # built and applied under the defaults
    B2 = M.MetricAMG(A, s.W, **kw)
    assert _pick(M._lib.resolved_options(), TAIL) == TAIL_DEFAULT
    z1, z2 = B1 * r, B2 * r                     # first applies: the tail programs are planned here
    assert _pick(B1.options(), TAIL) == TAIL
    assert _pick(B2.options(), TAIL) == TAIL_DEFAULT
    assert B1.num_levels == B2.num_levels == (2 if n == 8 else 3)
    B1.close()
    B2.close()
    assert np.array_equal(z1, want1)
    assert np.array_equal(z2, want2)


def test_upload_switches_stay_with_the_handle(lib_built):
    """MAMG_SELL_MIN_ROWS and MAMG_HALF choose level 0's formats at upload; a
    later setup under other values changes neither the first handle's formats
    nor its apply."""
    M = _M()
    s = M.problems.bidomain(2, 32, 1e4)
    A = s.scipy()
    r = mo.seeded_rhs(s.N)
    set_opt('MAMG_SELL_MIN_ROWS', '1')
    set_opt('MAMG_HALF', '0')
    B1 = M.MetricAMG(A, s.W, idofs=s.idofs, num_functions=2)
    f1 = B1.level_format(0)
    assert f1['sell'] and not f1['half']
    before = B1 * r
    set_opt('MAMG_SELL_MIN_ROWS', None)
    set_opt('MAMG_HALF', None)
    B2 = M.MetricAMG(A, s.W, idofs=s.idofs, num_functions=2)
    assert not B2.level_format(0)['sell']
    assert _pick(B2.options(), ('MAMG_SELL_MIN_ROWS', 'MAMG_HALF')) == {'MAMG_SELL_MIN_ROWS': str(1 << 20),
                                                                       'MAMG_HALF': '1'}
    assert _pick(B1.options(), ('MAMG_SELL_MIN_ROWS', 'MAMG_HALF')) == {'MAMG_SELL_MIN_ROWS': '1', 'MAMG_HALF': '0'}
    assert B1.level_format(0) == f1
    after = B1 * r
    B1.close()
    B2.close()
    assert np.array_equal(after, before)


class _PairExchange:
    """The host-staged exchange (DistMetricAMG.set_exchange) of two ranks that
    are threads of one process: one queue per direction.  Unlike the lockstep
    virtual_apply it does not need the two ranks' op lists to be alike."""

    def __init__(self, me, queues):
        self.me, self.q = me, queues

    def _swap(self, a, send=True, recv=True):
        if send:
            self.q[self.me].put(np.array(a))
        return self.q[1 - self.me].get(timeout=60) if recv else None

    def sendrecv(self, sends, recv_counts):
        got = self._swap(sends.get(1 - self.me), (1 - self.me) in sends, (1 - self.me) in recv_counts)
        return {} if got is None else {1 - self.me: got}

    def allreduce(self, a):
        return a + self._swap(a)


def test_two_ranks_set_up_in_threads_keep_their_own_switches(lib_built):
    """Two virtual ranks of one scalar hierarchy set up from two threads,
    MAMG_OVERLAP '0' when the first setup begins and reset while it runs:
    each rank keeps what its setup read (options() and the stream forks its
    apply issues), and the gathered apply is the one-GPU apply to 1e-12 (as
    test_gpu_dist_csr.py).  The main thread learns that rank 0's setup has
    read its switches from the setup's first progress line on stderr
    (print_level 2), which it waits for on a pipe.  The ranks then apply from
    two threads through the host-staged exchange: their op lists differ (one
    forks the interior rows, one does not), which the lockstep virtual_apply
    refuses."""
    import queue
    import torch
    M = _M()
    A, idofs, kw, _ = dc.case('bidomain2d')            # 2-D, n = 32
    r, _ = dc.oracle_apply('bidomain2d')
    B = M.MetricAMG(A, None, idofs=idofs, **kw)
    z1 = B * r
    B.close()
    queues = [queue.Queue(), queue.Queue()]
    hs, zs, errs = [None, None], [None, None], []

    def build(p, **more):
        try:
            hs[p] = M.DistMetricAMG(A, None, idofs=idofs, rank=p, nranks=2, comm_id=None, rep_nodes=1,
                                    exchange=_PairExchange(p, queues), **dict(kw, **more))
        except Exception as e:          # noqa: BLE001 -- reported below
            errs.append(repr(e))
        finally:
            if p == 0:
                os.write(2, b'[rank 0 built]\n')   # ends the wait below whatever happened

    def apply(p):
        try:
            x = torch.as_tensor(np.array(hs[p].local_slice(r), dtype=np.float64)).cuda()
            z = hs[p].apply_device(x, torch.full_like(x, float('nan')))
            torch.cuda.synchronize()
            zs[p] = z.cpu().numpy()
        except Exception as e:          # noqa: BLE001 -- reported below
            errs.append(repr(e))
    set_opt('MAMG_OVERLAP', '0')
    saved, (rd, wr) = os.dup(2), os.pipe()
    os.dup2(wr, 2)
    os.close(wr)
    try:
        t0 = threading.Thread(target=build, args=(0,), kwargs=dict(print_level=2))
        t0.start()
        seen = b''
        while b'rank 0' not in seen:                    # a progress line of rank 0's setup, or its end
            seen += os.read(rd, 4096)
    finally:
        os.dup2(saved, 2)
        os.close(saved)
        os.close(rd)
    set_opt('MAMG_OVERLAP', None)
    t1 = threading.Thread(target=build, args=(1,))
    t1.start()
    t0.join()
    t1.join()
    assert not errs, errs
    assert hs[0].options()['MAMG_OVERLAP'] == '0' and hs[1].options()['MAMG_OVERLAP'] == '1'
    assert [h.apply_launches['stream_forks'] for h in hs] == [0, 1]
    th = [threading.Thread(target=apply, args=(p,)) for p in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for h in hs:
        h.close()
    assert not errs, errs
    z = np.concatenate(zs)
    assert np.linalg.norm(z - z1) < 1e-12 * np.linalg.norm(z1)
