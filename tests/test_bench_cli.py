"""bench.py's --dump-outputs writer (no GPU needed: it is handed a CPU tensor)."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('mamg_bench', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_small_vector_whole(tmp_path):
    import torch
    b = _bench()
    z = torch.linspace(-1.0, 1.0, 1001, dtype=torch.float64)
    b.dump_outputs(str(tmp_path / 'd'), z, 0, 1)
    a = np.load(tmp_path / 'd' / 'z.npy')
    assert a.dtype == np.float64 and np.array_equal(a, z.numpy())


def test_dump_outputs_sample_fixed_and_bounded(tmp_path, monkeypatch):
    """Above the cap: the same sorted seeded indices on every call, every rank
    its own file, the ranks together within the cap."""
    import torch
    b = _bench()
    monkeypatch.setattr(b, 'DUMP_MAX', 64)
    z = torch.arange(1000, dtype=torch.float64)
    for d in ('d1', 'd2'):
        b.dump_outputs(str(tmp_path / d), z, 0, 1)
    a1, a2 = (np.load(tmp_path / d / 'z.npy') for d in ('d1', 'd2'))
    assert a1.shape == (64,) and np.array_equal(a1, a2)
    assert np.all(np.diff(a1) >= 0) and a1.min() >= 0 and a1.max() < 1000      # z[i] = i: the indices
    for rank in (0, 1):
        b.dump_outputs(str(tmp_path / 'dd'), z, rank, 2)
    r0, r1 = (np.load(tmp_path / 'dd' / ('z_rank%d.npy' % k)) for k in (0, 1))
    assert r0.shape == r1.shape == (32,) and not np.array_equal(r0, r1)


def test_dump_cap_within_64_mb():
    assert _bench().DUMP_MAX * 8 <= 64 * 10**6
