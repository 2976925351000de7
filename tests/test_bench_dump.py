"""bench.py --dump-outputs: file names, dtypes, the 64 MB budget and the seeded step sample (no GPU: CPU tensors)."""
import os

import numpy as np
import torch

import bench


def _sizes(d):
    return {f: os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_whole_chain(tmp_path):
    ch = torch.randn(64, 32, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    lp = torch.randn(64, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    bench.dump_outputs(str(tmp_path), ch, lp, ch[-1], lp[-1], np.full(32, 0.25))
    assert set(_sizes(tmp_path)) == {"chain.npy", "chain_log_prob.npy", "coords.npy", "log_prob.npy", "acceptance_fraction.npy"}
    for f in _sizes(tmp_path):
        assert np.load(tmp_path / f).dtype == np.float64
    assert np.array_equal(np.load(tmp_path / "chain.npy"), ch.numpy())
    assert np.array_equal(np.load(tmp_path / "chain_log_prob.npy"), lp.numpy())


def test_dump_large_chain_is_a_seeded_sample_within_budget(tmp_path):
    n, w, d = 4096, 256, 10                                   # 92 MB of chain + log-probabilities
    ch = torch.arange(n, dtype=torch.float64).reshape(n, 1, 1).expand(n, w, d).contiguous()
    lp = ch[:, :, 0].contiguous()
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), ch, lp, ch[-1], lp[-1], torch.zeros(w, dtype=torch.float64))
        assert sum(_sizes(tmp_path / sub).values()) <= bench.DUMP_LIMIT_BYTES
    steps = np.load(tmp_path / "a" / "chain_steps.npy")
    assert np.array_equal(steps, np.load(tmp_path / "b" / "chain_steps.npy"))
    assert len(steps) > n // 2 and np.all(np.diff(steps) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "chain.npy")[:, 0, 0], steps)
    assert np.array_equal(np.load(tmp_path / "a" / "chain_log_prob.npy")[:, 0], steps)
