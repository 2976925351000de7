"""The reference of test_gpu_not_pd.py, checked on the CPU: on the oracle's matrix (OracleGP.get_matrix) the constructions of
notpd_numpy.py fail at pivot p + 1 under netlib's dpotf2 rule (potf2_info), the healthy matrices pass it, LAPACK's dpotrf agrees
wherever the failing pivot is finite, and construction (b) is exact: zeros and ones, not small and nearly-one numbers."""
import numpy as np
import pytest

from conftest import make_problem
from notpd_numpy import (dpotrf_info, healthy_factors, nonfinite_row, ones_block, ones_hyper, ones_pairs, positions,
                         potf2_info)

FAMILIES = [("ExpSquaredKernel", 1.0), ("Matern32Kernel", 1.0), ("Matern52Kernel", 1.0), ("RationalQuadraticKernel", 0.4)]
SIZES = [70, 130, 150, 705]


def _oracle(h, kernel, log_alpha, d=6):
    from oracle.gp_oracle import OracleGP
    return OracleGP(d, h["mean"], h["log_white_noise"], h["log_amp"], h["log_M"], kernel=kernel, log_alpha=log_alpha)


def _matrix(o, X):
    with np.errstate(invalid="ignore", over="ignore"):
        return o.get_matrix(X)


def test_rule_on_small_known_matrices():
    assert potf2_info(np.eye(5)) == 0
    assert potf2_info(np.array([[4.0, 2.0], [2.0, 1.0]])) == 2                 # singular: pivot 2 = 1 - 1 = 0
    assert potf2_info(np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0]])) == 2
    assert potf2_info(np.array([[1.0, 0.0], [0.0, np.nan]])) == 2
    assert potf2_info(np.array([[0.0]])) == 1
    A = np.random.RandomState(0).randn(40, 40)
    K = A @ A.T + 40 * np.eye(40)
    assert potf2_info(K) == 0 and dpotrf_info(K) == 0
    K[17, 17] = -1.0
    assert potf2_info(K) == 18 == dpotrf_info(K)


@pytest.mark.parametrize("kernel,log_alpha", FAMILIES)
@pytest.mark.parametrize("N", SIZES)
def test_healthy_matrix_passes(N, kernel, log_alpha):
    X, y, h = make_problem(N, 6, 70 + N)
    for hy in ((h,) if kernel == "RationalQuadraticKernel" else (h, ones_hyper(h))):
        K = _matrix(_oracle(hy, kernel, log_alpha), X)
        assert potf2_info(K) == 0 and dpotrf_info(K) == 0 and healthy_factors(K)


@pytest.mark.parametrize("kernel,log_alpha", FAMILIES)
@pytest.mark.parametrize("N", SIZES)
def test_nonfinite_row_fails_at_its_own_pivot(N, kernel, log_alpha):
    X, y, h = make_problem(N, 6, 70 + N)
    o = _oracle(h, kernel, log_alpha)
    pos = positions(N)
    for p in pos:
        K = _matrix(o, nonfinite_row(X, p, np.nan, coord=p % 6))
        assert np.all(np.isnan(K[p])) and np.all(np.isnan(K[:, p])) and np.all(np.isfinite(np.delete(np.delete(K, p, 0), p, 1)))
        assert potf2_info(K) == p + 1, (p, "nan")
    for p in (pos[0], pos[len(pos) // 2], pos[-1]):
        for v in (np.inf, -np.inf):
            K = _matrix(o, nonfinite_row(X, p, v, coord=(p + 1) % 6))
            assert np.isnan(K[p, p]) and np.all(np.isfinite(np.delete(np.delete(K, p, 0), p, 1)))
            assert potf2_info(K) == p + 1, (p, v)


@pytest.mark.parametrize("kernel", ["ExpSquaredKernel", "Matern32Kernel", "Matern52Kernel"])
@pytest.mark.parametrize("N", SIZES)
def test_ones_block_is_exact_and_fails_at_p(N, kernel):
    X, y, h = make_problem(N, 6, 70 + N)
    o = _oracle(ones_hyper(h), kernel, 1.0)
    for q, p in ones_pairs(N):
        K = _matrix(o, ones_block(X, q, p))
        rest = np.setdiff1d(np.arange(N), [q, p])
        assert np.all(K[np.ix_([q, p], rest)] == 0.0) and np.all(K[np.ix_(rest, [q, p])] == 0.0)      # exact zeros
        assert np.all(K[np.ix_([q, p], [q, p])] == 1.0)                                                # exact ones
        assert np.all(np.isfinite(K))
        assert potf2_info(K) == p + 1, (q, p)
        assert dpotrf_info(K) == p + 1, (q, p)                                                          # finite: LAPACK agrees
