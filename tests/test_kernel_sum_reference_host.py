"""The extended-precision kernel-sum reference and its forward-error bound, checked on the host (tests/kernel_sum_reference.py).

  * the long-double sums agree with mpmath at 60 digits to 2^-8 of the bound (13 queries per case over the whole distance range);
  * plain fp64 NumPy restatements of the difference form and of the centred dot-product form stay inside the bound -- the bound
    is attainable by honest fp64 arithmetic (worst err/tol measured on this grid: 0.67 for either form, at the single-term case);
  * on the well-conditioned cases the bound is at least 1000 times tighter than the 1e-8 (|mu| + 1) it supplements;
  * a 1e-12 relative error in one term, or a dropped term that contributes less than 1e-8 of the sum, breaks it.
"""
import numpy as np
import pytest

import kernel_sum_reference as ksr
from conftest import make_problem

M_RAYS = 208


def _alpha_fp64(X, y, amp, wn, inv_len):
    """alpha of an fp64 solve: on the host any alpha will do, the solve is not under test."""
    xs = ksr.scaled(X, inv_len)
    r2 = ((xs[:, None, :] - xs[None, :, :]) ** 2).sum(-1)
    K = amp * np.exp(-0.5 * r2) + wn * np.eye(len(X))
    return np.linalg.solve(K, y)


def _case(name):
    """(X, alpha, amp, inv_len, well_conditioned) of the shared grid (GP mean 0 throughout)."""
    if name == "n1":
        X = np.array([[0.3, -1.1, 2.0]]); y = np.array([1.7])
        amp, wn, inv_len = ksr.hyper_fp64(0.3, -12.0, np.log([2.0, 1.5, 2.6]))
        return X, _alpha_fp64(X, y, amp, wn, inv_len), amp, inv_len, True
    if name == "lattice":
        amp, wn, inv_len = ksr.hyper_fp64(0.3, -12.0, np.log([2.0, 1.5, 2.6]))
        X, y = ksr.lattice(130, 3, 9.0, inv_len)
        return X, _alpha_fp64(X, y, amp, wn, inv_len), amp, inv_len, True
    N, d, log_wn, ell2 = {"p200x3": (200, 3, -12.0, None), "p130x10": (130, 10, -8.0, None), "p193x20": (193, 20, -12.0, None),
                          "ill200x3": (200, 3, -12.0, 8.0)}[name]
    X, y, h = make_problem(N, d, 11, log_wn=log_wn, ell2=ell2)
    amp, wn, inv_len = ksr.hyper_fp64(h["log_amp"], h["log_white_noise"], h["log_M"])
    return X, _alpha_fp64(X, y, amp, wn, inv_len), amp, inv_len, ell2 is None


CASES = ["n1", "lattice", "p200x3", "p130x10", "p193x20", "ill200x3"]


@pytest.fixture(scope="module")
def grid():
    out = {}
    for name in CASES:
        X, alpha, amp, inv_len, well = _case(name)
        Q = ksr.rays(X, inv_len, M_RAYS, seed=5)[::ksr.QUERY_STRIDE]
        ref, terms = ksr.kernel_sum(X, alpha, amp, inv_len, Q)
        out[name] = dict(X=X, alpha=alpha, amp=amp, inv_len=inv_len, well=well, Q=Q, ref=ref, terms=terms, d=X.shape[1])
    return out


@pytest.mark.parametrize("name", CASES)
def test_long_double_reference_against_mpmath(grid, name):
    g = grid[name]
    pick = np.unique(np.linspace(0, len(g["Q"]) - 1, 13).astype(int))
    ref_mp, _ = ksr.kernel_sum_mp(g["X"], g["alpha"], g["amp"], g["inv_len"], g["Q"][pick], digits=60)
    tol = ksr.tolerance(g["terms"][pick], ksr.arg_difference(g["X"], g["inv_len"], g["Q"][pick]), ksr.E_EXP_NEG_HALF,
                        ksr.c_difference(g["d"]), g["alpha"], g["amp"])
    gap = np.abs(g["ref"][pick] - ref_mp).astype(np.float64)
    S = np.abs(g["terms"][pick]).astype(np.float64).sum(1)
    print(name, "max gap / (u S) %.3g   max gap / tol %.3g" % (np.max(gap / np.maximum(ksr.U * S, 1e-320)), np.max(gap / tol)))
    assert np.all(gap <= tol * 2.0 ** -8)


@pytest.mark.parametrize("name", CASES)
def test_fp64_restatements_stay_inside_the_bound(grid, name):
    g = grid[name]
    X, alpha, amp, inv_len, Q, d = g["X"], g["alpha"], g["amp"], g["inv_len"], g["Q"], g["d"]
    ref = g["ref"]
    tol_d = ksr.tolerance(g["terms"], ksr.arg_difference(X, inv_len, Q), ksr.E_EXP_NEG_HALF, ksr.c_difference(d), alpha, amp)
    tol_c = ksr.tolerance(g["terms"], ksr.arg_dot(X, inv_len, Q), ksr.E_EXP_DIRECT, ksr.c_dot(d), alpha, amp)
    with np.errstate(under="ignore"):
        err_d = np.abs(ksr.difference_form_fp64(X, alpha, amp, inv_len, Q).astype(ksr.LD) - ref).astype(np.float64)
        err_c = np.abs(ksr.centred_dot_form_fp64(X, alpha, amp, inv_len, Q).astype(ksr.LD) - ref).astype(np.float64)
    print(name, "worst err/tol: difference %.3f  centred %.3f" % (np.max(err_d / tol_d), np.max(err_c / tol_c)))
    assert np.all(err_d <= tol_d)
    assert np.all(err_c <= tol_c)
    # the far queries: exactly zero, and finite
    assert np.all(ref[-3:] == 0)
    if g["well"]:
        # at least 1000 times tighter than 1e-8 (|mu| + 1) on nine queries in ten
        tight = tol_d <= 1e-11 * (np.abs(ref).astype(np.float64) + 1.0)
        print(name, "fraction with tol <= 1e-11 (|ref| + 1): %.3f" % tight.mean())
        assert tight.mean() >= 0.9
    # the grid reaches the denormal range and exact underflow, but not with more than a quarter of its queries
    below = np.abs(ref).astype(np.float64) < 2.0 ** -1022
    print(name, "fraction of queries below 2^-1022: %.3f" % below.mean())
    assert 0 < below.mean() <= 0.25


@pytest.mark.parametrize("name", ["n1", "lattice"])
def test_bound_catches_a_perturbed_and_a_dropped_term(grid, name):
    g = grid[name]
    terms, ref, d = g["terms"], g["ref"], g["d"]
    A = ksr.arg_difference(g["X"], g["inv_len"], g["Q"])
    tol = ksr.tolerance(terms, A, ksr.E_EXP_NEG_HALF, ksr.c_difference(d), g["alpha"], g["amp"])
    N = terms.shape[1]
    big = np.argmax(np.abs(terms), axis=1)
    rows = np.arange(len(ref))
    tbig = np.abs(terms[rows, big]).astype(np.float64)
    # Within 14 length scales of the dominant point (A <= 100, terms down to e^-100) the bound is at most
    # u (E + N - 1 + 100 c) sum|t| <= 7.1e-14 sum|t| here, and the dominant term is at least an eighth of sum|t| (the centre of
    # a lattice cell has eight equidistant neighbours): an error of 1e-12 of that term, >= 1.25e-13 sum|t|, must be caught.
    decidable = A[rows, big] <= 100.0
    assert decidable.mean() >= 0.3
    err = 1e-12 * tbig
    print(name, "perturbed term: min err/tol over %d decidable queries %.2f" % (decidable.sum(), np.min(err[decidable] / tol[decidable])))
    assert np.all(err[decidable] > tol[decidable]), "a 1e-12 relative error in one term passes the bound"
    if N > 1:
        # drop the largest term that contributes under 1e-8 of the sum: invisible to |dmu| / (|mu| + 1) <= 1e-8, not to this bound
        t = np.abs(terms).astype(np.float64)
        small = np.where(t < 1e-8 * np.abs(ref).astype(np.float64)[:, None], t, 0.0)
        drop = small.max(axis=1)
        cand = drop > 1e-12 * np.abs(ref).astype(np.float64)
        print(name, "queries with a droppable term in [1e-12, 1e-8) of the sum: %d" % cand.sum())
        assert cand.sum() >= 5
        assert np.all(drop[cand & decidable] > tol[cand & decidable]), "a dropped training point passes the bound"
        assert (cand & decidable).sum() >= 3
