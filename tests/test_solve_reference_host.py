"""The yardsticks of tests/solve_reference.py checked on the host, before any device is held to them.

  * the long-double truths (alpha, log-determinant, quadratic form, likelihood) agree with mpmath at 60 digits to 2^-8 of the
    first-order bound on the cases with N <= 65;
  * honest fp64 meets every criterion of tests/test_gpu_solve_truth.py on the whole case grid -- LAPACK's factor and cho_solve,
    blocked_solve_numpy in both modes, NumPy's reductions, the NumPy statement of the append -- which is the proof that the
    inputs are fair (MEASURED below);
  * every planted defect fails the new criterion while it passes the one that criterion supplements;
  * the append statement stays within its derived bound on every chain, and that bound is attained to within a factor 20;
  * every case is positive definite under LAPACK and under append_numpy.
"""
import math

import numpy as np
import pytest

import kernel_sum_reference as ksr
import solve_reference as sr
from conftest import make_problem

MEASURED = """
Worst over the grid (14 make_problem cases, 3 families, ill, clustered, big), this file's own output:
  LAPACK factor               worst |L L^T - K| / allowed            0.47   (clustered; 0.03 .. 0.43 elsewhere)
  LAPACK cho_solve            omega / u                              0.66 .. 6.9    (N = 1: 2.1 and 4.2)
  blocked_solve_numpy stream  omega / u                              0.66 .. 10.9     omega / (10 omega_ref + 16 u)  <= 0.13
  blocked_solve_numpy steps   omega / u                              0.66 .. 10.9     omega / (10 omega_ref + 16 u)  <= 0.13
  alpha, first-order bound    worst |a - a_true| / B_alpha           0.057  (LAPACK and both restatements)
  NumPy reductions            logdet, quad, nll error / tight bound  <= 0.03, <= 0.02, <= 0.09
  end to end                  logdet, nll error / first-order bound  <= 0.02, <= 0.01
  append_numpy, 63 rows       excess over the FRESH allowance        7.4 (n128d3)  0.29 (n128d10)  11.1 (n64d3)  5.8 (ill)  135 (clustered)
                              worst error / its own bound            0.31          0.83            0.30          0.12       0.20
The planted defects (factor: 48 of 48 first-column entries; alpha: largest and median component; block loss; dropped
log-determinant term; float product) all fail the new criteria; see the assertions for which of the old ones they pass.
"""

U = sr.U
ALL = sr.GRID + sr.FAMILY_CASES + ["ill", "clustered", "big"]
CHAINS = dict(sr.APPEND_CHAINS)
SMALL = [n for n in sr.GRID if int(n[1:].split("d")[0]) <= 65]
needs_extended = pytest.mark.skipif(not ksr.EXTENDED, reason="np.longdouble is a double here: the cases beyond N = 65 need the 64-bit significand")


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = sr.reference(sr.case(name, make_problem), CHAINS.get(name))
        return cache[name]
    return get


def _names(names):
    return [n if (ksr.EXTENDED or n in SMALL) else pytest.param(n, marks=needs_extended) for n in names]


@pytest.mark.parametrize("name", SMALL)
def test_long_double_truths_against_mpmath(refs, name, monkeypatch):
    import mpmath as mp
    monkeypatch.setattr(ksr, "MP_DIGITS", 60)
    ref = refs(name)
    with mp.workdps(60):
        K = ksr._kernel_matrix_mp(ref["X"], None, ref["amp"], ref["wn"], ref["inv_len"], ref["family"], ref["log_alpha"])
        t = sr.truths(ksr.cholesky(K), ref["r"])
        gap_a = np.array([abs(float(mp.mpf(float(a)) + mp.mpf(float(a - sr.LD(float(a)))) - b)) for a, b in zip(ref["alpha"], t["alpha"])])
        gaps = {k: abs(float(mp.mpf(float(ref[k])) + mp.mpf(float(ref[k] - sr.LD(float(ref[k])))) - t[k])) for k in ("logdet", "quad", "nll")}
    b_alpha, b_logdet, b_quad, b_nll = ref["fo"]
    print(name, "gap / first-order bound: alpha %.2e logdet %.2e quad %.2e nll %.2e" % (
        np.max(sr._ratio(gap_a, b_alpha)), gaps["logdet"] / b_logdet, gaps["quad"] / max(b_quad, 1e-300), gaps["nll"] / b_nll))
    assert np.all(gap_a <= b_alpha * 2.0 ** -8)
    assert gaps["logdet"] <= b_logdet * 2.0 ** -8 and gaps["quad"] <= b_quad * 2.0 ** -8 and gaps["nll"] <= b_nll * 2.0 ** -8


@pytest.mark.parametrize("name", _names(ALL))
def test_honest_fp64_meets_every_criterion(refs, name):
    ref = refs(name)                                     # raises where LAPACK or append_numpy finds a pivot that is not positive
    K, L, r, N = ref["K"], ref["L"], ref["r"], ref["N"]
    at = ref["alpha"].astype(np.float64)
    assert np.all(np.isfinite(ref["L_lapack"])) and ("L_app" not in ref or np.all(np.diagonal(ref["L_app"]) > 0))
    # LAPACK's factor within the allowance
    ex = float(np.max(sr.factor_excess(ref["L_lapack"], K, ref["allowed"])))
    floor = 10.0 * ref["omega_ref"] + 16.0 * U
    line = "%-30s LAPACK excess %.3f  omega/u: ref %.2f" % (name, ex, ref["omega_ref"] / U)
    assert ex <= 1.0
    assert ref["omega_ref"] <= sr.omega_first_order(N)
    b_alpha, b_logdet, b_quad, b_nll = ref["fo"]
    assert np.all(np.abs(ref["a_lapack"] - at) <= b_alpha)
    for mode in ("stream", "steps"):
        a = sr.blocked_solve_numpy(ref["L_lapack"], r, True, mode)
        om = sr.omega(K, L, a, r)
        line += "  %s %.2f (%.3f of the yardstick, alpha err/B %.3f)" % (mode, om / U, om / floor, np.max(sr._ratio(np.abs(a - at), b_alpha)))
        assert om <= floor and om <= sr.omega_first_order(N)
        assert np.all(np.abs(a - at) <= b_alpha)
    # the reductions in plain fp64 from LAPACK's factor and alpha: tight bounds given the inputs, first-order bounds end to end
    Ll, al = ref["L_lapack"], ref["a_lapack"]
    ld = 2.0 * float(np.sum(np.log(np.diagonal(Ll))))
    q = float(np.dot(r, al))
    nll = 0.5 * q + 0.5 * ld + 0.5 * N * math.log(2.0 * math.pi)
    e = (abs(float(ld - sr.logdet_given(Ll))) / sr.logdet_bound(Ll), abs(float(q - sr.quad_given(r, al))) / max(sr.quad_bound(r, al), 1e-300),
         abs(float(nll - sr.nll_given(Ll, r, al))) / sr.nll_bound(Ll, r, al))
    e2e = (abs(float(ld - ref["logdet"])) / b_logdet, abs(float(nll - ref["nll"])) / b_nll)
    print(line + "  reductions err/bound: logdet %.3f quad %.3f nll %.3f; end to end logdet %.4f nll %.4f" % (e + e2e))
    assert max(e) <= 1.0 and max(e2e) <= 1.0
    if N <= 200:
        W = sr.lower_inverse_fp64(Ll)
        print("%-30s inverse_omega/u of W^T W: %.2f" % (name, sr.inverse_omega(K, L, W.T @ W) / U))


FACTOR_DEFECT_CASES = ["n65d3", "n128d3", "n200d3", "ill", "clustered", "n65d10", "n128d10", "n200d10"]


@needs_extended
@pytest.mark.parametrize("name", FACTOR_DEFECT_CASES)
def test_planted_first_column_error_of_the_factor_is_caught(refs, name):
    """A relative error of 1e-13 in one entry of the first column of L: inside max |L L^T - K| <= 1e-12 max |K| (product in
    fp64, test_gpu_gp.py), outside the element-wise allowance."""
    ref = refs(name)
    caught = 0
    rows = np.unique(np.linspace(0, ref["N"] - 1, 6).astype(int))
    for i in rows:
        Ld = ref["L_lapack"].copy()
        Ld[i, 0] *= 1.0 + 1e-13
        assert np.max(np.abs(Ld @ Ld.T - ref["K64"])) <= 1e-12 * np.max(np.abs(ref["K64"]))
        caught += bool(np.max(sr.factor_excess(Ld, ref["K"], ref["allowed"])) > 1.0)
    print(name, "first-column entries caught: %d of %d" % (caught, len(rows)))
    assert caught == len(rows)


SOLVE_DEFECT_CASES = ["n65d3", "n128d3", "n129d3", "n200d3", "ill", "clustered", "n65d10", "n128d10", "n200d10"]


@needs_extended
@pytest.mark.parametrize("name", SOLVE_DEFECT_CASES)
def test_planted_alpha_errors_are_caught(refs, name):
    """1e-11 relative in the largest and in the median component of alpha, and a forward sweep that loses 1e-10 of one
    off-diagonal 64 x 64 block: inside |K a - r| <= 1e-8 max |r| (test_gpu_gp.py), outside 10 omega_ref + 16 u."""
    ref = refs(name)
    K, L, r, N = ref["K"], ref["L"], ref["r"], ref["N"]
    floor = 10.0 * ref["omega_ref"] + 16.0 * U
    order = np.argsort(np.abs(ref["a_lapack"]))
    bad = {}
    for tag, i in (("largest", order[-1]), ("median", order[N // 2])):
        a = ref["a_lapack"].copy()
        a[i] *= 1.0 + 1e-11
        bad[tag] = a
    if N > 64:
        nb = (N + 63) // 64
        bad["block (1, 0)"] = sr.blocked_solve_numpy(ref["L_lapack"], r, True, "stream", lose=(1, 0, 1e-10))
        bad["block (%d, %d)" % (nb - 1, nb - 2)] = sr.blocked_solve_numpy(ref["L_lapack"], r, True, "steps", lose=(nb - 1, nb - 2, 1e-10))
    for tag, a in bad.items():
        om = sr.omega(K, L, a, r)
        old = float(np.max(np.abs(ref["K64"] @ a - r)) / np.max(np.abs(r)))
        print("%-10s %-14s omega/u %.3g (yardstick %.3g)   |K a - r| / max|r| %.2e" % (name, tag, om / U, floor / U, old))
        assert old <= 1e-8
        assert om > floor


@needs_extended
@pytest.mark.parametrize("name", SOLVE_DEFECT_CASES)
def test_planted_reduction_errors_are_caught(refs, name):
    """A log-determinant that omits its smallest |log L_ii| term and a quadratic form with one product rounded to float (the
    largest, and the largest whose float rounding, at most 2^-24 of it, the likelihood's 1e-9 relative criterion cannot see):
    all outside the tight bounds given their inputs, and the second inside that 1e-9.  The largest product and the dropped
    term are 1e-8 and 1e-5 of their totals here, so 1e-9 would see them too: their relative size is printed, not asserted."""
    ref = refs(name)
    Ll, al, r, N = ref["L_lapack"], ref["a_lapack"], ref["r"], ref["N"]
    logs = np.log(np.diagonal(Ll))
    k = int(np.argmin(np.abs(logs)))
    ld_bad = 2.0 * float(np.sum(np.delete(logs, k)))
    err = abs(float(ld_bad - sr.logdet_given(Ll)))
    print(name, "dropped log term %.2e: err/bound %.3g, relative to logdet %.1e" % (abs(logs[k]), err / sr.logdet_bound(Ll), err / abs(float(ref["logdet"]))))
    assert err > sr.logdet_bound(Ll)
    nll = float(ref["nll"])
    order = np.argsort(np.abs(r * al))
    unseen = [j for j in order if abs(r[j] * al[j]) * 2.0 ** -24 <= 2e-9 * abs(nll)]
    for tag, j in (("largest", order[-1]), ("unseen", unseen[-1])):
        prod = r * al
        prod[j] = float(np.float32(prod[j]))
        err = abs(float(float(np.sum(prod)) - sr.quad_given(r, al)))
        print(name, "float product (%s): err/bound %.3g, 0.5 err relative to nll %.1e" % (tag, err / sr.quad_bound(r, al), 0.5 * err / abs(nll)))
        assert err > sr.quad_bound(r, al)
        if tag == "unseen":
            assert 0.5 * err <= 1e-9 * abs(nll)


@needs_extended
@pytest.mark.parametrize("name,n0", sr.APPEND_CHAINS)
def test_append_statement_within_its_bound_and_the_bound_attained(refs, name, n0):
    ref = refs(name)
    N, K = ref["N"], ref["K"]
    res = np.abs(sr.factor_residual(ref["L_app"], K))
    G = ref["G_numpy_substitution"]
    ratio = res / G
    fresh = res[n0:] / ref["allowed"][n0:]
    print("%-10s n0 = %d: appended rows: excess over the fresh allowance %.2f, worst error / append bound %.3f (generic form %.3f)" % (
        name, n0, fresh.max(), ratio[n0:].max(), (res / ref["G_numpy_generic"])[n0:].max()))
    assert np.all(res <= G)
    assert np.all(res <= ref["G_numpy_generic"])
    assert ratio[n0:].max() >= 1.0 / 20.0, "the bound exceeds the statement's actual error more than 20 times"
    # forward errors of the statement against a fresh LAPACK factorisation (the issue: within about 6 times)
    at = ref["alpha"].astype(np.float64)
    a_app = ref["W_app"].T @ (ref["W_app"] @ ref["r"])
    print("%-10s max |alpha - truth|: append %.2e, LAPACK %.2e; first-order bound ratio %.2e" % (
        name, np.max(np.abs(a_app - at)), np.max(np.abs(ref["a_lapack"] - at)), np.max(np.abs(a_app - at) / ref["fo_app"][0])))
    assert np.all(np.abs(a_app - at) <= ref["fo_app"][0])
    # planted: one row forms its l from a W with one entry off by 1e-10 relative (the entry with the largest share of that row's sum)
    for n in (n0, (n0 + N) // 2, N - 1):
        if n < 1:
            continue
        share = np.abs(ref["W_app"][:n, :n] * ref["K64"][:n, n][None, :])
        i, j = np.unravel_index(np.argmax(share), share.shape)
        Lp, _ = sr.append_numpy(ref["K64"], n0, plant=(n, i, j, 1e-10))
        resp = np.abs(sr.factor_residual(Lp, K))
        print("%-10s planted W[%d, %d] (1 + 1e-10) at row %d: worst error / bound %.3g" % (name, i, j, n, (resp / G).max()))
        assert np.any(resp > G)
