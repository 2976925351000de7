"""CPU checks of tests/grad_reference.py, the truth and the bounds tests/test_gpu_grad_truth.py holds the device to:

  1. the truths are right: at N = 12, d = 3 (r2 = 0 and a query 40 length scales out included) ``mean_gradient`` and
     ``variance_gradient`` agree with mpmath at 50 digits to the long-double route's own counted roundings (the fp64 bound's
     count with 2^-64 for 2^-53; the variance gradient, whose z is found through L, to cond(K) times the counted roundings of k* and of the two substitutions), and with central
     differences of ``ksr.kernel_sum`` / ``ksr.variance``'s formulas taken in extended precision with a step h of 1e-6 length
     scales, to the differences' own truncation order: h^2 max(1, r)^3 of the component's scale, r the query's largest distance
     from a training point (the third derivative of a radial profile grows as r^3 times the profile), plus, for the variance,
     the differences' own rounding 4 cond(K) 2^-64 / h;
  2. the bounds are attainable by honest fp64: the oracle's ``analytic_predict_grad`` and the device's formulation with an explicit
     W = L^-1 and sums in the kernels' order lie, per component, within ``mean_gradient_tolerance`` and
     ``variance_gradient_bound`` on every GPU case;
  3. the bounds are not slack: four planted defects leave them on every case (the dropped term in the strongest AND in the
     weakest coordinate of the ARD cases);
  4. the cases are what they claim to be: the ARD cases' weakest coordinate, the query kinds of every group of 16, and the
     GPU test's yardstick met by the explicit-W restatement without exception.
  5. the log-probability's gradient: ``log_prob_gradient`` agrees with central differences of its own value (the chain rule is
     right), lp_grad_eval's formulation in plain fp64 lies within ``log_prob_gradient_tolerance`` in every setting, and planted
     defects of the chain rule lie outside.
NOTES.md ("Gradient truth") records the printed figures."""
from functools import lru_cache

import numpy as np
import pytest

import grad_reference as gr
import kernel_sum_reference as ksr
import solve_reference as sr
from conftest import make_problem

LD = ksr.LD
CASE_FAMILIES = [(c, f) for c in gr.CASES for f in ksr.FAMILIES]


def _ids(v):
    return v.replace("Kernel", "") if isinstance(v, str) else str(v)


# ------------------------------------------------------------------------------------------------- 1. the truths are right
@lru_cache(maxsize=None)
def _small(family):
    rng = np.random.RandomState(3)
    N, d = 12, 3
    X = rng.uniform(-3.0, 3.0, (N, d))
    log_M = np.log(np.array([1.3, 2.0, 40.0]))
    amp, wn, inv_len = ksr.hyper_fp64(-0.3, -8.0, log_M)
    Q = rng.uniform(-3.0, 3.0, (6, d))
    Q[1] = X[4]                                                            # r2 = 0
    Q[2] = X[5] + 1e-3 / inv_len
    Q[3] = X[0]; Q[3, 0] = X[:, 0].max() + 40.0 / inv_len[0]               # 40 length scales out
    alpha = rng.randn(N) * 10.0 ** rng.uniform(-2, 2, N)
    la = gr.LOG_ALPHA[family]
    L = ksr.cholesky(ksr.kernel_matrix(X, amp, wn, inv_len, family, la))
    return X, Q, alpha, amp, wn, inv_len, la, L


@pytest.mark.parametrize("family", ksr.FAMILIES, ids=_ids)
def test_truths_agree_with_mpmath_at_50_digits(family):
    import mpmath as mp
    X, Q, alpha, amp, wn, inv_len, la, L = _small(family)
    ref, terms = gr.mean_gradient(X, alpha, amp, inv_len, Q, family, la)
    ref_mp, terms_mp = gr.mean_gradient(X, alpha, amp, inv_len, Q, family, la, mp_digits=50)
    scale = np.abs(terms_mp).sum(axis=1)
    # the long-double route's own roundings, counted as the fp64 bound counts them with 2^-64 in place of 2^-53
    N, d = X.shape
    w64 = LD(2.0) ** -64 * (32 + 2 * ksr.c_difference(d, family) * ksr.arg_difference(X, inv_len, Q, family, la).astype(LD))
    assert np.all(np.abs(terms - terms_mp) <= w64[:, :, None] * np.abs(terms_mp))
    assert np.all(np.abs(ref - ref_mp) <= (w64[:, :, None] * np.abs(terms_mp)).sum(axis=1) + LD(2.0) ** -64 * N * scale)
    assert np.all(ref[1] != 0) or family != "ExpSquaredKernel"             # on a training point the others still pull
    assert family != "ExpSquaredKernel" or np.all((np.abs(ref[3]) < LD(2.0) ** -1074) & (ref[3] != 0))   # 40 length scales out
    dv, vterms = gr.variance_gradient(L, X, amp, inv_len, Q, family, la)
    with mp.workdps(50):
        Lmp = ksr._cholesky_obj(ksr._kernel_matrix_mp(X, None, amp, wn, inv_len, family, la))
    dv_mp, vterms_mp = gr.variance_gradient(Lmp, X, amp, inv_len, Q, family, la, mp_digits=50)
    vscale = np.abs(vterms_mp).sum(axis=1)
    # the long-double route finds z by two substitutions of N + 2 roundings a row each, from a k* whose entries carry the
    # roundings counted above, all amplified by at most cond(K): per query, of the scale of its components
    cond = np.linalg.cond(ksr.kernel_matrix(X, amp, wn, inv_len, family, la).astype(np.float64))
    allow = cond * (2 * (N + 2) * 2.0 ** -64 + w64.max(axis=1).astype(np.float64))
    frac = np.max(np.abs(dv - dv_mp) / np.where(vscale > 0, vscale, 1), axis=1).astype(np.float64) / allow
    print("truth vs mpmath %s: dmu worst %.2e of scale, dvar worst %.2e of scale, %.3f of cond(K) = %.0f times the counted roundings" % (
        family, np.max(np.abs(ref - ref_mp) / np.where(scale > 0, scale, 1)),
        np.max(np.abs(dv - dv_mp) / np.where(vscale > 0, vscale, 1)), frac.max(), cond))
    assert np.all(frac <= 1.0)
    assert np.allclose(gr.radial_slope(np.array([0.0, 0.5, 7.0], dtype=LD), family, la).astype(np.float64),
                       gr.slope_fp64(np.array([0.0, 0.5, 7.0]), family, la), rtol=1e-14, atol=0)


@pytest.mark.parametrize("family", ksr.FAMILIES, ids=_ids)
def test_truths_agree_with_central_differences(family):
    """Step h = 1e-6 length scales in extended precision; agreement at the truncation order h^2 max(1, r)^3 (see below)."""
    if not ksr.EXTENDED:
        pytest.skip("the differences need the long double route")
    X, Q, alpha, amp, wn, inv_len, la, L = _small(family)
    if family == "Matern32Kernel":
        Q = np.delete(Q, 1, axis=0)                                        # its third derivative does not exist at r = 0
    ref, terms = gr.mean_gradient(X, alpha, amp, inv_len, Q, family, la)
    dv, vterms = gr.variance_gradient(L, X, amp, inv_len, Q, family, la)
    xs, qs = ksr.scaled(X, inv_len).astype(LD), ksr.scaled(Q, inv_len).astype(LD)
    w = np.asarray(alpha).astype(LD) * LD(amp)
    h = LD(1e-6)

    def value_and_variance(q):
        f = ksr._radial_ld(ksr._r2(q, xs, LD), family, la)
        V = ksr.forward_substitution(L, (LD(amp) * f).T)
        return (f * w[None, :]).sum(axis=1), LD(amp) - (V * V).sum(axis=0), np.abs(f * w[None, :]).sum(axis=1)

    # truncation of a central difference: h^2 |f'''| / 6, and the third derivative of a radial profile grows as r^3 times the
    # profile (squared exponential: (3 r - r^3) e^(-r^2 / 2)): h^2 max(1, r)^3 of the scale, r the query's largest distance.
    # The variance is a difference of numbers of size amp found through L: its differences carry 4 cond(K) 2^-64 / h besides.
    trunc = 1e-12 * np.maximum(1.0, np.sqrt(ksr._r2(qs.astype(np.float64), xs.astype(np.float64), np.float64)).max(axis=1)) ** 3
    rounding = 4.0 * np.linalg.cond(ksr.kernel_matrix(X, amp, wn, inv_len, family, la).astype(np.float64)) * 2.0 ** -64 / 1e-6
    worst_m = worst_v = 0.0
    for c in range(X.shape[1]):
        e = np.zeros(X.shape[1], dtype=LD); e[c] = h
        mp_, vp, sp = value_and_variance(qs + e)
        mm, vm, _ = value_and_variance(qs - e)
        fd_m = (mp_ - mm) / (2 * h) * LD(inv_len[c])
        fd_v = (vp - vm) / (2 * h) * LD(inv_len[c])
        sm = np.maximum(np.abs(terms[:, :, c]).sum(axis=1), sp * LD(inv_len[c]))
        sv = np.maximum(np.abs(vterms[:, :, c]).sum(axis=1), LD(amp) * LD(inv_len[c]))
        worst_m = max(worst_m, float(np.max(np.abs(fd_m - ref[:, c]) / sm / trunc)))
        worst_v = max(worst_v, float(np.max(np.abs(fd_v - dv[:, c]) / sv / (trunc + rounding))))
    print("truth vs central differences %s: dmu %.3f, dvar %.3f of the allowance" % (family, worst_m, worst_v))
    assert worst_m <= 1.0 and worst_v <= 1.0


# -------------------------------------------------------------------------------------------- 2.-4. on the GPU test's cases
@lru_cache(maxsize=None)
def _case(name, family):
    """The case, its truth, an fp64 factor with its explicit inverse, an fp64 alpha, the oracle's gradients and the two honest
    restatements -- once."""
    c = gr.case(name, make_problem)
    X, Q, h, y = c["X"], c["Q"], c["h"], c["y"]
    t = gr.truth(X, Q, h, family)
    dmu_o, dvar_o, alpha = gr.oracle_gradients(X, y, Q, h, family)
    Kf = sr.matrix_fp64(X, t["amp"], t["wn"], t["inv_len"], family, t["log_alpha"])
    W = sr.lower_inverse_fp64(np.linalg.cholesky(Kf))
    dmu_w, dvar_w = gr.device_form_fp64(X, alpha, t["amp"], t["inv_len"], Q, W, family, t["log_alpha"])
    ref, tol = gr.mean_truth(t, X, Q, alpha, family)
    return dict(c=c, t=t, alpha=alpha, W=W, dmu_o=dmu_o, dvar_o=dvar_o, dmu_w=dmu_w, dvar_w=dvar_w, dmu=ref, tol=tol)


def _mean_fraction(s, dmu):
    err = np.abs((np.asarray(dmu)[s["t"]["keep"]].astype(LD) - s["dmu"]).astype(np.float64))
    return err / s["tol"]


@pytest.mark.parametrize("name,family", CASE_FAMILIES, ids=_ids)
def test_honest_fp64_lies_within_the_bounds(name, family):
    s = _case(name, family)
    t = s["t"]
    assert np.all(np.isfinite(s["tol"])) and np.all(s["tol"] > 0) and np.all(np.isfinite(t["B"]))
    f_o, f_w = _mean_fraction(s, s["dmu_o"]), _mean_fraction(s, s["dmu_w"])
    e_ref, e_w, allowed, b_w = gr.yardstick(s["dvar_w"][t["keep"]], s["dvar_o"][t["keep"]], t)
    _, _, _, b_o = gr.yardstick(s["dvar_o"][t["keep"]], s["dvar_o"][t["keep"]], t)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.max(np.where(e_ref > 0, e_w / e_ref, 0.0))
    print("GRAD host %-11s %-24s dmu err/tol: oracle %.3f  explicit W %.3f | dvar err/B: oracle %.4f  explicit W %.4f | "
          "explicit W e/e_ref %.2f  e/allowed %.3f" % (name, family, f_o.max(), f_w.max(), b_o.max(), b_w.max(), ratio,
                                                       np.max(e_w / allowed)))
    assert np.all(f_o <= 1.0) and np.all(f_w <= 1.0)
    assert np.all(b_o <= 1.0) and np.all(b_w <= 1.0)
    # the GPU test's yardstick, met by the explicit-W restatement with no exception
    assert np.all(e_w <= allowed)


@pytest.mark.parametrize("name,family", CASE_FAMILIES, ids=_ids)
def test_planted_defects_leave_the_bounds(name, family):
    s = _case(name, family)
    c, t = s["c"], s["t"]
    X, Q, d, N = c["X"], c["Q"], c["d"], c["N"]
    _, terms = gr.mean_gradient(X, s["alpha"], t["amp"], t["inv_len"], Q[t["keep"]], family, t["log_alpha"], dks=t["dks"])
    # the dropped point: the one whose |term| is the median of a component -- of an in-box query's strongest coordinate
    m = int(t["keep"][0])
    comp = int(np.argmax(np.abs(s["dmu"][0]).astype(np.float64)))
    n_med = int(np.argsort(np.abs(terms[0, :, comp]).astype(np.float64))[N // 2])
    # f' off by a relative 1e-12 at every evaluation, each with the sign that moves the query's strongest component one way
    sign = np.ones((len(Q), N))
    strongest = np.argmax(np.abs(s["dmu"]).astype(np.float64), axis=1)
    sign[t["keep"]] = np.sign(np.take_along_axis(terms, strongest[:, None, None], axis=2)[:, :, 0].astype(np.float64))
    muts = [("drop", m, n_med, comp), ("slope", 1e-12, sign)]
    if d >= 3:                                          # ARD: the same defect in the coordinate whose gradient is weakest
        weak = int(np.argmin(np.max(np.abs(s["dmu"]).astype(np.float64), axis=0)))
        muts.append(("drop", m, int(np.argsort(np.abs(terms[0, :, weak]).astype(np.float64))[N // 2]), weak))
    if d > 1:
        muts.append(("inv_len", 0))
    if len(Q) > 1:
        muts.append(("stale_z",))
    for mut in muts:
        dmu, dvar = gr.device_form_fp64(X, s["alpha"], t["amp"], t["inv_len"], Q, s["W"], family, t["log_alpha"], mutate=mut)
        fm = _mean_fraction(s, dmu).max()
        e_ref, e_g, allowed, fb = gr.yardstick(dvar[t["keep"]], s["dvar_o"][t["keep"]], t)
        caught_v = bool(np.any(fb > 1.0) or np.any(e_g > allowed))
        what = mut[0] + ("" if mut[0] != "drop" else "@%d" % mut[3])
        print("GRAD mutation %-11s %-24s %-10s dmu err/tol %.3g | dvar err/B %.3g, e/allowed %.3g" % (
            name, family, what, fm, fb.max(), np.max(e_g / allowed)))
        if mut[0] != "stale_z":
            assert fm > 1.0, (name, family, mut[0])
        assert caught_v, (name, family, mut[0])


@pytest.mark.parametrize("name", list(gr.CASES))
def test_cases_are_what_they_claim(name):
    s = _case(name, "ExpSquaredKernel")
    c, t = s["c"], s["t"]
    kind, Q, X, inv_len = c["kind"], c["Q"], c["X"], c["inv_len"]
    assert len(Q) == gr.M_QUERIES == 37
    for lo, hi in ((0, 16), (16, 32), (32, 37)):
        assert set(kind[lo:hi]) == set(range(5))
    r = np.sqrt(ksr._r2(ksr.scaled(Q, inv_len), ksr.scaled(X, inv_len), np.float64))
    assert np.all(r[kind == 3].min(axis=1) == 0.0)
    assert np.all((r[kind == 1].min(axis=1) > 0) & (r[kind == 1].min(axis=1) <= 1e-3))
    assert np.all(r[kind == 4].min(axis=1) >= 40.0 * (1 - 1e-12))
    box = np.abs(Q - c["off"])
    assert np.all(box[kind == 0] <= 3.0) and np.all((box[kind == 2] >= 3.0) & (box[kind == 2] <= 4.5))
    if c["d"] >= 3:
        for family in ksr.FAMILIES:
            strength = np.max(np.abs(_case(name, family)["dmu"]).astype(np.float64), axis=0)
            print("GRAD ARD %-11s %-24s weakest / strongest coordinate of dmu: %.2e" % (name, family, strength.min() / strength.max()))
            assert strength.min() <= 1e-3 * strength.max()
    X0, Xa, ya = gr.append_sets(c)
    assert len(Xa) - len(X0) == 10 and all(n % 64 for n in range(len(X0), len(Xa)))


# ------------------------------------------------------------------------------------------- 5. the log-probability's gradient
@pytest.mark.parametrize("setting", gr.LP_SETTINGS)
@pytest.mark.parametrize("family", ksr.FAMILIES, ids=_ids)
def test_log_prob_gradient_is_the_gradient_of_its_value(family, setting):
    """Central differences of ``log_prob_gradient``'s own lp in the raw coordinates, step h = 1e-5 length scales.  The step is
    taken in fp64 inputs, so this checks the chain rule (a missing factor, a wrong sign, a prior on the wrong coordinate), not the
    last digits: truncation h^2 max(1, r)^3 = 1e-10 max(1, r)^3 of the scale -- times (1 + ln10 S)^2 under a y map, whose third
    derivative ln10 L (M''' + 3 ln10 M' M'' + ln10^2 M'^3) holds powers of the inner gradient, S = sum |terms| per length scale
    bounding M's derivatives -- and the inputs' rounding u |q| / h <= 1e-9."""
    X, Q, alpha, amp, wn, inv_len, la, L = _small(family)
    Q = np.delete(Q, [1, 3] if family == "Matern32Kernel" else [3], axis=0)   # not the far query; Matern-3/2 not at r = 0
    d = X.shape[1]
    ex = gr.lp_settings(dict(d=d, off=np.zeros(d)), setting)[1]
    kw = dict(affine=ex.get("affine", (1.0, 0.0)), ymap=ex.get("ymap"), prior=ex.get("prior"))
    mean = 0.3
    ref = gr.log_prob_gradient(X, alpha, amp, inv_len, Q, mean, family, la, **kw)
    chain = np.abs(ref["L"]).astype(np.float64) * np.log(10.0) if kw["ymap"] else np.ones(len(Q))
    r = np.sqrt(ksr._r2(ksr.scaled(Q, inv_len), ksr.scaled(X, inv_len), np.float64)).max(axis=1)
    worst = 0.0
    for c in range(d):
        h = 1e-5 / inv_len[c]
        e = np.zeros(d); e[c] = h
        up = gr.log_prob_gradient(X, alpha, amp, inv_len, Q + e, mean, family, la, **kw)["lp"]
        dn = gr.log_prob_gradient(X, alpha, amp, inv_len, Q - e, mean, family, la, **kw)["lp"]
        step = LD((Q + e)[:, c]) - LD((Q - e)[:, c])
        fd = ((up - dn) / step).astype(np.float64)
        scale = chain * np.abs(ref["gterms"][:, :, c]).sum(axis=1).astype(np.float64) + np.abs(ref["prior_grad"][:, c]).astype(np.float64)
        inner = np.log(10.0) * np.abs(ref["gterms"][:, :, c]).sum(axis=1).astype(np.float64) / inv_len[c] if kw["ymap"] else 0.0
        allow = (1e-10 * np.maximum(1.0, r) ** 3 * (1.0 + inner) ** 2 + 1e-9) * np.maximum(scale, 1e-300)
        worst = max(worst, float(np.max(np.abs(fd - ref["grad"][:, c].astype(np.float64)) / allow)))
    print("log_prob_gradient vs central differences %s %s: %.3f of the allowance" % (family, setting, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("setting", gr.LP_SETTINGS)
@pytest.mark.parametrize("family", ksr.FAMILIES, ids=_ids)
@pytest.mark.parametrize("name", gr.LP_CASES)
def test_log_prob_gradient_tolerance_is_attainable_and_not_slack(name, family, setting):
    """lp_grad_eval's formulation in plain fp64 (``log_prob_grad_fp64``) lies within the tolerance per component; planted defects
    of the chain rule lie outside on every case: f' off by a relative 1e-12, and per setting the scale folded into the value
    but not the gradient (affine), the y map's factor of the previous query (nlog, log), a prior mean of another coordinate."""
    s = _case(name, family)
    c, t = s["c"], s["t"]
    X, Q, h, N = c["X"], c["Q"], c["h"], c["N"]
    ex = gr.lp_settings(c, setting)[1]
    kw = dict(affine=ex.get("affine", (1.0, 0.0)), ymap=ex.get("ymap"), prior=ex.get("prior"))
    lpg, tol = gr.lp_truth(t, X, Q, s["alpha"], h["mean"], family, ex)
    assert np.all(np.isfinite(tol)) and np.all(tol > 0)

    def fraction(mutate=None):
        lp, g = gr.log_prob_grad_fp64(X, s["alpha"], t["amp"], t["inv_len"], Q, h["mean"], family, t["log_alpha"], mutate=mutate, **kw)
        return np.abs((g[t["keep"]].astype(LD) - lpg["grad"]).astype(np.float64)) / tol, lp

    honest, lp = fraction()
    lp_t = lpg["lp"].astype(np.float64)
    assert np.max(np.abs(lp[t["keep"]] - lp_t) / (1.0 + np.abs(lp_t))) < 1e-12
    sign = np.ones((len(Q), N))
    strongest = np.argmax(np.abs(lpg["dmu_a"]).astype(np.float64), axis=1)
    sign[t["keep"]] = np.sign(np.take_along_axis(lpg["gterms"], strongest[:, None, None], axis=2)[:, :, 0].astype(np.float64))
    muts = [("slope", 1e-12, sign)] + {"affine": [("no_fold",)], "nlog": [("stale_L",)], "log": [("stale_L",)],
                                       "prior": [("prior_swap",)]}.get(setting, [])
    worst = {m[0]: float(fraction(m)[0].max()) for m in muts}
    print("GRAD host lp %-8s %-24s %-8s honest err/tol %.3f | defects %s" % (
        name, family, setting, honest.max(), " ".join("%s %.3g" % kv for kv in worst.items())))
    assert np.all(honest <= 1.0)
    assert all(v > 1.0 for v in worst.values()), worst
