"""Host side of nested sampling (alabi_amd/nested.py): the bookkeeping of NestedSampler with a NumPy walk backend defined here,
the integrals, merging, the scale rule, resampling, the run_dynesty signature, and the evidence of a 3-D correlated Gaussian."""
import inspect
import math
from functools import partial

import numpy as np
import pytest

from alabi_amd import nested as ns


class GaussianCubeBackend:
    """logL = log N(theta; mu, Sigma) with theta = lo + u (hi - lo); rwalk in NumPy (own generator)."""

    def __init__(self, mu, cov, lo, hi, seed=0):
        self.mu, self.cov = np.asarray(mu, float), np.asarray(cov, float)
        self.lo, self.hi = np.asarray(lo, float), np.asarray(hi, float)
        self.ndim = len(mu)
        self.prec = np.linalg.inv(self.cov)
        self.norm = -0.5 * (self.ndim * math.log(2 * math.pi) + np.linalg.slogdet(self.cov)[1])
        self.rng = np.random.default_rng(seed)

    def theta(self, u):
        return self.lo + np.asarray(u) * (self.hi - self.lo)

    def logl(self, u):
        r = self.theta(u) - self.mu
        return self.norm - 0.5 * np.einsum("ni,ij,nj->n", r, self.prec, r)

    def prior(self, call, n):
        u = self.rng.random((n, self.ndim))
        return u, self.logl(u)

    def walk(self, call, u0, logl0, lstar, chol, scale, walks):
        u, l = np.array(u0, float), np.array(logl0, float)
        nacc, nev = np.zeros(len(u), int), np.zeros(len(u), int)
        for _ in range(walks):
            up = u + scale * self.rng.standard_normal(u.shape) @ np.asarray(chol).T
            inside = np.all((up > 0) & (up < 1), axis=1)
            lp = np.full(len(u), -np.inf)
            lp[inside] = self.logl(up[inside])
            nev += inside
            ok = inside & (lp > lstar)
            u[ok], l[ok] = up[ok], lp[ok]
            nacc += ok
        return u, l, nacc, nev


def _problem(seed=0):
    A = np.array([[1.0, 0.6, 0.2], [0.6, 1.5, -0.4], [0.2, -0.4, 0.8]])
    mu = np.array([0.3, -0.5, 0.1])
    lo, hi = np.full(3, -6.0), np.full(3, 6.0)
    return GaussianCubeBackend(mu, A, lo, hi, seed), A, lo, hi


def _hand_trapezoid(logl, n):
    """Plain-float trapezoid rule with X_i = exp(-i / n), L_0 = 0, X_0 = 1."""
    Z, X_prev, L_prev, out = 0.0, 1.0, 0.0, []
    for i, li in enumerate(logl, start=1):
        X = math.exp(-i / n)
        w = 0.5 * (math.exp(li) + L_prev) * (X_prev - X)
        out.append(math.log(w))
        Z += w
        X_prev, L_prev = X, math.exp(li)
    return np.array(out), math.log(Z)


def test_k1_logvol_and_trapezoid_weights():
    rng = np.random.default_rng(1)
    n = 40
    logl = np.sort(rng.normal(-3.0, 2.0, 300))
    logvol, logwt, logz, _, _ = ns.compute_integrals(logl, np.full(300, n))
    assert np.allclose(logvol, -np.arange(1, 301) / n, rtol=0, atol=1e-12)
    lw_hand, lz_hand = _hand_trapezoid(logl, n)
    assert np.allclose(logwt, lw_hand, rtol=0, atol=1e-10)
    assert abs(logz[-1] - lz_hand) < 1e-10
    assert np.allclose(logz, np.logaddexp.accumulate(logwt), atol=1e-12)
    # the sampler with K = 1: every loop point is removed from n live points
    be, *_ = _problem(2)
    s = ns.NestedSampler(be, 30, batch=1, walks=10, seed=3)
    r = s.run_nested(dlogz=0.5)
    m = r.niter
    assert m > 0 and np.all(r.samples_n[:m] == 30)
    assert np.allclose(r.logvol[:m], -np.arange(1, m + 1) / 30, atol=1e-12)
    assert np.all(np.diff(r.logl) >= 0)


def test_batch_logvol_equals_sequential_removal():
    be, *_ = _problem(4)
    n, K = 40, 7
    s = ns.NestedSampler(be, n, batch=K, walks=10, seed=5)
    r = s.run_nested(dlogz=0.5)
    m = r.niter
    assert m % K == 0
    assert np.array_equal(r.samples_n[:m], np.tile(n - np.arange(K), m // K))
    seq = np.cumsum(-1.0 / (n - np.arange(K)))      # removing K points one by one from n
    assert np.allclose(r.logvol[K - 1:m:K], seq[-1] * np.arange(1, m // K + 1), atol=1e-11)
    assert np.allclose(r.logvol, -np.cumsum(1.0 / r.samples_n), atol=1e-12)


def test_add_live_tail():
    be, *_ = _problem(6)
    n = 25
    s = ns.NestedSampler(be, n, batch=5, walks=10, seed=7)
    r = s.run_nested(dlogz=1.0)
    tail = r.samples_n[r.niter:]
    assert np.array_equal(tail, n - np.arange(n))
    assert np.all(np.diff(r.logl[r.niter:]) >= 0)
    assert r.logl[r.niter] >= r.logl[r.niter - 1]


def test_merge_two_runs_sharing_a_start_equals_one_run():
    rng = np.random.default_rng(8)
    n1, n2, m1, m2 = 6, 9, 20, 30
    interior = np.sort(rng.uniform(-10, 0, m1 + m2))
    tail = np.sort(rng.uniform(0.5, 3, n1 + n2))
    pick1, pickt = rng.permutation(m1 + m2) < m1, rng.permutation(n1 + n2) < n1
    d = 2

    def run(li, lt, nl):
        logl = np.concatenate([li, lt])
        n = np.concatenate([np.full(len(li), nl), nl - np.arange(nl)])
        return ns._Run(rng.random((len(logl), d)), logl, n, -np.inf)
    r1 = run(interior[pick1], tail[pickt], n1)
    r2 = run(interior[~pick1], tail[~pickt], n2)
    u, logl, n = ns.merge_runs([r1, r2])
    n_tot = n1 + n2
    assert np.array_equal(logl, np.concatenate([interior, tail]))
    assert np.array_equal(n, np.concatenate([np.full(m1 + m2, n_tot), n_tot - np.arange(n_tot)]))
    # a batch run starting above L_lo adds its live count only above L_lo
    r3 = ns._Run(rng.random((3, d)), np.array([-5.0, -4.0, -3.0]), np.array([3, 2, 1]), -6.0)
    _, l3, n3 = ns.merge_runs([r1, r2, r3])
    assert interior.max() > -3.0
    full = np.concatenate([np.full(m1 + m2, n_tot), n_tot - np.arange(n_tot)])
    base = np.where(l3 <= interior.max(), n_tot, full[np.searchsorted(np.concatenate([interior, tail]), l3)])
    extra = np.select([l3 <= -6.0, l3 <= -5.0, l3 <= -4.0, l3 <= -3.0], [0, 3, 2, 1], 0)
    assert np.array_equal(n3, base + extra)


def test_logzerr_is_sqrt_h_over_n_for_constant_live_set():
    rng = np.random.default_rng(9)
    n = 50
    logl = np.sort(rng.normal(0, 3, 800))
    _, _, _, logzerr, h = ns.compute_integrals(logl, np.full(800, n))
    assert np.allclose(logzerr, np.sqrt(np.maximum(h, 0) / n), rtol=1e-9, atol=1e-12)


def test_scale_rule_pinned():
    assert ns.update_scale(1.0, 0.5, 3) == 1.0
    assert ns.update_scale(1.0, 0.8, 2) == pytest.approx(math.exp(0.3), rel=1e-15)
    assert ns.update_scale(0.7, 0.0, 4) == pytest.approx(0.7 * math.exp(-0.25), rel=1e-15)
    assert ns.update_scale(9.9, 1.0, 1) == 10.0 and ns.update_scale(1.5e-4, 0.0, 1) == 1e-4


def test_resample_equal_preserves_weights_in_expectation():
    w = np.array([0.05, 0.4, 0.1, 0.3, 0.15])
    x = np.arange(5)
    rng = np.random.default_rng(10)
    counts = np.zeros(5)
    reps = 4000
    for _ in range(reps):
        counts += np.bincount(ns.resample_equal(x, w, rng), minlength=5)
    assert np.allclose(counts / reps, w * 5, atol=0.02)
    # systematic: every draw count is floor or ceil of n w
    c = np.bincount(ns.resample_equal(x, w, rng), minlength=5)
    assert np.all(np.abs(c - 5 * w) < 1)


def test_unsupported_weight_kwargs_raise():
    be, *_ = _problem(11)
    s = ns.NestedSampler(be, 20, dynamic=True)
    with pytest.raises(NotImplementedError, match="pfrac"):
        s.run_nested(wt_kwargs={"pfrac": 0.8})
    with pytest.raises(NotImplementedError, match="pfrac"):
        s.run_nested(stop_kwargs={"pfrac": 1.0, "n_mc": 50})


def test_run_dynesty_signature_matches_reference():
    from alabi_amd import SurrogateModel
    sig = inspect.signature(SurrogateModel.run_dynesty)
    ref = ("(self, like_fn=None, prior_transform=None, mode='dynamic', sampler_kwargs={}, run_kwargs={}, multi_proc=False, "
           "save_iter=None, prior_transform_comment=None, samples_file=None, min_ess=10000)")
    assert str(sig) == ref


def test_unsupported_sample_method_raises(tmp_path):
    from alabi_amd import SurrogateModel
    sm = SurrogateModel(lnlike_fn=lambda t: -0.5 * float(np.sum(np.asarray(t) ** 2)), bounds=[(-1, 1), (-1, 1)],
                        savedir=str(tmp_path), verbose=False, random_state=0)
    with pytest.raises(NotImplementedError, match="random walk"):
        sm.run_dynesty(like_fn="true", sampler_kwargs={"sample": "slice"})


@pytest.mark.parametrize("dynamic", [False, True])
def test_evidence_of_correlated_gaussian_in_a_box(dynamic):
    be, A, lo, hi = _problem(12)
    s = ns.NestedSampler(be, 300, dynamic=dynamic, seed=13)
    r = s.run_nested(dlogz=0.1, n_effective=3000, maxbatch=3) if dynamic else s.run_nested(dlogz=0.1)
    logz_true = -np.sum(np.log(hi - lo))            # the Gaussian is normalised and lies well inside the box
    assert abs(r.logz[-1] - logz_true) < 3 * r.logzerr[-1], (r.logz[-1], logz_true, r.logzerr[-1])
    eq = r.samples_equal(np.random.default_rng(0))
    assert np.allclose(eq.mean(0), be.mu, atol=0.25)
    assert np.allclose(np.cov(eq.T), A, atol=0.35)
    assert r.status in (("converged",) if not dynamic else ("n_effective", "maxbatch"))
    assert r.eff > 0 and r.ncall >= r.niter


def test_uniform_prior_transform_partial_selects_the_fused_box():
    """run_dynesty samples the box of the tutorial's partial(prior_transform_uniform, bounds=B) on the fused path; any other
    prior transform (including prior_transform_uniform itself with bounds passed positionally) goes to the host."""
    from alabi_amd import utility as ut
    from alabi_amd.posterior import _uniform_prior_box
    B = np.array([[-2.0, 3.0], [0.5, 1.5]])
    box = _uniform_prior_box(partial(ut.prior_transform_uniform, bounds=B), 2)
    assert np.array_equal(box, B)
    u = np.array([0.25, 0.75])
    assert np.allclose(box[:, 0] + u * (box[:, 1] - box[:, 0]), ut.prior_transform_uniform(u, B))
    assert _uniform_prior_box(lambda u: B[:, 0] + u * (B[:, 1] - B[:, 0]), 2) is None
    assert _uniform_prior_box(partial(ut.prior_transform_uniform, B), 2) is None
    assert _uniform_prior_box(partial(ut.prior_sampler, bounds=B), 2) is None


@pytest.mark.parametrize("dynamic", [False, True])
def test_save_iter_checkpoint_fires_during_the_baseline_run(tmp_path, dynamic):
    """PickleCheckpoint (run_dynesty's save_iter) pickles the results so far while the first static loop is still running."""
    import pickle
    be, *_ = _problem(14)
    s = ns.NestedSampler(be, 60, dynamic=dynamic, walks=10, seed=15)
    path = str(tmp_path / "ck.pkl")
    seen = []
    ck = ns.PickleCheckpoint(s, path, 50)

    def spy(niter):
        before = len(seen)
        ck(niter)
        if ck.last == niter and niter > 0 and len(seen) == before:
            with open(path, "rb") as fh:
                seen.append((niter, len(s.runs), pickle.load(fh)))
    r = s.run_nested(dlogz=0.5, checkpoint=spy, n_effective=2000, maxbatch=2)
    assert seen and seen[0][1] == 0                     # the first pickle was written inside the baseline run
    niter0, _, snap = seen[0]
    assert snap["status"] == "running" and snap["niter"] == niter0 < r.niter
    assert len(snap["logl"]) == niter0 + 60 and np.array_equal(snap["samples_n"][niter0:], 60 - np.arange(60))
    assert np.all(np.diff(snap["logl"]) >= 0) and np.isfinite(snap["logz"][-1])
    ck.write(r)
    with open(path, "rb") as fh:
        assert pickle.load(fh)["niter"] == r.niter


def test_walk_covariance_uses_the_surviving_live_points(monkeypatch):
    rows = []
    real = ns._chol
    monkeypatch.setattr(ns, "_chol", lambda u: rows.append(len(u)) or real(u))
    be, *_ = _problem(16)
    ns.NestedSampler(be, 40, batch=8, walks=5, seed=17).run_nested(dlogz=1.0)
    assert rows and set(rows) == {32}
