"""What run_emcee and run_dynesty decide before any kernel runs: which part of the log-posterior the device evaluates and which
part is a host call, for combinations of likelihood, prior, theta scaler and y scaler.  Runs without a GPU: recording stubs
stand in for EnsembleSampler / GPUWalkBackend / HipGP and raise a sentinel, the model's GP is a placeholder.  Expected floats are
written in closed form from the fitted scalers' own attributes."""
from functools import partial

import numpy as np
import pytest
from sklearn.preprocessing import FunctionTransformer, MinMaxScaler, StandardScaler

import alabi_amd.core as core
import alabi_amd.dist as adist
import alabi_amd.nested as nested
from alabi_amd import utility as ut
from alabi_amd.posterior import _affine_map, _uniform_prior_box, _y_unscale_kind

BOUNDS = np.array([[-2.0, 3.0], [0.5, 1.5]])          # unequal sides
NARROW = np.array([[-1.0, 2.5], [0.75, 1.25]])        # a prior box inside BOUNDS
NORMAL = [(0.4, 0.7), (None, None)]                   # lnprior_normal data: a normal on coordinate 0 only
RANDOM_STATE = 1234
RTOL = 1e-11                                          # the tolerance _affine_map itself uses to call a map affine
POINTS = np.array([[-0.5, 0.9], [1.25, 1.1], [2.0, 0.8]])      # inside NARROW
CUBE = np.array([[0.1, 0.9], [0.5, 0.25], [0.7, 0.6]])


class _Stop(Exception):
    """Raised by the recording stubs: the front end has handed over every decision at that point."""


class _Fn:
    """A host callable that records the shape of every argument it receives."""

    def __init__(self, f):
        self.f, self.shapes = f, []

    def __call__(self, x):
        self.shapes.append(np.shape(x))
        return self.f(np.asarray(x, dtype=np.float64).reshape(-1))


def _lnlike(x):
    return -0.5 * float(np.sum(x ** 2)) - 1.0


def _lnprior(x):
    return -0.25 * float(np.sum((x - 0.5) ** 2))


class _PlaceholderGP:
    """Stands for a trained HipGP: only what surrogate_log_likelihood needs on the host."""

    def __init__(self):
        self.shapes = []

    def predict(self, y, x, return_var=False, return_cov=False):
        self.shapes.append(np.shape(x))
        return -np.sum(np.asarray(x) ** 2, axis=1)


class _StubHipGP:
    def __init__(self, ndim):
        self.ndim = ndim


THETA_SCALERS = {
    "identity": lambda: ut.no_scaler,
    "minmax": MinMaxScaler,
    "nonaffine": lambda: FunctionTransformer(func=np.arcsinh, inverse_func=np.sinh),
}
Y_SCALERS = {
    "identity": lambda: ut.no_scaler,
    "standard": StandardScaler,
    "nlog": lambda: ut.nlog_scaler,
    "log": lambda: ut.log_scaler,
    "other": lambda: FunctionTransformer(func=np.arcsinh, inverse_func=np.sinh),
}


def _model(tmp_path, tsc, ysc, with_gp=True):
    lnlike = _Fn(_lnlike)
    m = core.SurrogateModel(lnlike_fn=lnlike, bounds=BOUNDS, savedir=str(tmp_path), cache=False, verbose=False,
                            random_state=RANDOM_STATE)
    theta = np.random.RandomState(5).uniform(BOUNDS[:, 0], BOUNDS[:, 1], (12, 2))
    y = np.array([_lnlike(t) for t in theta])                  # all negative: nlog_scaler's domain
    if ysc == "log":
        y = -y
    m._theta, m._y = m.refit_scalers(theta, y, theta_scaler=THETA_SCALERS[tsc](), y_scaler=Y_SCALERS[ysc]())
    m.training_results = {"iteration": []}
    if with_gp:
        m.gp = _PlaceholderGP()
    return m


def _theta_map(m, tsc):
    """(mult, add) of the theta scaler in closed form from its fitted attributes."""
    if tsc == "minmax":
        lo, hi = m.theta_scaler.data_min_, m.theta_scaler.data_max_
        assert np.array_equal(lo, BOUNDS[:, 0]) and np.array_equal(hi, BOUNDS[:, 1])
        return 1.0 / (hi - lo), -lo / (hi - lo)
    return np.ones(2), np.zeros(2)


def _y_map(m, ysc):
    if ysc == "standard":
        return float(m.y_scaler.scale_[0]), float(m.y_scaler.mean_[0])
    return 1.0, 0.0


def _prior(kind):
    return {None: None,
            "uniform_kw": partial(ut.lnprior_uniform, bounds=NARROW),
            "uniform_pos": partial(ut.lnprior_uniform, NARROW),         # recognised by position; fused, so never called
            "normal_kw": partial(ut.lnprior_normal, bounds=NARROW, data=NORMAL),
            "normal_pos": partial(ut.lnprior_normal, NARROW, NORMAL),
            "lambda": _Fn(_lnprior)}[kind]


def _one(v):
    return float(np.asarray(v).reshape(-1)[0])


# ------------------------------------------------------------------------------------------------ run_emcee
# like, prior, theta scaler, y scaler -> coords ("scaled": walkers move in scaled theta, "theta": in theta itself), y
# ("device": the y un-scaling is folded into logp_affine, "host": it is not), logp_map, normal (fused normal prior), host callables
# ("prior", "like" row by row, "like_batch" the surrogate in one predict), gate_box (None: not passed), like_fn_name
EMCEE_ROWS = {
    "defaults":              (None, None, "identity", "identity", "scaled", "device", None, False, (), None, "surrogate"),
    "gp_uniform_kw":         ("gp", "uniform_kw", "minmax", "standard", "scaled", "device", None, False, (), None, "surrogate"),
    "uniform_pos":           (None, "uniform_pos", "minmax", "identity", "scaled", "device", None, False, (), None, "surrogate"),
    "normal_kw_fused":       (None, "normal_kw", "minmax", "standard", "scaled", "device", None, True, (), None, "surrogate"),
    "normal_pos_identity":   (None, "normal_pos", "identity", "identity", "scaled", "device", None, True, (), None, "surrogate"),
    "nlog":                  (None, None, "minmax", "nlog", "scaled", "device", "nlog", False, (), None, "surrogate"),
    "log":                   ("surrogate", None, "identity", "log", "scaled", "device", "log", False, (), None, "surrogate"),
    "normal_nlog_unit_mult": (None, "normal_kw", "identity", "nlog", "scaled", "device", "nlog", True, (), None, "surrogate"),
    # demotion: non-affine y map with t_mult != 1 under a normal prior -> the prior runs on the host
    "normal_nlog_minmax":    (None, "normal_kw", "minmax", "nlog", "scaled", "device", "nlog", False, ("prior",), False,
                              "surrogate"),
    "lambda_prior":          (None, "lambda", "minmax", "standard", "scaled", "device", None, False, ("prior",), False,
                              "surrogate"),
    "true":                  ("true", None, "minmax", "standard", "theta", "host", None, False, ("like",), True, "true"),
    "true_uniform_kw":       ("TRUE", "uniform_kw", "identity", "identity", "theta", "host", None, False, ("like",), True, "true"),
    "callable":              ("callable", None, "identity", "identity", "theta", "host", None, False, ("like",), True,
                              "likelihood"),
    "callable_lambda":       ("callable", "lambda", "minmax", "standard", "theta", "host", None, False, ("prior", "like"), False,
                              "likelihood"),
    # demotion: host likelihood together with a normal prior -> the prior runs on the host too
    "true_normal":           ("true", "normal_kw", "minmax", "standard", "theta", "host", None, False, ("prior", "like"), False,
                              "true"),
    # demotion: scalers that cannot be folded -> the surrogate is a host call on the whole batch
    "nonaffine_theta":       (None, None, "nonaffine", "standard", "theta", "host", None, False, ("like_batch",), True,
                              "surrogate"),
    "other_y":               (None, "uniform_kw", "minmax", "other", "theta", "host", None, False, ("like_batch",), True,
                              "surrogate"),
    "nonaffine_normal":      (None, "normal_kw", "nonaffine", "identity", "theta", "host", None, False,
                              ("prior", "like_batch"), False, "surrogate"),
}


def record_emcee(row, tmp_path, monkeypatch, with_gp=True, **kwargs):
    """Drive run_emcee up to the EnsembleSampler constructor; returns (model, recorded args, recorded kwargs, like, prior)."""
    like, prior_kind, tsc, ysc = row[:4]
    m = _model(tmp_path, tsc, ysc, with_gp=with_gp)
    rec = {}

    class Recorder:
        def __init__(self, *args, **kw):
            rec["args"], rec["kwargs"] = args, kw
            raise _Stop

    monkeypatch.setattr(core, "EnsembleSampler", Recorder)
    monkeypatch.setattr(core, "HipGP", _StubHipGP)
    like_fn = _Fn(_lnlike) if like == "callable" else like
    prior_fn = _prior(prior_kind)
    with pytest.raises(_Stop):
        m.run_emcee(like_fn=like_fn, prior_fn=prior_fn, nsteps=10, **kwargs)
    return m, rec["args"], rec["kwargs"], like_fn, prior_fn


@pytest.mark.parametrize("name", list(EMCEE_ROWS))
def test_run_emcee_plan(name, tmp_path, monkeypatch):
    row = EMCEE_ROWS[name]
    like, prior_kind, tsc, ysc, coords, y_where, logp_map, normal, host, gate_box, like_name = row
    m, args, kw, like_fn, prior_fn = record_emcee(row, tmp_path, monkeypatch)
    nwalkers, ndim, gp_obj, y_obj, box = args
    assert (nwalkers, ndim) == (20, 2) and gp_obj is m.gp and y_obj is m._y
    assert m.like_fn_name == like_name and m.nwalkers == 20 and m.nsteps == 10
    assert m.like_fn == {"surrogate": m.surrogate_log_likelihood, "true": m.true_log_likelihood}.get(like_name, like_fn)
    if prior_fn is None:
        assert m.prior_fn.func is ut.lnprior_uniform and np.array_equal(m.prior_fn.keywords["bounds"], BOUNDS)
        assert m.prior_fn_comment.startswith("Default uniform prior. \nPrior function: ut.prior_fn_uniform\n")
    else:
        assert m.prior_fn is prior_fn
    # the seed: the start-point draw comes first, the sampler seed second
    rs = np.random.RandomState(RANDOM_STATE)
    rs.randint(0, 2 ** 31 - 1)
    assert kw["seed"] == int(rs.randint(0, 2 ** 31 - 1))
    # sampler coordinates and the box in them
    t_mult, t_add = _theta_map(m, tsc) if coords == "scaled" else (np.ones(2), np.zeros(2))
    pbox = BOUNDS if prior_kind in (None, "lambda") else NARROW
    want_box = np.sort(pbox * t_mult[:, None] + t_add[:, None], axis=1)
    np.testing.assert_allclose(box, want_box, rtol=RTOL, atol=0)
    # y un-scaling and the fused normal prior
    scale, shift = _y_map(m, ysc) if y_where == "device" else (1.0, 0.0)
    if normal:
        if logp_map is None:
            shift += float(np.log(np.abs(t_mult[0])))          # sum(log|mult|) over the normal coordinates: coordinate 0
        mean, std = kw["normal_prior"]
        np.testing.assert_allclose(mean[0], NORMAL[0][0] * t_mult[0] + t_add[0], rtol=RTOL, atol=0)
        np.testing.assert_allclose(std[0], NORMAL[0][1] * abs(t_mult[0]), rtol=RTOL, atol=0)
        assert np.isnan(mean[1]) and np.isnan(std[1])
    else:
        assert kw["normal_prior"] is None
    np.testing.assert_allclose(kw["logp_affine"], (scale, shift), rtol=RTOL, atol=0)
    assert kw["logp_map"] == logp_map
    # host callables
    assert kw.get("gate_box") is gate_box
    assert (kw.get("prior_fn") is not None) == ("prior" in host)
    assert (kw.get("like_fn") is not None) == ("like" in host or "like_batch" in host)
    assert set(kw) == {"logp_affine", "normal_prior", "logp_map", "seed"} | ({"prior_fn", "like_fn", "gate_box"} if host else set())
    q = POINTS * t_mult + t_add
    if "prior" in host:
        want = np.array([_one(prior_fn(th.reshape(1, -1))) for th in POINTS])
        if isinstance(prior_fn, _Fn):
            prior_fn.shapes.clear()
        np.testing.assert_allclose(kw["prior_fn"](q), want, rtol=1e-9, atol=0)
        if isinstance(prior_fn, _Fn):
            assert prior_fn.shapes == [(1, 2)] * 3
    if "like" in host:
        fn = m.true_log_likelihood if like_name == "true" else like_fn
        want = np.array([_one(fn(th.reshape(1, -1))) for th in POINTS])
        fn.shapes.clear()
        assert np.array_equal(kw["like_fn"](q), want)
        assert fn.shapes == [(1, 2)] * 3
    if "like_batch" in host:
        want = m.surrogate_log_likelihood(POINTS)
        m.gp.shapes.clear()
        assert np.array_equal(kw["like_fn"](q), want)
        assert m.gp.shapes == [(3, 2)]


def test_run_emcee_true_before_any_gp(tmp_path, monkeypatch):
    m, args, kw, _, _ = record_emcee(EMCEE_ROWS["true"], tmp_path, monkeypatch, with_gp=False)
    assert isinstance(args[2], _StubHipGP) and args[2].ndim == 2
    assert np.array_equal(args[3], np.zeros(1))
    assert kw["like_fn"] is not None and kw["gate_box"] is True and m.like_fn_name == "true"


def test_run_emcee_opt_init_draws_before_the_sampler_seed(tmp_path, monkeypatch):
    m, args, kw, _, _ = record_emcee(EMCEE_ROWS["true"], tmp_path, monkeypatch, opt_init=True)
    rs = np.random.RandomState(RANDOM_STATE)
    rs.randint(0, 2 ** 31 - 1)                                 # find_map's candidate draw
    rs.standard_normal((20, 2))                                # ... and its ball around the MAP
    assert kw["seed"] == int(rs.randint(0, 2 ** 31 - 1))
    assert np.all(np.abs(m.map_theta - np.array([0.0, 0.5])) < 1e-3)       # arg-max of _lnlike in BOUNDS


def test_run_emcee_sampler_kwargs_seed_is_kept(tmp_path, monkeypatch):
    _, _, kw, _, _ = record_emcee(EMCEE_ROWS["defaults"], tmp_path, monkeypatch, sampler_kwargs={"seed": 99, "a": 1.5})
    assert kw["seed"] == 99 and kw["a"] == 1.5


def test_run_emcee_errors(tmp_path, monkeypatch):
    msg = "like_fn must be None, 'surrogate', 'gp', 'true' or a callable"
    for bad in ("bogus", "surrogate_log_likelihood", 3):
        with pytest.raises(ValueError) as e:
            _model(tmp_path, "identity", "identity").run_emcee(like_fn=bad)
        assert str(e.value) == msg
    for like in (None, "gp"):
        with pytest.raises(NameError) as e:
            _model(tmp_path, "identity", "identity", with_gp=False).run_emcee(like_fn=like)
        assert str(e.value) == "GP has not been trained"
    monkeypatch.setattr(adist, "world_info", lambda: (0, 2))
    for kwargs in (dict(like_fn="true"), dict(prior_fn=_Fn(_lnprior)), dict(like_fn=_Fn(_lnlike))):
        with pytest.raises(ValueError) as e:
            _model(tmp_path, "minmax", "standard").run_emcee(sampler_kwargs={"shard": True}, **kwargs)
        assert str(e.value) == ('sampler_kwargs={"shard": True} needs the fused log-probability (surrogate likelihood, shipped '
                                'priors and scalers); host callables run as replicas')


# ---------------------------------------------------------------------------------------------- run_dynesty
def _transform(kind):
    return {None: None,
            "uniform_kw": partial(ut.prior_transform_uniform, bounds=NARROW),
            "uniform_pos": partial(ut.prior_transform_uniform, NARROW),
            "lambda": _Fn(lambda u: NARROW[:, 0] + u ** 2 * (NARROW[:, 1] - NARROW[:, 0]))}[kind]


# like, prior transform, theta scaler, y scaler -> fused, logp_map, host likelihood (None, "rows", "batch"), like_fn_name
DYNESTY_ROWS = {
    "defaults":          (None, None, "identity", "identity", True, None, None, "surrogate"),
    "gp_uniform_kw":     ("gp", "uniform_kw", "minmax", "standard", True, None, None, "surrogate"),
    "bound_surrogate":   ("bound_surrogate", None, "minmax", "identity", True, None, None, "surrogate"),
    "nlog":              ("surrogate", None, "minmax", "nlog", True, "nlog", None, "surrogate"),
    "log":               (None, "uniform_kw", "identity", "log", True, "log", None, "surrogate"),
    "uniform_pos":       ("surrogate_log_likelihood", "uniform_pos", "minmax", "standard", False, None, "batch", "surrogate"),
    "lambda_transform":  (None, "lambda", "identity", "identity", False, None, "batch", "surrogate"),
    "nonaffine_theta":   (None, None, "nonaffine", "standard", False, None, "batch", "surrogate"),
    "other_y":           (None, "uniform_kw", "minmax", "other", False, None, "batch", "surrogate"),
    "true":              ("true", None, "minmax", "standard", False, None, "rows", "true"),
    "true_long_name":    ("true_log_likelihood", "uniform_kw", "identity", "identity", False, None, "rows", "true"),
    "bound_true":        ("bound_true", "lambda", "minmax", "standard", False, None, "rows", "true"),
    "callable":          ("callable", None, "identity", "standard", False, None, "rows", "custom"),
}


def record_dynesty(row, tmp_path, monkeypatch, with_gp=True, **kwargs):
    """Drive run_dynesty up to the GPUWalkBackend constructor; returns (model, args, kwargs, like, prior transform)."""
    like, pt_kind, tsc, ysc = row[:4]
    m = _model(tmp_path, tsc, ysc, with_gp=with_gp)
    rec = {}

    class Recorder:
        def __init__(self, *args, **kw):
            rec["args"], rec["kwargs"] = args, kw
            raise _Stop

    monkeypatch.setattr(nested, "GPUWalkBackend", Recorder)
    monkeypatch.setattr(core, "HipGP", _StubHipGP)
    like_fn = {"callable": _Fn(_lnlike), "bound_surrogate": m.surrogate_log_likelihood,
               "bound_true": m.true_log_likelihood}.get(like, like)
    pt = _transform(pt_kind)
    with pytest.raises(_Stop):
        m.run_dynesty(like_fn=like_fn, prior_transform=pt, **kwargs)
    return m, rec["args"], rec["kwargs"], like_fn, pt


@pytest.mark.parametrize("name", list(DYNESTY_ROWS))
def test_run_dynesty_plan(name, tmp_path, monkeypatch):
    row = DYNESTY_ROWS[name]
    like, pt_kind, tsc, ysc, fused, logp_map, host, like_name = row
    m, args, kw, like_fn, pt = record_dynesty(row, tmp_path, monkeypatch)
    gp_obj, y_obj, box = args
    assert gp_obj is m.gp and y_obj is m._y
    assert m.like_fn_name == like_name
    assert m.like_fn == {"surrogate": m.surrogate_log_likelihood, "true": m.true_log_likelihood}.get(like_name, like_fn)
    if pt is None:
        assert m.prior_transform.func is ut.prior_transform_uniform
        assert np.array_equal(m.prior_transform.keywords["bounds"], BOUNDS)
        assert m.prior_transform_comment.startswith("Default uniform prior transform. \nPrior function: ")
    else:
        assert m.prior_transform is pt
        assert m.prior_transform_comment.startswith("User defined prior transform.Prior function: ")
    assert set(kw) == {"seed", "to_theta", "logp_affine", "logp_map", "host_loglike"}
    assert kw["seed"] == int(np.random.RandomState(RANDOM_STATE).randint(0, 2 ** 31 - 1))     # one draw, rank 0
    assert kw["logp_map"] == logp_map
    assert (kw["host_loglike"] is None) == fused
    pbox = BOUNDS if pt_kind is None else NARROW
    if fused:
        t_mult, t_add = _theta_map(m, tsc)
        np.testing.assert_allclose(box, pbox * t_mult[:, None] + t_add[:, None], rtol=RTOL, atol=1e-300)
        np.testing.assert_allclose(kw["logp_affine"], _y_map(m, ysc), rtol=RTOL, atol=0)
        np.testing.assert_allclose(kw["to_theta"](CUBE), pbox[:, 0] + CUBE * (pbox[:, 1] - pbox[:, 0]), rtol=RTOL, atol=0)
        return
    assert np.array_equal(box, [[0.0, 1.0], [0.0, 1.0]]) and tuple(kw["logp_affine"]) == (1.0, 0.0)
    if pt_kind == "uniform_pos":             # binds the box to the transform's first parameter: handed on as it is, not callable
        return
    transform = m.prior_transform
    thetas = np.array([np.asarray(transform(u)) for u in CUBE])
    if isinstance(pt, _Fn):
        pt.shapes.clear()
    assert np.array_equal(kw["to_theta"](CUBE), thetas)
    if isinstance(pt, _Fn):
        assert pt.shapes == [(2,)] * 3
    if host == "batch":
        want = m.surrogate_log_likelihood(thetas)
        m.gp.shapes.clear()
        assert np.array_equal(kw["host_loglike"](CUBE), want)
        assert m.gp.shapes == [(3, 2)]
    else:
        fn = m.true_log_likelihood if like_name == "true" else like_fn
        want = np.array([_one(fn(th)) for th in thetas])
        fn.shapes.clear()
        assert np.array_equal(kw["host_loglike"](CUBE), want)
        assert fn.shapes == [(2,)] * 3


def test_run_dynesty_true_before_any_gp(tmp_path, monkeypatch):
    m, args, kw, _, _ = record_dynesty(DYNESTY_ROWS["true"], tmp_path, monkeypatch, with_gp=False)
    assert isinstance(args[0], _StubHipGP) and args[0].ndim == 2
    assert np.array_equal(args[1], np.zeros(1))
    assert kw["host_loglike"] is not None and m.like_fn_name == "true"


def test_run_dynesty_given_seed_draws_nothing(tmp_path, monkeypatch):
    m, _, kw, _, _ = record_dynesty(DYNESTY_ROWS["defaults"], tmp_path, monkeypatch, sampler_kwargs={"seed": 77})
    assert kw["seed"] == 77
    assert m._seed() == int(np.random.RandomState(RANDOM_STATE).randint(0, 2 ** 31 - 1))      # the model's stream is untouched


def test_run_dynesty_errors(tmp_path, monkeypatch):
    with pytest.raises(ValueError) as e:
        _model(tmp_path, "identity", "identity").run_dynesty(like_fn="bogus")
    assert str(e.value) == ("Unknown string identifier for like_fn: 'bogus'. "
                            "Valid options: 'surrogate', 'true', 'gp', 'surrogate_log_likelihood', 'true_log_likelihood'")
    with pytest.raises(TypeError) as e:
        _model(tmp_path, "identity", "identity").run_dynesty(like_fn=3)
    assert str(e.value) == "like_fn must be None, a string, or a callable function. Received type: <class 'int'>"
    for like in (None, "gp", "surrogate_log_likelihood"):
        with pytest.raises(NameError) as e:
            _model(tmp_path, "identity", "identity", with_gp=False).run_dynesty(like_fn=like)
        assert str(e.value) == "GP has not been trained"
    # run_dynesty has no sharded mode: the setting is refused whatever the likelihood, in a world of 2 as well
    monkeypatch.setattr(adist, "world_info", lambda: (0, 2))
    for like in (None, "true", _Fn(_lnlike)):
        with pytest.raises(TypeError) as e:
            _model(tmp_path, "minmax", "standard").run_dynesty(like_fn=like, sampler_kwargs={"shard": True})
        assert str(e.value) == "run_dynesty: unsupported sampler_kwargs ['shard']"


# ------------------------------------------------------------------------------------------- the moved helpers
def test_affine_map_and_y_unscale_kind(tmp_path):
    m = _model(tmp_path, "minmax", "standard")
    mult, add = _affine_map(m.theta_scaler.transform, BOUNDS)
    want_mult, want_add = _theta_map(m, "minmax")
    np.testing.assert_allclose(mult, want_mult, rtol=RTOL, atol=0)
    np.testing.assert_allclose(add, want_add, rtol=RTOL, atol=0)
    assert _affine_map(np.arcsinh, BOUNDS) is None
    assert _affine_map(lambda x: x, np.array([[1.0, 1.0]])) is None            # an empty side
    kind = _y_unscale_kind(m.y_scaler, m._y)
    assert kind[0] == "affine"
    np.testing.assert_allclose(kind[1:], _y_map(m, "standard"), rtol=RTOL, atol=0)
    for name in ("nlog", "log"):
        mm = _model(tmp_path, "identity", name)
        assert _y_unscale_kind(mm.y_scaler, mm._y) == (name,)
    mm = _model(tmp_path, "identity", "other")
    assert _y_unscale_kind(mm.y_scaler, mm._y) is None
    assert _uniform_prior_box(partial(ut.prior_transform_uniform, NARROW), 2) is None        # positional: not fused today


# ------------------------------------------------------------- the runs after the plan: seeds per run, attributes, files
class _FakeEnsemble:
    """Records its constructor arguments and returns a chain of 8 steps: enough for run_emcee's loop, records and files."""
    made = []

    def __init__(self, nwalkers, ndim, *args, **kw):
        self.nwalkers, self.ndim, self.kw, self.acceptance_fraction = nwalkers, ndim, kw, np.full(nwalkers, 0.25)
        _FakeEnsemble.made.append(self)

    def run_mcmc(self, p0, nsteps):
        self.p0 = np.array(p0)

    def get_chain(self, discard=0, thin=1, flat=False):
        chain = np.tile(self.p0, (8, 1, 1))[discard::thin]
        return chain.reshape(-1, self.ndim) if flat else chain

    def get_last_sample(self):
        return type("State", (), {"coords": self.p0 + 1.0})()

    def get_autocorr_time(self, tol=0):
        return np.full(self.ndim, 3.0)


def test_run_emcee_repeats_until_min_ess_and_writes(tmp_path, monkeypatch, capsys):
    m = _model(tmp_path, "minmax", "standard")
    m.cache, m.verbose = True, True
    _FakeEnsemble.made = []
    monkeypatch.setattr(core, "EnsembleSampler", _FakeEnsemble)
    monkeypatch.setattr(core.mcmc_utils, "estimate_burnin", lambda sampler, verbose=False: (2, 3))
    m.run_emcee(nsteps=8, min_ess=100)                         # 20 walkers x 2 kept steps = 40 samples per run: three runs
    rs = np.random.RandomState(RANDOM_STATE)
    draws = [int(rs.randint(0, 2 ** 31 - 1)) for _ in range(4)]            # start points, then one sampler seed per run
    assert [s.kw["seed"] for s in _FakeEnsemble.made] == draws[1:]
    first, second = _FakeEnsemble.made[:2]
    assert np.array_equal(second.p0, first.p0 + 1.0)           # a later run starts where the one before stopped
    t_mult, t_add = _theta_map(m, "minmax")
    assert m.emcee_samples.shape == (120, 2) and m.emcee_samples_gp is m.emcee_samples
    np.testing.assert_allclose(m.emcee_samples[:20], (first.p0 - t_add) / t_mult, rtol=RTOL, atol=1e-15)
    assert (m.iburn, m.ithin, m.burn, m.thin) == (2, 3, 2, 3) and m.acc_frac == 0.25 and m.autcorr_time == 3.0
    assert m.emcee_run and m.emcee_ranks == 1 and m.emcee_mode == "single" and m.emcee_sampler is _FakeEnsemble.made[-1]
    assert m.emcee_samples_full.shape == (8, 20, 2)
    assert np.array_equal(np.load(tmp_path / "emcee_samples_final_surrogate_iter_0.npz")["samples"], m.emcee_samples)
    assert (tmp_path / "surrogate_model.pkl").exists()
    out = capsys.readouterr().out
    assert "Run 1 complete: 40 samples (total 40)\n" in out and "Run 3 complete: 40 samples (total 120)\n" in out
    m.verbose = False
    m.run_emcee(like_fn="true", nsteps=8, min_ess=10 ** 6, burn=0, thin=1, samples_file="mine.npz")
    assert len(_FakeEnsemble.made) == 3 + 10 and m.emcee_samples.shape == (1600, 2) and m.emcee_samples_true is m.emcee_samples
    assert (m.iburn, m.ithin, m.burn, m.thin) == (2, 3, 0, 1)
    assert capsys.readouterr().out == "WARNING: Reached maximum of 10 runs, stopping with 1600 samples\n"
    assert (tmp_path / "mine.npz").exists()
    m.run_emcee(like_fn="true", nsteps=8, min_ess=0)
    assert (tmp_path / "emcee_samples_final_true.npz").exists() and m.like_fn_name == "true"


def test_run_dynesty_repeats_until_min_ess_and_writes(tmp_path, monkeypatch, capsys):
    made = []

    class Backend:
        path = "fused"

        def __init__(self, *args, seed, **kw):
            made.append(seed)

        def close(self):
            pass

    class Sampler:
        def __init__(self, backend, nlive, dynamic, walks, batch, seed):
            self.seed = seed

        def run_nested(self, checkpoint=None, **kw):
            n = len(made)
            return type("Res", (), {"logz": np.array([-3.0, -2.0 + (n == 2)]), "logzerr": np.array([0.5, 0.1 * n]),
                                    "samples_equal": lambda self, rng: np.full((30, 2), float(n))})()

    monkeypatch.setattr(nested, "GPUWalkBackend", Backend)
    monkeypatch.setattr(nested, "NestedSampler", Sampler)
    m = _model(tmp_path, "identity", "identity")
    m.cache, m.verbose = True, True
    m.run_dynesty(mode="static", min_ess=80)                   # 30 samples per run: three runs, one draw of the model's stream each
    rs = np.random.RandomState(RANDOM_STATE)
    assert made == [int(rs.randint(0, 2 ** 31 - 1)) for _ in range(3)]
    assert m.dynesty_samples.shape == (90, 2) and np.array_equal(m.dynesty_samples[::30, 0], [1.0, 2.0, 3.0])
    assert m.dynesty_logz == -1.0 and m.dynesty_logz_err == pytest.approx(0.3) and m.dynesty_path == "fused"
    assert m.dynesty_samples_surrogate is m.dynesty_samples and m.dynesty_run and m.dynesty_sampler.seed == made[-1]
    assert np.array_equal(np.load(tmp_path / "dynesty_samples_final_surrogate_iter_0.npz")["samples"], m.dynesty_samples)
    out = capsys.readouterr().out
    assert "Run 2 complete: 30 samples, logZ = -1.000\n" in out and f"Saved dynesty samples to {tmp_path}/dynesty_samples_final" in out
    del made[:]
    m.verbose = False
    m.run_dynesty(like_fn="true", mode="static", sampler_kwargs={"seed": 5}, min_ess=40, samples_file="mine.npz")
    assert made == [5, 5 + 1000003] and (tmp_path / "mine.npz").exists() and m.dynesty_samples_true is m.dynesty_samples
    m.run_dynesty(like_fn="true", mode="static", sampler_kwargs={"seed": 5}, min_ess=0)
    assert (tmp_path / "dynesty_samples_final_true.npz").exists()
