"""CPU checks of leave-one-out cross-validation (gphip_loo / gphip_loo_grad): the symbols, argument validation that happens
before any device work, the numpy references the GPU tests compare against (tests/loo_reference.py) pinned to brute-force refits
and to finite differences, and the host logic of leaveOneOutFromGaussianProcess / selectHyperparameters / approximateEvidence
on a stub object whose closures are numpy."""
import ctypes
import math

import numpy as np
import pytest
from scipy.optimize import minimize

import loo_reference as ref
from bayesianinference_amd import _lib, build, gaussian_process as gp, laplace, synthetic as syn

NAMES = ("gphip_loo", "gphip_loo_grad")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_loo_symbols_are_declared_and_exported(lib):
    names = _lib.declared_symbols()
    for name in NAMES:
        assert name in names and name in _lib._SIGNATURES
        assert hasattr(lib, name)


def test_null_handle_and_null_arguments_are_rejected(lib):
    dp = ctypes.POINTER(ctypes.c_double)
    th = np.ones(4)
    out, info = ctypes.c_double(7.0), ctypes.c_int(-1)
    t = th.ctypes.data_as(dp)
    assert lib.gphip_loo(None, t, 4, None, None, None, ctypes.byref(out), ctypes.byref(info)) == 1
    assert lib.gphip_loo(None, None, 4, None, None, None, None, None) == 1
    assert lib.gphip_loo_grad(None, t, 4, ctypes.byref(out), t, ctypes.byref(info)) == 1
    assert lib.gphip_loo_grad(None, None, 4, None, None, None) == 1
    assert out.value == 7.0 and info.value == -1       # nothing written


def test_python_layer_rejects_a_theta_of_the_wrong_length_before_device_work(lib):
    h = object.__new__(_lib.Handle)                    # a Handle without a device handle behind it
    h._lib, h._h, h.d, h.N, h.p = lib, None, 2, 5, 4
    for call in (h.loo, h.loo_grad):
        with pytest.raises(_lib.GphipError) as e:
            call(np.ones(3))
        assert e.value.status == 2


def _theta(d):
    return np.concatenate([np.linspace(0.8, 1.3, d), [1.1, 0.15, 0.2]])      # l.., sf, sn (>= 0.1 sf), mu


@pytest.mark.parametrize("n", [60, 200])
def test_closed_form_reference_equals_brute_force_refits(n):
    """mu_-i = y_i - alpha_i / k_i, var_-i = 1 / k_i against N fresh Cholesky factorisations of the other N - 1 points."""
    X, y = syn.make_dataset(n, 3)
    th = _theta(3)
    a, b = ref.loo_closed_form("se_ard", th, X, y), ref.loo_brute_force("se_ard", th, X, y)
    em = np.abs(a["mean"] - b["mean"]).max() / np.abs(y).max()
    ev = np.abs(a["var"] / b["var"] - 1.0).max()
    print(f"n={n}: mean {em:.2e} (x max|y|), var {ev:.2e} relative, total {abs(a['total'] - b['total']):.2e}")
    assert em <= 1e-10 and ev <= 1e-10
    assert abs(a["total"] - b["total"]) <= 1e-10 * abs(b["total"])
    assert ref.device_total(a["logp"]) == pytest.approx(a["total"], rel=1e-13)


@pytest.mark.parametrize("n", [60, 150])
def test_gradient_reference_equals_central_differences(n):
    X, y = syn.make_dataset(n, 3)
    th = _theta(3)
    g = ref.loo_grad_formula("se_ard", th, X, y)
    fd = np.zeros_like(g)
    for j in range(len(th)):
        step = 1e-5 * max(abs(th[j]), 0.1)
        tp, tm = th.copy(), th.copy()
        tp[j] += step
        tm[j] -= step
        fd[j] = (ref.loo_closed_form("se_ard", tp, X, y)["total"] - ref.loo_closed_form("se_ard", tm, X, y)["total"]) / (2 * step)
    err = np.abs(g - fd).max() / np.abs(g).max()
    print(f"n={n}: formula vs central differences {err:.2e} of max |grad| = {np.abs(g).max():.3g}")
    assert err <= 1e-6


# ---- host logic on a stub: an inferenceObject whose closures are numpy -------------------------------------------------------
class _StubHandle:
    """loo(theta) from the numpy reference; theta with a negative entry 'does not factor' (info = 1)."""

    def __init__(self, X, y):
        self.X, self.y, self.calls = X, y, []

    def loo(self, theta, mean=True, var=True, logp=True):
        theta = np.asarray(theta, dtype=np.float64)
        self.calls.append(theta.copy())
        if np.any(theta <= 0):
            nan = np.full(len(self.y), np.nan)
            return {"mean": nan, "var": nan, "logp": nan, "total": float("nan"), "info": 1}
        r = ref.loo_closed_form("se_ard", theta, self.X, self.y, "zero")
        return {**r, "info": 0}


def _stub_object(normalize=False, samples=None):
    X, y = syn.make_dataset(40, 2)
    y = 3.0 * y + 5.0
    rules = {}
    Xn, yn = X, y
    if normalize:
        nd = gp.normalizeData(X, y[:, None])
        Xn, yn = nd["Input"]["NormalizedData"], nd["Output"]["NormalizedData"][:, 0]
        rules["DataPreProcessors"] = {k: {"Function": v["Function"], "InverseFunction": v["InverseFunction"]} for k, v in nd.items()}
    handle = _StubHandle(Xn, yn)

    def value_grad(theta):
        if np.any(np.asarray(theta) <= 0):
            return gp.MACHINE_LOG_ZERO, np.full(4, np.nan)
        return (ref.loo_closed_form("se_ard", theta, Xn, yn, "zero")["total"], ref.loo_grad_formula("se_ard", theta, Xn, yn, "zero"))

    assoc = {"Data": (Xn, yn[:, None]), "Parameters": [("l1", 0.1, 10.0), ("l2", 0.1, 10.0), ("sf", 0.1, 10.0), ("sn", 0.05, 2.0)],
             "GaussianProcessData": {"ModelFunctions": {"NuggetFunction": "sn^2", "MeanFunction": "zero"}, "HIPHandle": handle},
             "LogPseudoLikelihoodGradientFunction": value_grad, **rules}
    if samples is not None:
        assoc["Samples"] = samples
    return gp.inferenceObject(assoc), handle, (X, y)


def test_leave_one_out_for_one_theta_and_the_pre_processors():
    th = np.array([0.9, 1.2, 1.0, 0.2])
    obj, handle, _ = _stub_object()
    out = gp.leaveOneOutFromGaussianProcess(obj, th)
    assert set(out) == {"Mean", "StandardDeviation", "LogDensity", "LogPseudoLikelihood", "StandardizedResiduals"}
    want = ref.loo_closed_form("se_ard", th, handle.X, handle.y, "zero")
    np.testing.assert_allclose(out["Mean"], want["mean"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(out["StandardDeviation"], np.sqrt(want["var"]), rtol=1e-13)
    np.testing.assert_allclose(out["StandardizedResiduals"], (handle.y - want["mean"]) / np.sqrt(want["var"]), rtol=1e-12, atol=1e-12)
    assert out["LogPseudoLikelihood"] == pytest.approx(want["total"], rel=1e-13)
    # normalised data: moments back in the units of the data, the density with the Jacobian of the output scaling
    objn, hn, (X, y) = _stub_object(normalize=True)
    outn = gp.leaveOneOutFromGaussianProcess(objn, th)
    wn = ref.loo_closed_form("se_ard", th, hn.X, hn.y, "zero")
    sd_y = y.std(ddof=1)
    np.testing.assert_allclose(outn["Mean"], wn["mean"] * sd_y + y.mean(), rtol=1e-12)
    np.testing.assert_allclose(outn["StandardDeviation"], np.sqrt(wn["var"]) * sd_y, rtol=1e-12)
    np.testing.assert_allclose(outn["LogDensity"], wn["logp"] - math.log(sd_y), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(outn["StandardizedResiduals"], (y - outn["Mean"]) / outn["StandardDeviation"], rtol=1e-9, atol=1e-9)
    # a theta that does not factor: None, no exception; so for a failed object
    assert gp.leaveOneOutFromGaussianProcess(obj, np.array([0.9, -1.0, 1.0, 0.2])) is None
    assert gp.leaveOneOutFromGaussianProcess(gp.inferenceObject(None), th) is None
    assert gp.leaveOneOutFromGaussianProcess(obj) is None          # no "Samples"


def test_leave_one_out_posterior_mixture_weights():
    t1, t2, bad = np.array([0.9, 1.2, 1.0, 0.2]), np.array([1.4, 0.7, 1.3, 0.3]), np.array([1.0, 1.0, -1.0, 0.2])
    samples = [{"Point": t1, "CrudePosteriorWeight": 0.2}, {"Point": t2, "CrudePosteriorWeight": 0.5},
               {"Point": t1, "CrudePosteriorWeight": 0.1}, {"Point": bad, "CrudePosteriorWeight": 0.2}]
    obj, handle, _ = _stub_object(samples=samples)
    out = gp.leaveOneOutFromGaussianProcess(obj)
    assert len(handle.calls) == 3                                    # one evaluation per DISTINCT theta
    a, b = (ref.loo_closed_form("se_ard", t, handle.X, handle.y, "zero") for t in (t1, t2))
    w1, w2 = 0.3 / 0.8, 0.5 / 0.8                                    # the sample that does not factor carries no weight
    np.testing.assert_allclose(out["LogDensity"], np.log(w1 * np.exp(a["logp"]) + w2 * np.exp(b["logp"])), rtol=1e-12, atol=1e-12)
    mean = w1 * a["mean"] + w2 * b["mean"]
    np.testing.assert_allclose(out["Mean"], mean, rtol=1e-12, atol=1e-12)
    var = w1 * (a["var"] + a["mean"] ** 2) + w2 * (b["var"] + b["mean"] ** 2) - mean ** 2
    np.testing.assert_allclose(out["StandardDeviation"], np.sqrt(var), rtol=1e-10)
    assert out["LogPseudoLikelihood"] == pytest.approx(out["LogDensity"].sum())


def test_select_hyperparameters_on_the_stub():
    obj, handle, _ = _stub_object()
    start = np.array([0.9, 1.2, 1.0, 0.2])
    res = laplace.selectHyperparameters(obj, Criterion="LeaveOneOut", InitialGuess=start)
    assert set(res) == {"Maximum", "Criterion"} and res["Criterion"] == "LeaveOneOut"
    value, theta = res["Maximum"]
    v0, g0 = obj["LogPseudoLikelihoodGradientFunction"](start)
    v1, g1 = obj["LogPseudoLikelihoodGradientFunction"](theta)
    assert value == pytest.approx(v1, rel=1e-12) and v1 >= v0
    lo, hi = np.array([p[1] for p in obj["Parameters"]]), np.array([p[2] for p in obj["Parameters"]])
    free = (theta > lo) & (theta < hi)
    assert np.linalg.norm(g1[free]) <= 1e-3 * np.linalg.norm(g0)
    # no closure for the criterion -> None; the sentinel everywhere -> None, never an exception; an unknown criterion raises
    assert laplace.selectHyperparameters(obj, Criterion="MarginalLikelihood") is None
    wall = obj.append({"LogPseudoLikelihoodGradientFunction": lambda th: (gp.MACHINE_LOG_ZERO, np.full(4, np.nan))})
    assert laplace.selectHyperparameters(wall, Starts=2) is None
    with pytest.raises(ValueError):
        laplace.selectHyperparameters(obj, Criterion="Evidence")


def test_approximate_evidence_is_unchanged_by_the_refactoring():
    """The multi-start loop moved into a helper: the result on a stub must equal what the loop gave before, restated here."""
    A = np.array([[3.0, 0.5], [0.5, 2.0]])
    centre = np.array([1.5, 0.8])
    params = [("a", 0.2, 4.0), ("b", 0.1, 3.0)]

    def value_grad(theta):
        dlt = np.asarray(theta) - centre
        return -0.5 * dlt @ A @ dlt, -A @ dlt

    def logprior(theta):
        return -float(np.sum(np.log([p[2] - p[1] for p in params])))

    obj = gp.inferenceObject({"Parameters": params, "LogLikelihoodGradientFunction": value_grad, "LogPriorPDFFunction": logprior,
                              "LogLikelihoodFunction": lambda th: value_grad(th)[0]})
    got = laplace.approximateEvidence(obj, Starts=3, Seed=5)
    # the loop as it stood: `Starts` log-uniform starts from default_rng(Seed), L-BFGS-B on the box, the best finite minimum
    lo, hi = np.array([p[1] for p in params]), np.array([p[2] for p in params])

    def neg_post(theta):
        theta = np.clip(theta, lo, hi)
        ll, g = value_grad(theta)
        return -(ll + logprior(theta)), -(g + laplace._prior_grad(logprior, theta, lo, hi))

    rng = np.random.default_rng(5)
    starts = [np.exp(np.log(lo) + rng.random(2) * (np.log(hi) - np.log(lo))) for _ in range(3)]
    best = None
    for x0 in starts:
        res = minimize(neg_post, np.clip(x0, lo, hi), jac=True, method="L-BFGS-B", bounds=list(zip(lo, hi)))
        if math.isfinite(res.fun) and (best is None or res.fun < best.fun):
            best = res
    assert got["Maximum"][0] == -float(best.fun) and np.array_equal(got["Mean"], np.clip(best.x, lo, hi))
    np.testing.assert_allclose(got["Mean"], centre, atol=1e-5)
    np.testing.assert_allclose(got["PrecisionMatrix"], A, rtol=1e-5, atol=1e-6)
    want = got["Maximum"][0] + 0.5 * (2 * math.log(2 * math.pi) - np.linalg.slogdet(got["PrecisionMatrix"])[1])
    assert got["LogEvidence"] == pytest.approx(want, rel=1e-12)
    assert got["Parameters"] == ["a", "b"]
    single = laplace.approximateEvidence(obj, InitialGuess=[1.0, 1.0])
    np.testing.assert_allclose(single["Mean"], centre, atol=1e-5)
