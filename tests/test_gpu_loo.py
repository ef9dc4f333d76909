"""Leave-one-out cross-validation on the device (gphip_loo / gphip_loo_grad) against the numpy references of
tests/loo_reference.py (pinned on the CPU by tests/test_loo.py).  Bars are the project's own for the same quantities: 1e-7 for
predicted means (x max |y|) and variances (x sf^2), 1e-8 relative for the scalar L_LOO, 1e-7 of max |grad| for gradients."""
import numpy as np
import pytest

import loo_reference as ref
from bayesianinference_amd import _lib, gaussian_process as gp, laplace, synthetic as syn

pytestmark = pytest.mark.gpu

SE_ARD_BODY = "T s = 0; for (int k = 0; k < D; ++k) { const T u = (X(k) - Y(k)) / P(k); s += u * u; } return P(D) * P(D) * exp((T)-0.5 * s);"
FIXED_TYPE_BODY = ("double s = 0; for (int k = 0; k < D; ++k) { const double u = (double)(X(k) - Y(k)) / (double)P(k); s += u * u; } "
                   "return (T)((double)P(D) * (double)P(D) * exp(-0.5 * s));")       # compiles as a value, not with dual numbers
SF = 1.1                                                          # sigma_f of every case below; sigma_n = 0.15 >= 0.1 sigma_f


def se_ard_fn(A, B, p):
    d = A.shape[-1]
    return p[d] ** 2 * np.exp(-0.5 * (((A - B) / p[:d]) ** 2).sum(-1))


def _kernel(name, d):
    return _lib.CustomKernel(SE_ARD_BODY, d + 1, fn=se_ard_fn) if name == "custom" else name


def _theta(name, d, mean):
    ell = list(np.linspace(0.8, 1.3, d))
    if name in ("se_ard", "matern52_ard", "matern32_ard", "custom"):
        th = ell + [SF, 0.15]
    elif name == "rq_ard":
        th = ell + [1.7, SF, 0.15]
    elif name == "se_ard*matern52_ard+const":
        th = ell + [SF] + [1.4 * v for v in ell] + [0.9, 0.3, 0.15]
    elif name == "null":
        th = [0.4]
    else:
        raise ValueError(name)
    return np.array(th + ([0.2] if mean == "const" else []))


def _check_values(res, want, y, label=""):
    em = np.abs(res["mean"] - want["mean"]).max() / np.abs(y).max()
    ev = np.abs(res["var"] - want["var"]).max() / SF ** 2
    el = np.abs(res["logp"] - want["logp"]).max()
    et = abs(res["total"] - want["total"]) / abs(want["total"])
    print(f"{label}: mean {em:.2e} var {ev:.2e} logp {el:.2e} total {et:.2e}")
    assert res["info"] == 0
    assert em <= 1e-7 and ev <= 1e-7 and et <= 1e-8
    assert el <= 1e-7 * max(1.0, np.abs(want["logp"]).max())
    assert res["total"] == ref.device_total(res["logp"])          # the documented summation order, exactly


# every kernel family at a ragged small N; every factorisation route for SE-ARD: single-launch dataflow (2048, 8192), the
# look-ahead schedule forced with the existing option (as scripts/gpu_large_fuzz.py does)
VALUE_CASES = [("se_ard", 333, 3, "const", None), ("se_ard", 333, 3, "zero", None), ("matern52_ard", 333, 3, "const", None),
               ("matern32_ard", 333, 3, "zero", None), ("rq_ard", 333, 3, "const", None),
               ("se_ard*matern52_ard+const", 333, 2, "const", None), ("custom", 333, 3, "const", None), ("null", 333, 2, "const", None),
               ("null", 333, 2, "zero", None), ("se_ard", 2048, 3, "const", None), ("se_ard", 8192, 3, "const", None),
               ("se_ard", 1500, 8, "const", {"dataflow": 0}), ("matern52_ard", 2048, 3, "zero", {"dataflow": 0, "lookahead": 1})]


@pytest.mark.parametrize("name,n,d,mean,opts", VALUE_CASES)
def test_loo_values_match_numpy(name, n, d, mean, opts):
    X, y = syn.make_dataset(n, d)
    kernel, th = _kernel(name, d), _theta(name, d, mean)
    h = _lib.Handle(X, y, kernel, mean)
    for k, v in (opts or {}).items():
        h.set_option(k, v)
    res = h.loo(th)
    _check_values(res, ref.loo_closed_form(kernel, th, X, y, mean), y, f"{name} n={n} {mean} {opts}")
    again = h.loo(th)                                             # bit-repeatable
    assert all(np.array_equal(res[k], again[k]) for k in ("mean", "var", "logp")) and res["total"] == again["total"]
    h.close()


def test_each_output_may_be_null():
    X, y = syn.make_dataset(500, 3)
    th = _theta("se_ard", 3, "const")
    h = _lib.Handle(X, y, "se_ard", "const")
    full = h.loo(th)
    for skip in ("mean", "var", "logp"):
        part = h.loo(th, **{skip: False})
        assert part[skip] is None and part["total"] == full["total"] and part["info"] == 0
        for k in ("mean", "var", "logp"):
            if k != skip:
                assert np.array_equal(part[k], full[k])
    none = h.loo(th, mean=False, var=False, logp=False)
    assert none["total"] == full["total"] == ref.device_total(full["logp"])
    h.close()


GRAD_CASES = [("se_ard", 333, 3, "const", None), ("se_ard", 333, 3, "zero", None), ("matern52_ard", 333, 3, "const", None),
              ("matern32_ard", 333, 3, "zero", None), ("rq_ard", 333, 3, "const", None), ("se_ard*matern52_ard+const", 333, 2, "const", None),
              ("custom", 333, 3, "const", None), ("null", 333, 2, "const", None), ("se_ard", 700, 8, "const", {"dataflow": 0}),
              ("se_ard", 1100, 3, "const", None)]


@pytest.mark.parametrize("name,n,d,mean,opts", GRAD_CASES)
def test_loo_gradient_matches_numpy(name, n, d, mean, opts):
    X, y = syn.make_dataset(n, d)
    kernel, th = _kernel(name, d), _theta(name, d, mean)
    h = _lib.Handle(X, y, kernel, mean)
    for k, v in (opts or {}).items():
        h.set_option(k, v)
    total, g, info = h.loo_grad(th)
    want = ref.loo_grad_formula(kernel, th, X, y, mean)
    err = np.abs(g - want).max() / np.abs(want).max()
    print(f"{name} n={n} {mean} {opts}: gradient {err:.2e} of max |grad| = {np.abs(want).max():.3g}")
    assert info == 0 and h.get_option("grad_analytic") == 1
    assert err <= 1e-7
    assert total == h.loo(th)["total"]
    t2, g2, _ = h.loo_grad(th)                                    # bit-repeatable
    assert t2 == total and np.array_equal(g, g2)
    h.close()


def test_custom_body_on_the_central_difference_route():
    """A body that dual numbers cannot differentiate, and option custom_grad = 0: central differences of gphip_loo with the step
    of gphip_loglik_grad.  Bar: that route's own for the likelihood gradient (tests/test_gpu_custom_kernel.py: 2e-5), here of
    max |grad| -- the step eps^(1/3) |theta| leaves a truncation error ~ h^2 = 4e-11 relative and a rounding error
    eps |L| / h ~ 1e-8, both far inside."""
    n, d = 400, 3
    X, y = syn.make_dataset(n, d)
    th = _theta("custom", d, "const")
    ok = _lib.Handle(X, y, _kernel("custom", d), "const")
    want = ref.loo_grad_formula(_kernel("custom", d), th, X, y, "const")
    t0, g0, _ = ok.loo_grad(th)
    assert ok.get_option("grad_analytic") == 1
    ok.set_option("custom_grad", 0)
    for h in (ok, _lib.Handle(X, y, _lib.CustomKernel(FIXED_TYPE_BODY, d + 1, fn=se_ard_fn), "const")):
        total, g, info = h.loo_grad(th)
        err = np.abs(g - want).max() / np.abs(want).max()
        print(f"difference route: {err:.2e}")
        assert info == 0 and h.get_option("grad_analytic") == 0
        assert err <= 2e-5
        assert total == pytest.approx(t0, rel=1e-12)
        mu, var = h.predict(X[:5])                                # the resident fit is theta's, not a stepped theta's
        h.fit(th)
        mu2, var2 = h.predict(X[:5])
        np.testing.assert_allclose(mu, mu2, rtol=0, atol=1e-12)
        h.close()


def test_no_side_effects_resident_fit_and_no_growth():
    n, d = 1500, 3
    X, y = syn.make_dataset(n, d)
    th, th2 = _theta("se_ard", d, "const"), _theta("se_ard", d, "const") * 1.1
    Xs = syn.make_test_points(50, d)
    h = _lib.Handle(X, y, "se_ard", "const")
    ll0 = h.loglik(th)
    lg0 = h.loglik_grad(th)
    assert h.fit(th) == 0
    p0 = h.predict(Xs)
    h.loo(th2)
    h.loo_grad(th2)
    assert h.loglik(th) == ll0
    lg1 = h.loglik_grad(th)
    assert lg1[0] == lg0[0] and np.array_equal(lg1[1], lg0[1])
    assert h.fit(th) == 0
    p1 = h.predict(Xs)
    assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1])
    # the calls leave the fit of THEIR theta resident: predict without gphip_fit
    for call in (h.loo, h.loo_grad):
        h.fit(th2)
        call(th)
        got = h.predict(Xs)
        np.testing.assert_allclose(got[0], p0[0], rtol=0, atol=1e-10 * np.abs(y).max())
        np.testing.assert_allclose(got[1], p0[1], rtol=0, atol=1e-10)
        a = h.solve(y)
        assert np.all(np.isfinite(a))
    mean_c, cov_c = h.predict_cov(Xs[:8])
    np.testing.assert_allclose(mean_c, p0[0][:8], rtol=0, atol=1e-10)
    before = h.factor_bytes()
    for _ in range(25):
        h.loo(th)
        h.loo_grad(th)
    assert h.factor_bytes() == before
    h.close()


def test_agrees_with_predictions_from_the_other_points():
    """The definition, through the library itself: mu_-i, var_-i = gphip_predict at x_i from a handle on the other N - 1."""
    n, d = 300, 3
    X, y = syn.make_dataset(n, d)
    th = _theta("matern52_ard", d, "const")
    h = _lib.Handle(X, y, "matern52_ard", "const")
    res = h.loo(th)
    h.close()
    for i in (0, 1, 17, 63, 64, 127, 128, 200, 255, 299):
        keep = np.arange(n) != i
        o = _lib.Handle(X[keep], y[keep], "matern52_ard", "const")
        assert o.fit(th) == 0
        mu, var = o.predict(X[i:i + 1])
        o.close()
        assert abs(mu[0] - res["mean"][i]) <= 1e-7 * np.abs(y).max()
        assert abs(var[0] - res["var"][i]) <= 1e-7 * SF ** 2


def test_failure_modes():
    n, d = 400, 3
    X, y = syn.make_dataset(n, d)
    th = _theta("se_ard", d, "const")
    h = _lib.Handle(X, y, "se_ard", "const")
    bad = th.copy()
    bad[1] = np.nan
    res = h.loo(bad)
    assert res["info"] == _lib.INFO_NAN
    assert np.isnan(res["total"]) and np.all(np.isnan(res["mean"]))
    total, g, info = h.loo_grad(bad)
    assert info == _lib.INFO_NAN and np.all(np.isnan(g))
    with pytest.raises(_lib.GphipError) as e:
        h.loo(th[:-1])
    assert e.value.status == 2
    h.close()
    Xd = X.copy()
    Xd[5] = Xd[9]                                                 # duplicated inputs, no nugget: singular K
    sing = th.copy()
    sing[d + 1] = 0.0
    hd = _lib.Handle(Xd, y, "se_ard", "const")
    res = hd.loo(sing)
    assert res["info"] == _lib.INFO_NOT_SPD and np.isnan(res["total"])
    assert all(np.all(np.isnan(res[k])) for k in ("mean", "var", "logp"))
    total, g, info = hd.loo_grad(sing)
    assert info == _lib.INFO_NOT_SPD and np.isnan(total) and np.all(np.isnan(g))
    assert hd.loo(th)["info"] == 0                                # the handle stays usable
    hd.close()


def test_two_virtual_ranks_factor_on_the_first_device():
    n, d = 1500, 3
    X, y = syn.make_dataset(n, d)
    th = _theta("se_ard", d, "const")
    g = _lib.Handle(X, y, "se_ard", "const", device=[0, 0])
    g.set_option("shard_min_n", 0)                               # its likelihood is sharded over the two virtual ranks
    ll0 = g.loglik(th)
    res = g.loo(th)
    _check_values(res, ref.loo_closed_form("se_ard", th, X, y, "const"), y, "2 virtual ranks")
    total, grad, info = g.loo_grad(th)
    one = _lib.Handle(X, y, "se_ard", "const")
    t1, g1, _ = one.loo_grad(th)
    one.close()
    assert info == 0 and total == res["total"]
    np.testing.assert_allclose(grad, g1, rtol=1e-9, atol=1e-9 * np.abs(g1).max())
    assert g.loglik(th) == ll0                                    # the sharded evaluation afterwards is unchanged
    g.close()


def test_fp32_handles():
    """fp32 device arithmetic against the fp64 numpy reference.  No bar can be derived (the error scales with eps32 cond(K),
    DESIGN.md section 9), so it was measured on these inputs at the first device run and the bars are 4 x that:
    mean 3.2e-5 max|y| -> 1.3e-4, var 7.2e-7 -> 2.9e-6, log p 3.0e-4 -> 1.2e-3, L_LOO 3.8e-6 relative -> 1.5e-5,
    gradient 2.0e-5 of max |grad| -> 8.2e-5 (all far tighter than the 2-3e-2 of the fp32 likelihood-gradient tests)."""
    n, d = 1000, 3
    X, y = syn.make_dataset(n, d)
    th = _theta("se_ard", d, "const")
    want = ref.loo_closed_form("se_ard", th, X, y, "const")
    gwant = ref.loo_grad_formula("se_ard", th, X, y, "const")
    for opts in (None, {"dataflow": 0}):
        h = _lib.Handle(X, y, "se_ard", "const", dtype=32)
        for k, v in (opts or {}).items():
            h.set_option(k, v)
        res = h.loo(th)
        em = np.abs(res["mean"] - want["mean"]).max() / np.abs(y).max()
        ev = np.abs(res["var"] - want["var"]).max()
        el = np.abs(res["logp"] - want["logp"]).max()
        et = abs(res["total"] - want["total"]) / abs(want["total"])
        total, g, info = h.loo_grad(th)
        eg = np.abs(g - gwant).max() / np.abs(gwant).max()
        print(f"fp32 {opts}: mean {em:.2e} var {ev:.2e} logp {el:.2e} total {et:.2e} grad {eg:.2e}")
        assert res["info"] == 0 and info == 0
        assert em <= 1.3e-4 and ev <= 2.9e-6 and el <= 1.2e-3 and et <= 1.5e-5 and eg <= 8.2e-5
        assert total == res["total"] == ref.device_total(res["logp"])
        assert np.array_equal(h.loo_grad(th)[1], g)
        h.close()


def test_python_layer_on_the_device():
    n, d = 300, 2
    X, y = syn.make_dataset(n, d)
    y = 2.0 * y + 1.0
    variables = [("l1", 0.1, 10.0), ("l2", 0.1, 10.0), ("sf", 0.1, 10.0), ("sn", 0.05, 2.0)]
    th = np.array([0.9, 1.2, 1.0, 0.2])
    obj = gp.defineGaussianProcess((X, y), "SEARD", variables=variables)
    assert "LogPseudoLikelihoodFunction" in obj and "LogPseudoLikelihoodGradientFunction" in obj
    want = ref.loo_closed_form("se_ard", th, X, y, "zero")
    out = gp.leaveOneOutFromGaussianProcess(obj, th)
    np.testing.assert_allclose(out["Mean"], want["mean"], rtol=0, atol=1e-7 * np.abs(y).max())
    np.testing.assert_allclose(out["StandardDeviation"] ** 2, want["var"], rtol=0, atol=1e-7)
    assert out["LogPseudoLikelihood"] == pytest.approx(want["total"], rel=1e-8)
    np.testing.assert_allclose(out["StandardizedResiduals"], (y - want["mean"]) / np.sqrt(want["var"]), rtol=0, atol=1e-6)
    assert obj["LogPseudoLikelihoodFunction"](th) == pytest.approx(want["total"], rel=1e-8)
    val, grad = obj["LogPseudoLikelihoodGradientFunction"](th)
    gw = ref.loo_grad_formula("se_ard", th, X, y, "zero")
    assert val == pytest.approx(want["total"], rel=1e-8) and np.abs(grad - gw).max() <= 1e-7 * np.abs(gw).max()
    # the sentinel, never an exception
    assert obj["LogPseudoLikelihoodFunction"]([0.9, 1.2, 1.0, float("nan")]) == gp.MACHINE_LOG_ZERO
    v, g = obj["LogPseudoLikelihoodGradientFunction"]([0.9, 1.2, 1.0, float("nan")])
    assert v == gp.MACHINE_LOG_ZERO and np.all(np.isnan(g))
    # the posterior mixture over "Samples"
    t2 = np.array([1.3, 0.8, 1.2, 0.3])
    samples = [{"Point": th, "CrudePosteriorWeight": 0.25}, {"Point": t2, "CrudePosteriorWeight": 0.75}]
    mix = gp.leaveOneOutFromGaussianProcess(obj.append({"Samples": samples}))
    w2 = ref.loo_closed_form("se_ard", t2, X, y, "zero")
    np.testing.assert_allclose(mix["LogDensity"], np.log(0.25 * np.exp(want["logp"]) + 0.75 * np.exp(w2["logp"])), rtol=0, atol=1e-7)
    # hyper-parameter selection from a start near the truth
    start = np.array([0.8, 0.8, 1.0, 0.25])
    v0, g0 = obj["LogPseudoLikelihoodGradientFunction"](start)
    sel = laplace.selectHyperparameters(obj, Criterion="LeaveOneOut", InitialGuess=start)
    v1, g1 = obj["LogPseudoLikelihoodGradientFunction"](sel["Maximum"][1])
    print(f"selectHyperparameters: L_LOO {v0:.4f} -> {v1:.4f}, |grad| {np.linalg.norm(g0):.3g} -> {np.linalg.norm(g1):.3g}")
    assert sel["Criterion"] == "LeaveOneOut" and sel["Maximum"][0] == pytest.approx(v1, rel=1e-12)
    assert v1 >= v0 and np.linalg.norm(g1) <= 1e-3 * np.linalg.norm(g0)
    ml = laplace.selectHyperparameters(obj, Criterion="MarginalLikelihood", InitialGuess=start)
    assert ml is not None and obj["LogLikelihoodFunction"](ml["Maximum"][1]) >= obj["LogLikelihoodFunction"](start)
    obj["GaussianProcessData"]["HIPHandle"].close()
    # normalised data: the answer comes back in the units of the data
    nd = gp.normalizeData(X, y[:, None])
    objn = gp.defineGaussianProcess(nd, "SEARD", variables=variables)
    outn = gp.leaveOneOutFromGaussianProcess(objn, th)
    Xn, yn = nd["Input"]["NormalizedData"], nd["Output"]["NormalizedData"][:, 0]
    wn = ref.loo_closed_form("se_ard", th, Xn, yn, "zero")
    sd_y = y.std(ddof=1)
    np.testing.assert_allclose(outn["Mean"], wn["mean"] * sd_y + y.mean(), rtol=0, atol=1e-7 * np.abs(y).max())
    np.testing.assert_allclose(outn["StandardDeviation"], np.sqrt(wn["var"]) * sd_y, rtol=1e-6)
    np.testing.assert_allclose(outn["LogDensity"], wn["logp"] - np.log(sd_y), rtol=0, atol=1e-6)
    objn["GaussianProcessData"]["HIPHandle"].close()
