"""gphip_predict_grad on the device -- the gradients of the predictive mean and variance in the test inputs of the exact object --
against the CPU references of tests/predict_grad_reference.py (pinned by tests/test_predict_grad.py: numpy and torch autograd
agree to 1e-10 on every case).

The fp64 bar is the project's parity bar, 1e-8 of max |reference| over the test set.  The shapes are the smallest that reach
every branch: N = 300 (Npad = 384, a ragged last tile, five slabs of 64 training points), M = 130 (two 128-tiles of test points,
the last one ragged).  Errors measured on an MI355X are in DESIGN.md section 8j."""
import numpy as np
import pytest

import predict_grad_reference as pg
from bayesianinference_amd import _lib, gaussian_process as gp

pytestmark = pytest.mark.gpu

BAR = 1e-8
IDS = [pg.case_id(c) for c in pg.CASES]
SE_ARD_BODY = "T s = 0; for (int k = 0; k < D; ++k) { const T u = (X(k) - Y(k)) / P(k); s += u * u; } return P(D) * P(D) * exp((T)-0.5 * s);"


def _err(g, want):
    return float(np.abs(g - want).max() / np.abs(want).max())


def _fitted(c, dtype=64, opts=None):
    h = _lib.Handle(c["X"], c["y"], c["kernel"], c["mean_kind"], dtype=dtype)
    for k, v in (opts or {}).items():
        h.set_option(k, v)
    assert h.fit(c["theta"]) == 0
    return h


def _check(c, out, label, bar=BAR):
    mean, var, dmean, dvar = out
    em, ev = _err(dmean, c["dmean"][:len(dmean)]), _err(dvar, c["dvar"][:len(dvar)])
    print(f"{label}: dmean {em:.3e} dvar {ev:.3e} of max |reference|; mean {_err(mean, c['mean'][:len(mean)]):.3e} "
          f"var {_err(var, c['var'][:len(var)]):.3e}")
    assert em <= bar and ev <= bar, label
    return em, ev


@pytest.mark.parametrize("name,d,mean", pg.CASES, ids=IDS)
def test_gradients_match_the_reference(name, d, mean):
    c = pg.case_reference(name, d, mean)
    h = _fitted(c)
    pm, pv = h.predict(c["Xs"])
    out = h.predict_grad(c["Xs"])
    h.close()
    assert out[2].shape == (pg.M, d) and out[3].shape == (pg.M, d)
    _check(c, out, f"{name} d={d} {mean}")
    # mean / var are gphip_predict's, to rounding (the same launches on the same operands)
    assert _err(out[0], pm) <= 1e-13 and _err(out[1], pv) <= 1e-13
    assert _err(out[0], c["mean"]) <= BAR and _err(out[1], c["var"]) <= BAR


def test_one_test_point_and_no_variance():
    name, d, mean = pg.CASES[1]
    c = pg.case_reference(name, d, mean)
    h = _fitted(c)
    one = h.predict_grad(c["Xs"][:1])
    full = h.predict_grad(c["Xs"])
    mean_only = h.predict_grad(c["Xs"], variance=False)
    h.close()
    assert one[2].shape == (1, d)
    _check(c, one, "M = 1")
    assert mean_only[3] is None
    assert np.array_equal(mean_only[2], full[2])                 # dvar = NULL: dmean is the same bytes
    assert np.array_equal(mean_only[0], full[0]) and np.array_equal(mean_only[1], full[1])


def test_strips_agree_with_the_reference_and_repeat_bit_for_bit():
    name, d, mean = pg.CASES[5]                                   # two terms
    c = pg.case_reference(name, d, mean)
    h = _fitted(c)
    for split, want in ((0, None), (1, 1), (3, 3)):
        h.set_option("predict_grad_split", split)
        a = h.predict_grad(c["Xs"])
        b = h.predict_grad(c["Xs"])
        ns = int(h.get_option("last_predict_grad_nsplit"))
        _check(c, a, f"split {split} -> {ns} strips")
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), split              # the same bytes
        assert ns == (want if want is not None else 5)            # by the rule: one strip per slab of 64 while workgroups are few
    h.close()


def test_chunk_seam():
    name, d, mean = pg.CASES[2]
    c = pg.case_reference(name, d, mean)
    h = _fitted(c)
    one = h.predict_grad(c["Xs"])
    assert int(h.get_option("last_predict_grad_chunk")) >= 256
    h.set_option("predict_grad_chunk", 128)
    two = h.predict_grad(c["Xs"])
    assert int(h.get_option("last_predict_grad_chunk")) == 128
    h.close()
    _check(c, one, "one chunk")
    _check(c, two, "chunks of 128 + 2")
    for a, b in zip(one, two):                                    # to rounding: eps x cond(K) ~ 1e-16 x 2e4, over sums of 300 terms
        assert np.abs(a - b).max() <= 1e-10 * np.abs(a).max()


@pytest.mark.parametrize("opts", [{}, {"dataflow": 0}], ids=["dataflow-fit", "lookahead-fit"])
def test_both_substitution_routes(opts):
    name, d, mean = pg.CASES[4]
    c = pg.case_reference(name, d, mean)
    h = _fitted(c, opts=opts)
    out = h.predict_grad(c["Xs"])
    h.close()
    _check(c, out, f"{name} {opts}")


def test_after_loglik_grad_and_loo():
    name, d, mean = pg.CASES[1]
    c = pg.case_reference(name, d, mean)
    h = _lib.Handle(c["X"], c["y"], name, mean)
    assert h.loglik_grad(c["theta"])[2] == 0
    _check(c, h.predict_grad(c["Xs"]), "after loglik_grad")
    assert h.loo(c["theta"])["info"] == 0
    _check(c, h.predict_grad(c["Xs"]), "after loo")
    h.close()


def test_statuses_and_no_side_effects():
    name, d, mean = pg.CASES[1]
    c = pg.case_reference(name, d, mean)
    Xs = c["Xs"]
    h = _lib.Handle(c["X"], c["y"], name, mean)
    with pytest.raises(_lib.GphipError) as e:
        h.predict_grad(Xs)
    assert e.value.status == 4                                    # before a fit
    assert h.fit(c["theta"]) == 0
    pm, pv = h.predict(Xs)
    h.predict_grad(Xs)
    pm2, pv2 = h.predict(Xs)
    assert np.array_equal(pm, pm2) and np.array_equal(pv, pv2)    # the fit is untouched
    # a fit with point-dependent arrays has no gradient; with both NULL it is a plain fit
    assert h.fit_pw(c["theta"], nugget_train=np.full(pg.N, pg.SN ** 2)) == 0
    with pytest.raises(_lib.GphipError) as e:
        h.predict_grad(Xs)
    assert e.value.status == 6
    assert h.fit_pw(c["theta"]) == 0
    _check(c, h.predict_grad(Xs), "after fit_pw with both arrays NULL")
    h.close()
    custom = _lib.Handle(c["X"], c["y"], _lib.CustomKernel(SE_ARD_BODY, d + 1), mean)
    th = c["theta"]
    assert custom.fit(th) == 0
    with pytest.raises(_lib.GphipError) as e:
        custom.predict_grad(Xs)
    assert e.value.status == 6
    custom.close()
    null = _lib.Handle(c["X"], c["y"], "null", "const")
    assert null.fit(np.array([0.3, 0.2])) == 0
    mean_, var_, dm, dv = null.predict_grad(Xs)
    null.close()
    assert np.all(dm == 0.0) and np.all(dv == 0.0) and dm.shape == (pg.M, d)
    assert np.all(mean_ == 0.2) and np.allclose(var_, 0.09, rtol=1e-15)


@pytest.mark.parametrize("name,d,mean", [pg.CASES[1], pg.CASES[2]], ids=[IDS[1], IDS[2]])
def test_fp32_handle(name, d, mean):
    """The bar is 10 x the relative error of the fp32 handle's own predictive mean on the case (what the parent commit computes):
    one division by the length scale and one more substitution.  Measured on an MI355X: see DESIGN.md section 8j."""
    c = pg.case_reference(name, d, mean)
    h = _fitted(c, dtype=32)
    pm, _ = h.predict(c["Xs"])
    out = h.predict_grad(c["Xs"])
    h.close()
    base = _err(pm, c["mean"])
    em, ev = _err(out[2], c["dmean"]), _err(out[3], c["dvar"])
    print(f"fp32 {name} d={d}: predict mean {base:.3e}; dmean {em:.3e} dvar {ev:.3e}; bar {10 * base:.3e}")
    assert em <= 10 * base and ev <= 10 * base


def test_maximising_the_mean_with_the_device_gradient():
    import scipy.optimize as so
    name, d, mean = pg.CASES[3]                                   # d = 2
    c = pg.case_reference(name, d, mean)
    h = _fitted(c)

    def neg_mu(x):
        m, _, dm, _ = h.predict_grad(x[None, :], variance=False)
        return -m[0], -dm[0]
    start = c["Xs"][int(np.argmax(c["mean"]))]
    res = so.minimize(neg_mu, start, jac=True, method="BFGS", options={"gtol": 1e-9})
    h.close()
    end = pg.exact(name, c["theta"], c["X"], c["y"], res.x[None, :], mean)
    scale = np.abs(c["dmean"]).max()
    print(f"from {start} to {res.x} in {res.nit} iterations ({res.nfev} calls): mean {c['mean'].max():.6f} -> {end['mean'][0]:.6f}; "
          f"reference |grad| at the end {np.abs(end['dmean']).max():.3e} of {scale:.3e} over the start set")
    assert end["mean"][0] >= c["mean"].max()
    assert np.abs(end["dmean"]).max() <= 1e-6 * scale


def test_python_layer():
    name, d, mean = pg.CASES[0]                                   # se, d = 1, zero mean
    c = pg.case_reference(name, d, mean)
    pts = c["Xs"][:40]
    out = gp.predictGradientFromGaussianProcess((c["X"], c["y"][:, None]), pts[:, 0], "se", c["theta"])
    marg = gp.predictFromGaussianProcess((c["X"], c["y"][:, None]), pts[:, 0], "se", c["theta"])
    assert out["MeanGradient"].shape == (40, 1) and out["VarianceGradient"].shape == (40, 1)
    assert _err(out["MeanGradient"], c["dmean"][:40]) <= BAR and _err(out["VarianceGradient"], c["dvar"][:40]) <= BAR
    np.testing.assert_allclose(out["Mean"], marg["Mean"][0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["StandardDeviation"], marg["StandardDeviation"][0], rtol=1e-10)
    # a posterior of two samples: per-sample arrays from a host loop
    obj = gp.defineGaussianProcess((c["X"], c["y"][:, None]), "se", variables=[("l", 0.05, 2.0), ("sf", 0.1, 5.0), ("sn", 0.01, 1.0)])
    obj = obj.append({"Samples": [{"Point": c["theta"], "CrudePosteriorWeight": 0.6},
                                  {"Point": np.array([0.6, 0.7, 0.2]), "CrudePosteriorWeight": 0.4}]})
    samp = gp.predictGradientFromGaussianProcess(obj, pts[:, 0])
    assert samp["MeanGradient"].shape == (2, 40, 1) and np.allclose(samp["Weights"], [0.6, 0.4])
    assert _err(samp["MeanGradient"][0], c["dmean"][:40]) <= BAR
    want = pg.exact("se", np.array([0.6, 0.7, 0.2]), c["X"], c["y"], pts, "zero")
    assert _err(samp["VarianceGradient"][1], want["dvar"]) <= BAR
