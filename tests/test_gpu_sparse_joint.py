"""The sparse object's joint predictive distribution on the device (gphip_sparse_predict_cov / _draws / _logpdf) against the numpy
reference of tests/sparse_joint_reference.py (pinned on the CPU by tests/test_sparse_joint.py).  Bars are the sparse path's own
(DESIGN.md section 8c): 1e-7 x sf^2 for covariance entries, 1e-7 x max |y| for means; what differs from gphip_sparse_predict only
by summation order is held to 1e-12 (m eps k ~ 4e-14 at m <= 300)."""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.stats as sst

import sparse_joint_reference as jref
from bayesianinference_amd import _lib, gaussian_process as gp, nested_sampling as ns, synthetic as syn

pytestmark = pytest.mark.gpu

SF2 = jref.SF ** 2
ERR_DIM, ERR_STATE = 2, 4                      # GPHIP_ERR_DIM, GPHIP_ERR_STATE (include/gphip.h)
JOINT_MAX_M = 16384                            # GPHIP_JOINT_MAX_M


def _fitted(case, dtype=64, jitter=None):
    _, n, d, m, M, name, mean = case
    X, y, Z, Xs, ys, kernel, th, jit = jref.case_data(n, d, m, M, name, mean)
    h = _lib.SparseHandle(X, y, Z, kernel, mean, dtype=dtype)
    assert h.fit(th, jit if jitter is None else jitter) == 0
    return h, X, y, Xs, ys, th


def _status(fn, *args, **kw):
    with pytest.raises(_lib.GphipError) as e:
        fn(*args, **kw)
    return e.value.status


@pytest.mark.parametrize("case", jref.CASES, ids=lambda c: c[0])
def test_cov_and_mean_match_numpy_and_predict(case):
    _, n, d, m, M, name, mean = case
    h, X, y, Xs, _, th = _fitted(case)
    mu_ref, S_ref = jref.case_reference(n, d, m, M, name, mean)
    mu, cov = h.predict_cov(Xs)
    es, em = np.abs(cov - S_ref).max() / SF2, np.abs(mu - mu_ref).max() / np.abs(y).max()
    print(f"{case[0]}: cov {es:.2e} x sf^2, mean {em:.2e} x max|y|, strips {h.get_option('last_sparse_joint_nsplit'):.0f}")
    assert cov.shape == (M, M) and mu.shape == (M,)
    assert es <= 1e-7 and em <= 1e-7
    assert np.array_equal(cov, cov.T)
    # latent form: the same matrix without sn^2 on the diagonal, the same mean bytes
    sn2 = float(th[-2 if mean == "const" else -1]) ** 2
    mu_l, cov_l = h.predict_cov(Xs, latent=True)
    assert np.abs(cov - sn2 * np.eye(M) - cov_l).max() <= 1e-12
    assert np.array_equal(mu_l, mu)
    # consistency with the per-point call: only the summation order differs
    pm, pv = h.predict(Xs)
    ed, ep = np.abs(np.diag(cov) - pv).max() / SF2, np.abs(mu - pm).max() / np.abs(y).max()
    print(f"{case[0]}: diag(cov) vs predict {ed:.2e} x sf^2, mean {ep:.2e} x max|y|")
    assert ed <= 1e-12 and ep <= 1e-12
    h.close()


def test_strips_agree_and_repeat_bit_for_bit():
    _, n, d, m, M, name, mean = jref.STRIPS
    h, X, y, Xs, _, th = _fitted(jref.STRIPS)
    res = {}
    for split in (4, 1, 0):
        h.set_option("sparse_joint_split", split)
        mu, cov = h.predict_cov(Xs)
        used = int(h.get_option("last_sparse_joint_nsplit"))
        mu2, cov2 = h.predict_cov(Xs)
        assert np.array_equal(cov, cov2) and np.array_equal(mu, mu2), split
        res[split] = (mu, cov, used)
    print("strips used:", {k: v[2] for k, v in res.items()})
    # m_pad = 384: six tile columns of the stacked index; 4 asked -> strips of two, the middle one spans the V1 / V2 boundary
    assert res[4][2] == 3 and res[1][2] == 1
    for split in (1, 0):
        assert np.abs(res[4][1] - res[split][1]).max() <= 1e-12
        assert np.abs(res[4][0] - res[split][0]).max() <= 1e-12
    mu_ref, S_ref = jref.case_reference(n, d, m, M, name, mean)
    for split in (4, 1, 0):
        assert np.abs(res[split][1] - S_ref).max() <= 1e-7 * SF2
        assert np.abs(res[split][0] - mu_ref).max() <= 1e-7 * np.abs(y).max()
    h.close()


def test_logpdf_matches_scipy():
    case = jref.CASES[4]                       # N = 1500, d = 2, m = 200, M = 300
    _, n, d, m, M, name, mean = case
    h, X, y, Xs, ys, th = _fitted(case)
    mu_ref, S_ref = jref.case_reference(n, d, m, M, name, mean)
    want = sst.multivariate_normal(mu_ref, S_ref).logpdf(ys)
    got, info = h.predict_logpdf(Xs, ys)
    print(f"logpdf {got:.10f} reference {want:.10f} rel {abs(got - want) / abs(want):.2e}")
    assert info == 0 and abs(got - want) <= 1e-9 * abs(want)
    pm, pv = h.predict(Xs[:1])
    one, info = h.predict_logpdf(Xs[:1], ys[:1])
    assert info == 0 and abs(one - sst.norm(pm[0], np.sqrt(pv[0])).logpdf(ys[0])) <= 1e-10 * max(1.0, abs(one))
    h.close()


def test_draws_with_given_normals_and_seeded_draws():
    _, n, d, m, M, name, mean = jref.DRAWS
    h, X, y, Xs, _, th = _fitted(jref.DRAWS)
    mu, S = jref.case_reference(n, d, m, M, name, mean)
    jit = 1e-8
    z = np.random.default_rng(3).standard_normal((50, M))
    out, info = h.predict_draws(Xs, 50, z=z, latent=False, jitter=jit)
    Lr = np.linalg.cholesky(S + jit * np.eye(M))
    assert info == 0 and out.shape == (50, M)
    print(f"draws from given normals: max |error| {np.abs(out - (mu + z @ Lr.T)).max():.2e}")
    np.testing.assert_allclose(out, mu + z @ Lr.T, rtol=0, atol=1e-9)
    # seeded: same seed -> same bytes, S = 100 is the prefix of S = 300, another seed differs
    a, ia = h.predict_draws(Xs, 300, seed=11)
    a2, _ = h.predict_draws(Xs, 300, seed=11)
    b, ib = h.predict_draws(Xs, 100, seed=11)
    c, _ = h.predict_draws(Xs, 100, seed=12)
    assert ia == ib == 0
    assert np.array_equal(a, a2) and np.array_equal(a[:100], b) and not np.array_equal(b, c)
    # whitened residuals of 4000 latent draws are standard normal (the exact path's criteria)
    SL = jref.case_reference(n, d, m, M, name, mean, True)[1]
    w4, info = h.predict_draws(Xs, 4000, seed=5, latent=True, jitter=1e-9)
    assert info == 0
    Ll = np.linalg.cholesky(SL + 1e-9 * np.eye(M))
    w = sla.solve_triangular(Ll, (w4 - mu).T, lower=True)
    nw = w.size
    print(f"whitened latent draws: mean {w.mean():.2e} (bar {4.0 / np.sqrt(nw):.2e}) var - 1 {w.var() - 1.0:.2e} (bar {4.0 * np.sqrt(2.0 / nw):.2e})")
    assert abs(w.mean()) <= 4.0 / np.sqrt(nw)
    assert abs(w.var() - 1.0) <= 4.0 * np.sqrt(2.0 / nw)
    h.close()


def test_state_statuses_and_no_side_effects():
    case = jref.CASES[1]                       # N = 700, d = 3, m = 60, M = 130
    _, n, d, m, M, name, mean = case
    X, y, Z, Xs, ys, kernel, th, jit = jref.case_data(n, d, m, M, name, mean)
    h = _lib.SparseHandle(X, y, Z, kernel, mean)
    # before a fit
    assert _status(h.predict_cov, Xs) == ERR_STATE
    assert _status(h.predict_draws, Xs, 3) == ERR_STATE
    assert _status(h.predict_logpdf, Xs, ys) == ERR_STATE
    assert h.fit(th, jit) == 0
    # the three calls leave the fit as it was: predict and bound return the same bytes before and after
    pm0, pv0 = h.predict(Xs)
    mu, cov = h.predict_cov(Xs)
    _, info = h.predict_draws(Xs, 5)
    assert info == 0
    _, info = h.predict_logpdf(Xs, ys)
    assert info == 0
    pm1, pv1 = h.predict(Xs)
    assert np.array_equal(pm0, pm1) and np.array_equal(pv0, pv1)
    F0 = h.bound(th, jit)
    h.predict_cov(Xs)
    h.predict_draws(Xs, 5)
    h.predict_logpdf(Xs, ys)
    assert h.bound(th, jit) == F0
    # dimensions
    assert _status(h.predict_cov, np.zeros((0, d))) == ERR_DIM
    assert _status(h.predict_logpdf, np.zeros((0, d)), np.zeros(0)) == ERR_DIM
    assert _status(h.predict_cov, np.zeros((JOINT_MAX_M + 1, d))) == ERR_DIM
    assert _status(h.predict_draws, Xs, 0) == ERR_DIM
    # a non-finite held-out output
    bad = ys.copy()
    bad[7] = np.inf
    val, info = h.predict_logpdf(Xs, bad)
    assert info == _lib.INFO_NAN and np.isnan(val)
    # a second call with another M
    Xs2 = Xs[:77]
    mu2, cov2 = h.predict_cov(Xs2)
    assert np.abs(cov2 - cov[:77, :77]).max() <= 1e-12 and np.abs(mu2 - mu[:77]).max() <= 1e-12
    mu3, cov3 = h.predict_cov(Xs)
    assert np.array_equal(cov3, cov) and np.array_equal(mu3, mu)
    # bound_batch and set_inducing drop the fit
    h.bound_batch(np.vstack([th, th]), jit)
    assert _status(h.predict_cov, Xs) == ERR_STATE
    assert h.fit(th, jit) == 0
    h.set_inducing(Z[::-1].copy())
    assert _status(h.predict_draws, Xs, 3) == ERR_STATE
    assert _status(h.predict_logpdf, Xs, ys) == ERR_STATE
    # another m and a refit: the calls work and match the reference
    Z2 = gp.selectInducingPoints(X, 150, seed=1)
    h.set_inducing(Z2)
    assert h.fit(th, jit) == 0
    mu_ref, S_ref = jref.joint_formulas(kernel, th, X, y, Z2, jit, Xs, mean)
    mu4, cov4 = h.predict_cov(Xs)
    assert np.abs(cov4 - S_ref).max() <= 1e-7 * SF2 and np.abs(mu4 - mu_ref).max() <= 1e-7 * np.abs(y).max()
    val, info = h.predict_logpdf(Xs, ys)
    want = sst.multivariate_normal(mu_ref, S_ref).logpdf(ys)
    assert info == 0 and abs(val - want) <= 1e-9 * abs(want)
    h.close()


def test_latent_sigma_without_jitter_is_not_spd_not_an_error():
    case = ("rank-deficient", 700, 3, 60, 1000, "se_ard", "zero")
    _, n, d, m, M, name, mean = case
    S_ref = jref.case_reference(n, d, m, M, name, mean, True)[1]
    with pytest.raises(np.linalg.LinAlgError):         # (the premise: the reference's latent Sigma has a negative eigenvalue)
        np.linalg.cholesky(S_ref)
    h, X, y, Xs, _, th = _fitted(case)
    out, info = h.predict_draws(Xs, 3, seed=1, latent=True, jitter=0.0)
    assert info == _lib.INFO_NOT_SPD and out.shape == (3, M) and np.isnan(out).all()
    out, info = h.predict_draws(Xs, 3, seed=1, latent=True)                  # the default jitter factors it
    assert info == 0 and np.isfinite(out).all()
    h.close()


# fp32 bars: 4 x the errors measured on the MI355X (cov 5.14e-6 x sf^2, mean 7.34e-5 x max |y|, log density
# 2.74e-5 relative), the convention of section 8c's fp32 bars
FP32_COV, FP32_MEAN, FP32_LOGPDF = 4 * 5.14e-6, 4 * 7.34e-5, 4 * 2.74e-5


def test_fp32_object():
    _, n, d, m, M, name, mean = jref.STRIPS
    X, y, Z, Xs, ys, kernel, th, _ = jref.case_data(n, d, m, M, name, mean)
    h = _lib.SparseHandle(X, y, Z, kernel, mean, dtype=32)
    assert h.fit(th) == 0                      # default jitters
    jit = h.get_option("last_jitter")
    mu_ref, S_ref = jref.joint_formulas(kernel, th, X, y, Z, jit, Xs, mean)
    mu, cov = h.predict_cov(Xs)
    es, em = np.abs(cov - S_ref).max() / SF2, np.abs(mu - mu_ref).max() / np.abs(y).max()
    want = sst.multivariate_normal(mu_ref, S_ref).logpdf(ys)
    got, info = h.predict_logpdf(Xs, ys)
    el = abs(got - want) / abs(want)
    print(f"fp32 (jitter {jit:.3e}): cov {es:.3e} x sf^2, mean {em:.3e} x max|y|, logpdf {el:.3e} relative")
    assert info == 0
    assert np.array_equal(cov, cov.T)
    assert es <= FP32_COV and em <= FP32_MEAN and el <= FP32_LOGPDF
    out, info = h.predict_draws(Xs, 8)
    assert info == 0 and np.isfinite(out).all()
    h.close()


def test_python_layer():
    X, y = syn.make_dataset(600, 2)
    Y = y[:, None]
    th = jref.theta_of("se_ard", 2, "zero")
    variables = [("l1", 0.1, 3.0), ("l2", 0.1, 3.0), ("sf", 0.1, 5.0), ("sn", 0.01, 1.0)]
    obj = gp.defineSparseGaussianProcess((X, Y), "se_ard", 40, variables=variables, Jitter=1e-8 * SF2, Seed=1)
    Z = obj["InducingPoints"]
    pts = syn.make_test_points(30, 2)
    joint = gp.predictJointFromSparseGaussianProcess(obj, np.vstack([pts, pts[:5]]), th)
    marg = gp.predictFromSparseGaussianProcess(obj, pts, th)
    assert joint["Covariance"].shape == (30, 30) and np.array_equal(joint["Points"], pts)
    np.testing.assert_allclose(joint["Mean"], marg["Mean"][0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.sqrt(np.diag(joint["Covariance"])), marg["StandardDeviation"][0], rtol=1e-10)
    mu_ref, S_ref = jref.joint_formulas("se_ard", th, X, y, Z, obj["Jitter"], pts)
    assert np.abs(joint["Covariance"] - S_ref).max() <= 1e-7 * SF2
    ys = syn.make_outputs(pts)
    ld = gp.sparsePredictiveLogDensity(obj, (pts, ys), th)
    assert abs(ld - sst.multivariate_normal(mu_ref, S_ref).logpdf(ys)) <= 1e-9 * abs(ld)
    assert gp.gaussianProcessFunctionSamples(obj, pts, 5) is None                  # unsampled
    # a small sampled object: the native sampler on the bound, pool 20
    sampled = ns.nestedSampling(obj, SamplePoolSize=20, MaxIterations=30, MinIterations=10, Seed=3)
    assert not isinstance(sampled, str) and "Samples" in sampled
    fs = gp.gaussianProcessFunctionSamples(sampled, pts, 50, seed=4)
    fs2 = gp.gaussianProcessFunctionSamples(sampled, pts, 50, seed=4)
    assert fs["Values"].shape == (50, 30) and fs["Sample"].shape == (50,) and np.array_equal(fs["Points"], pts)
    assert fs["Sample"].min() >= 0 and fs["Sample"].max() < len(sampled["Samples"])
    assert np.isfinite(fs["Values"]).all()
    assert np.array_equal(fs["Values"], fs2["Values"]) and np.array_equal(fs["Sample"], fs2["Sample"])
    obj["SparseGaussianProcessData"]["HIPHandle"].close()
