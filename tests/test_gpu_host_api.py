"""GPU tests of the host-side mirror: defineGaussianProcess / predictFromGaussianProcess behave
like the reference's (BGP:228-330, 332-394) with the HIP closure installed."""
import numpy as np
import pytest

from bayesianinference_amd import _lib, gaussian_process as gp, synthetic as syn
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu


def test_define_gaussian_process_object_and_closure():
    X, y = syn.make_dataset(200, 2)
    variables = [("l1", 0.1, 10.0), ("l2", 0.1, 10.0), ("sf", 0.1, 10.0), ("sn", 0.05, 1.0)]
    obj = gp.defineGaussianProcess((X, y), "SEARD", "Constant", None, variables, "Uniform", Note="extra rule")
    assert not obj.failed
    for key in ("Data", "PriorDistribution", "Parameters", "ParameterSymbols", "GaussianProcessData",
                "LogLikelihoodFunction", "LogPriorPDFFunction", "LogLikelihoodGradientFunction", "Note"):
        assert key in obj
    mf = obj["GaussianProcessData", "ModelFunctions"]
    assert set(mf) == {"KernelFunction", "NuggetFunction", "MeanFunction", "CovarianceFunction",
                       "InverseCovarianceFunction"}
    th = np.array([0.8, 1.7, 1.2, 0.3])
    want = orc.log_likelihood("se_ard", th, X, y)
    assert obj["LogLikelihoodFunction"](th) == pytest.approx(want, rel=1e-8)
    # Listable use (B x p) and sentinel on numerical failure, never an exception (BS:276-298)
    batch = obj["LogLikelihoodFunction"](np.array([th, [0.8, 1.7, 1.2, 0.0]]))
    assert batch[0] == pytest.approx(want, rel=1e-8)
    Xd = X.copy()
    Xd[5] = Xd[9]
    obj2 = gp.defineGaussianProcess((Xd, y), "SEARD", variables=variables,
                                    LogLikelihoodFunction=None)
    assert obj2["LogLikelihoodFunction"]([1.0, 1.0, 1.0, 0.0]) == gp.MACHINE_LOG_ZERO
    np.testing.assert_allclose(mf["CovarianceFunction"](th), orc.covariance_matrix("se_ard", th, X), rtol=1e-12)
    val, grad = obj["LogLikelihoodGradientFunction"](th)
    assert val == pytest.approx(want, rel=1e-8)
    np.testing.assert_allclose(grad, orc.log_likelihood_grad("se_ard", th, X, y), rtol=1e-6)
    inv = mf["InverseCovarianceFunction"](th)
    assert inv["LogDet"] == pytest.approx(orc.log_likelihood("se_ard", th, X, y, parts=True)[1], rel=1e-9)


def test_user_supplied_loglikelihood_passes_through():
    X, y = syn.make_dataset(50, 1)
    f = lambda theta: -1.0                                       # noqa: E731  (BGP:293-294)
    obj = gp.defineGaussianProcess((X, y), "SE", variables=[("l", 0.1, 1), ("sf", 0.1, 1), ("sn", 0.1, 1)],
                                   LogLikelihoodFunction=f)
    assert obj["LogLikelihoodFunction"] is f


def test_predict_from_gaussian_process_forms():
    X, y = syn.make_dataset(150, 1)
    variables = [("l", 0.05, 5.0), ("sf", 0.1, 5.0), ("sn", 0.05, 1.0)]
    obj = gp.defineGaussianProcess((X, y), "SE", variables=variables)
    samples = [{"Point": [0.3, 1.0, 0.1], "CrudePosteriorWeight": 0.7},
               {"Point": [0.5, 1.3, 0.2], "CrudePosteriorWeight": 0.3}]
    res = gp.predictFromGaussianProcess(obj.append({"Samples": samples}), 9)      # integer-grid form
    assert res["Points"].shape == (9, 1) and res["Mean"].shape == (2, 9)
    w, mu, sd = orc.predict_mixture("se", [s["Point"] for s in samples], [0.7, 0.3], X, y, res["Points"])
    np.testing.assert_allclose(res["Mean"], mu, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(res["StandardDeviation"], sd, rtol=1e-7)
    m, v = gp.mixture_moments(res)
    mo, vo = orc.mixture_moments(w, mu, sd)
    np.testing.assert_allclose(m, mo, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(v, vo, rtol=1e-6)
    assert gp.predictFromGaussianProcess(obj, 9) is None                          # no "Samples" key
    # direct form, duplicates removed (BGP:380)
    pts = np.array([[0.1], [0.2], [0.1]])
    res = gp.predictFromGaussianProcess((X, y), pts, "SE", [0.3, 1.0, 0.1])
    assert res["Points"].shape == (2, 1)
    mo, so = orc.predict_internal("se", [0.3, 1.0, 0.1], X, y, res["Points"])
    np.testing.assert_allclose(res["Mean"][0], mo, rtol=1e-7, atol=1e-9)


def test_normalized_data_and_persistence_roundtrip(tmp_path):
    rng = np.random.default_rng(5)
    X = rng.normal(10.0, 3.0, (120, 2))
    y = np.sin(X[:, 0] / 3.0) + 0.05 * rng.standard_normal(120) + 4.0
    nd = gp.normalizeData(X, y)
    variables = [("l1", 0.1, 10.0), ("l2", 0.1, 10.0), ("sf", 0.1, 10.0), ("sn", 0.02, 1.0)]
    obj = gp.defineGaussianProcess(nd, "SEARD", variables=variables)
    assert not obj.failed and set(obj["DataPreProcessors"]) == {"Input", "Output"}       # BGP:214-218
    th = np.array([1.0, 2.0, 1.0, 0.1])
    want = orc.log_likelihood("se_ard", th, nd["Input"]["NormalizedData"], nd["Output"]["NormalizedData"][:, 0])
    assert obj["LogLikelihoodFunction"](th) == pytest.approx(want, rel=1e-8)
    samples = [{"Point": th, "CrudePosteriorWeight": 1.0, "CrudeLogPosteriorWeight": 0.0}]
    path = str(tmp_path / "gp.npz")
    gp.save_gaussian_process(obj.append({"Samples": samples}), path, theta=th)
    obj2, th2 = gp.load_gaussian_process(path)
    np.testing.assert_array_equal(th2, th)
    pts = nd["Input"]["Function"](X[:7])
    mu, var = obj2["GaussianProcessData"]["HIPHandle"].predict(pts)                      # re-fitted on load
    a = gp.predictFromGaussianProcess(obj.append({"Samples": samples}), pts)
    b = gp.predictFromGaussianProcess(obj2, pts)
    np.testing.assert_allclose(a["Mean"], b["Mean"], rtol=1e-12)
    np.testing.assert_allclose(mu, a["Mean"][0], rtol=1e-12)
    back = nd["Output"]["InverseFunction"](mu)[:, 0]                                     # original units
    assert np.sqrt(np.mean((back - y[:7]) ** 2)) < 0.3


def test_automatic_branch_precision_and_device_rules():
    """BGP:272-292: "LogLikelihoodFunction" -> Automatic selects LogLikelihood[MultinormalDistribution[m, K], {y}]
    (unevaluated -> $MachineLogZero).  On the HIP path that is the same device computation; it must equal the
    MVN log-pdf the oracle evaluates with scipy (the second formulation the reference itself sanctions)."""
    X, y = syn.make_dataset(180, 2)
    variables = [("l1", 0.1, 10.0), ("l2", 0.1, 10.0), ("sf", 0.1, 10.0), ("sn", 0.05, 1.0), ("mu", -1.0, 1.0)]
    obj = gp.defineGaussianProcess((X, y), "Matern52ARD", "Constant", "Constant", variables,
                                   LogLikelihoodFunction="Automatic", Devices=[0])
    assert not obj.failed and obj["LikelihoodBranch"] == "Automatic"
    th = np.array([0.9, 1.4, 1.1, 0.2, 0.15])
    want = orc.log_likelihood_mvn("matern52_ard", th, X, y, "const")
    assert obj["LogLikelihoodFunction"](th) == pytest.approx(want, rel=1e-8)
    Xd = X.copy()
    Xd[3] = Xd[77]                                               # MultinormalDistribution refuses a singular covariance
    bad = gp.defineGaussianProcess((Xd, y), "Matern52ARD", "Constant", "Constant", variables,
                                   LogLikelihoodFunction="Automatic")
    assert bad["LogLikelihoodFunction"]([1.0, 1.0, 1.0, 0.0, 0.0]) == gp.MACHINE_LOG_ZERO
    # Precision -> "Single": fp32 device arithmetic (BASELINE.json cfg 5), 1e-3 against the fp64 oracle
    single = gp.defineGaussianProcess((X, y), "Matern52ARD", "Constant", "Constant", variables, Precision="Single")
    assert single["GaussianProcessData"]["HIPHandle"].dtype == 32
    assert single["LogLikelihoodFunction"](th) == pytest.approx(want, rel=1e-3)
    with pytest.raises(ValueError):
        gp.defineGaussianProcess((X, y), "Matern52ARD", "Constant", "Constant", variables, Precision="Half")


def test_predictive_distribution_forwards_for_gp_objects():
    """BS:1373-1416: predictiveDistribution[obj, inputs] and its "MaximumLikelihood" / "MAP" forms."""
    X, y = syn.make_dataset(120, 1)
    variables = [("l", 0.05, 5.0), ("sf", 0.1, 5.0), ("sn", 0.05, 1.0)]
    obj = gp.defineGaussianProcess((X, y), "SE", variables=variables)
    pts = np.linspace(-1, 1, 6)
    assert gp.predictiveDistribution(obj, pts) is None                        # ::unsampled (BS:1375-1380)
    samples = [{"Point": [0.3, 1.0, 0.1], "CrudePosteriorWeight": 0.2, "LogLikelihood": -10.0, "LogPriorPDF": -1.0},
               {"Point": [0.5, 1.3, 0.2], "CrudePosteriorWeight": 0.5, "LogLikelihood": -12.0, "LogPriorPDF": 3.0},
               {"Point": [0.4, 0.9, 0.3], "CrudePosteriorWeight": 0.3, "LogLikelihood": -11.0, "LogPriorPDF": -1.0}]
    sampled = obj.append({"Samples": samples})
    full = gp.predictiveDistribution(sampled, pts)
    ref = gp.predictFromGaussianProcess(sampled, pts)
    np.testing.assert_array_equal(full["Mean"], ref["Mean"])
    ml = gp.predictiveDistribution(sampled, pts, "MaximumLikelihood")         # TakeLargestBy LogLikelihood
    mo, so = orc.predict_internal("se", samples[0]["Point"], X, y, pts[:, None])
    assert ml["Mean"].shape == (1, 6)
    np.testing.assert_allclose(ml["Mean"][0], mo, rtol=1e-7, atol=1e-9)
    mp = gp.predictiveDistribution(sampled, pts, "MAP")                       # LogLikelihood + LogPriorPDF
    mo, so = orc.predict_internal("se", samples[1]["Point"], X, y, pts[:, None])
    np.testing.assert_allclose(mp["StandardDeviation"][0], so, rtol=1e-7)
    assert gp.predictiveDistribution(sampled) is None                         # no inputs: ::MissGenDist
    # null-kernel object: Normal[m(x*), sn] at every point (BGP:63-89)
    nobj = gp.defineGaussianProcess((X, y), None, "Constant", "Constant", [("sn", 0.05, 2.0), ("mu", -1.0, 1.0)])
    pred = gp.predictFromGaussianProcess(nobj.append({"Samples": [{"Point": [0.7, 0.1], "CrudePosteriorWeight": 1.0}]}), pts)
    assert np.all(pred["Mean"] == 0.1) and np.allclose(pred["StandardDeviation"], 0.7)


def test_covariance_function_listable_and_null_kernel_vector():
    """compiledCovarianceMatrix is Listable (BGP:59): a B x p matrix of thetas gives B matrices; with the null
    kernel covarianceMatrix returns the diagonal as a VECTOR (BGP:27), which matrixInverseAndDet's third form takes."""
    X, y = syn.make_dataset(90, 2)
    variables = [("l1", 0.1, 10.0), ("l2", 0.1, 10.0), ("sf", 0.1, 10.0), ("sn", 0.05, 1.0)]
    obj = gp.defineGaussianProcess((X, y), "SEARD", variables=variables)
    cov = obj["GaussianProcessData", "ModelFunctions", "CovarianceFunction"]
    Th = np.array([[0.8, 1.7, 1.2, 0.3], [1.1, 0.6, 0.9, 0.2], [2.0, 2.0, 0.5, 0.1]])
    Ks = cov(Th)
    assert Ks.shape == (3, 90, 90)
    for b in range(3):
        np.testing.assert_allclose(Ks[b], orc.covariance_matrix("se_ard", Th[b], X), rtol=1e-12)
        np.testing.assert_array_equal(Ks[b], cov(Th[b]))
    nobj = gp.defineGaussianProcess((X, y), None, "Constant", None, [("sn", 0.05, 2.0)])
    diag = nobj["GaussianProcessData", "ModelFunctions", "CovarianceFunction"]([0.7])
    np.testing.assert_allclose(diag, orc.covariance_matrix("null", [0.7], X), rtol=1e-15)
    assert diag.shape == (90,)


def test_define_gaussian_process_with_nugget_and_mean_functions_of_the_point():
    """The reference takes ANY nugget[x] and meanFunction[x] (BGP:37, 300, 113, 408).  Host mirror: callables
    f(X, theta) -> values; the object's closure, covariance, inverse and mixture prediction all follow them."""
    X, y = syn.make_dataset(180, 2)
    variables = [("l1", 0.2, 5.0), ("l2", 0.2, 5.0), ("sf", 0.3, 3.0), ("sn", 0.05, 1.0)]
    nugget = lambda P, th: th[3] ** 2 * (1.0 + P[:, 0] ** 2)          # noqa: E731  heteroscedastic noise
    mean = lambda P, th: 0.2 + 0.5 * P[:, 1]                          # noqa: E731  linear mean
    obj = gp.defineGaussianProcess((X, y), "SEARD", nugget, mean, variables, "Uniform")
    assert not obj.failed                                             # the 100-theta smoke sweep ran through gphip_loglik_batch_pw
    th = np.array([0.8, 1.7, 1.2, 0.3])
    nf = lambda x: nugget(x[None, :], th)[0]                          # noqa: E731
    mf = lambda x: mean(x[None, :], th)[0]                            # noqa: E731
    want = orc.log_likelihood("se_ard", th, X, y, nugget_fn=nf, mean_fn=mf)
    assert obj["LogLikelihoodFunction"](th) == pytest.approx(want, rel=1e-8)
    batch = obj["LogLikelihoodFunction"](np.array([th, th * 1.1]))
    assert batch.shape == (2,) and batch[0] == pytest.approx(want, rel=1e-8)
    fns = obj["GaussianProcessData", "ModelFunctions"]
    assert fns["NuggetFunction"] is nugget and fns["MeanFunction"] is mean
    np.testing.assert_allclose(fns["CovarianceFunction"](th), orc.covariance_matrix("se_ard", th, X, nugget_fn=nf), rtol=1e-12)
    inv = fns["InverseCovarianceFunction"](th)
    K = orc.covariance_matrix("se_ard", th, X, nugget_fn=nf)
    assert inv["LogDet"] == pytest.approx(np.linalg.slogdet(K)[1], rel=1e-9)
    samples = [{"Point": th, "CrudePosteriorWeight": 0.6}, {"Point": th * 1.2, "CrudePosteriorWeight": 0.4}]
    Xs = syn.make_test_points(11, 2)
    res = gp.predictFromGaussianProcess(obj.append({"Samples": samples}), Xs)
    for s, smp in enumerate(samples):
        t = np.asarray(smp["Point"])
        mo, so = orc.predict_internal("se_ard", t, X, y, Xs, nugget_fn=lambda x, t=t: nugget(x[None, :], t)[0],
                                      mean_fn=lambda x, t=t: mean(x[None, :], t)[0])
        np.testing.assert_allclose(res["Mean"][s], mo, rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(res["StandardDeviation"][s], so, rtol=1e-7)


# ---- launch state of a call does not outlive the call ----
_LS_N, _LS_D = 640, 3                              # 5 tile columns: panel = 2 gives three outer panels, panel = 1 five
_LS_TH = syn.default_theta("se_ard", _LS_D)
_LS_THS = _LS_TH[None, :] * (1.0 + 0.05 * np.arange(4))[:, None]
_LS_XS = syn.make_test_points(3, _LS_D)


def _ls_fit_predict(h):
    assert h.fit(_LS_TH) == 0
    return h.predict(_LS_XS)


_LS_CALLS = {
    "loglik": lambda h: h.loglik(_LS_TH),
    "loglik_grad": lambda h: h.loglik_grad(_LS_TH),
    "fit+predict": _ls_fit_predict,
    "solve1": lambda h: (h.solve(np.random.default_rng(1).standard_normal(h.N)),),          # (after fit+predict: the fit is resident)
    "solve8": lambda h: (h.solve(np.random.default_rng(8).standard_normal((h.N, 8))),),
    "samples": lambda h: h.predict_samples(_LS_THS, _LS_XS),
}


def _ls_lookahead(h):
    """a look-ahead multi-kernel factorisation: panel stream, fused first-tile factorisation, LA / REST alternation"""
    assert h.loglik(_LS_TH)[1] == 0


def _ls_sharded(h):
    """a sharded evaluation over the two virtual ranks, a sharded fit and a streamed prediction from it; then local calls only"""
    assert h.loglik(_LS_TH)[1] == 0
    assert h.get_option("last_issue_us") > 0 and h.get_option("last_dist_panel_df") == h.get_option("dist_panel_df")
    assert h.fit(_LS_TH) == 0
    h.predict(_LS_XS)
    h.set_option("shard_min_n", 1 << 30)


@pytest.mark.parametrize("device,opts,retarget", [
    (None, {"dataflow": 0, "panel": 2}, _ls_lookahead),
    (None, {"dataflow": 0, "panel": 2, "latency_gemm": 0}, _ls_lookahead),      # (the 256-thread GEMM shape: the one that takes the fused tile)
    ([0, 0], {"shard_min_n": 0, "panel": 1, "dist_panel_df": 0}, _ls_sharded),
    ([0, 0], {"shard_min_n": 0, "panel": 1, "dist_panel_df": 3}, _ls_sharded),
], ids=["lookahead", "lookahead-fused", "sharded-df0", "sharded-df3"])
def test_launch_state_does_not_outlive_the_call_that_set_it(device, opts, retarget):
    """The per-call fields of a context (targeted stream, workspace override, column-event sinks, fused-tile request, a
    member's slices of the per-point arrays) are set through scopes and are back to their resting values when the call
    returns.  So after calls that retarget launches -- the look-ahead schedule on the panel stream; a sharded evaluation,
    a sharded fit and a streamed prediction over two virtual ranks on device 0 -- every ordinary call gives bit for bit
    (np.array_equal) what a fresh handle with the same options gives; for the group the ordinary calls run locally
    (shard_min_n raised).  Two fresh handles are compared with each other first: every route used here is bit-repeatable,
    the multi-kernel one (dataflow = 0) included.  No fault is injected: the early-return paths are covered by the
    scopes' destructors."""
    X, y = syn.make_dataset(_LS_N, _LS_D)

    def run(used):
        h = _lib.Handle(X, y, "se_ard", device=device)
        for k, v in opts.items():
            h.set_option(k, v)
        if used:
            retarget(h)
        elif "shard_min_n" in opts:
            h.set_option("shard_min_n", 1 << 30)
        res = {name: [np.asarray(a) for a in call(h)] for name, call in _LS_CALLS.items()}
        assert (h.get_option("last_issue_us") > 0) == (used and device is not None)       # the ordinary calls did not shard
        h.close()
        return res

    fresh, again, used = run(False), run(False), run(True)
    for name in _LS_CALLS:
        for a, b in zip(fresh[name], again[name]):
            assert np.array_equal(a, b), ("two fresh handles differ", name, a, b)
    for name in _LS_CALLS:
        for a, b in zip(used[name], fresh[name]):
            assert np.array_equal(a, b), (name, a, b)
