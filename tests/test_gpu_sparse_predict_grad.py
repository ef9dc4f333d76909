"""gphip_sparse_predict_grad on the device -- the gradients of the sparse object's predictive mean and variance in the test inputs --
against the CPU references of tests/predict_grad_reference.py (pinned by tests/test_predict_grad.py) and, for the default
jitter, against the extended-precision fixture tests/golden/predict_grad_mpmath.npz (scripts/make_predict_grad_golden.py).

N = 300, M = 130, m = 40 inducing points (m_pad = 128; one case with m = 200: two tiles), jitter = 1e-6 sf^2; the bar is 1e-8
of max |reference|.  With the default jitter cond(K_uu) is 1.6e11 and the float64 reference itself is only good to a few
1e-11: there the bar is 10 x the reference's own measured disagreement with the 30-digit evaluation.  Errors measured on an
MI355X are in DESIGN.md section 8j."""
import os

import numpy as np
import pytest

import predict_grad_reference as pg
from bayesianinference_amd import _lib, gaussian_process as gp

pytestmark = pytest.mark.gpu

BAR = 1e-8
IDS = [pg.case_id(c) for c in pg.CASES]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_grad_mpmath.npz")
SE_ARD_BODY = "T s = 0; for (int k = 0; k < D; ++k) { const T u = (X(k) - Y(k)) / P(k); s += u * u; } return P(D) * P(D) * exp((T)-0.5 * s);"


def _err(g, want):
    return float(np.abs(g - want).max() / np.abs(want).max())


def _fitted(c, jitter=None, opts=None):
    h = _lib.SparseHandle(c["X"], c["y"], c["Z"], c["kernel"], c["mean_kind"])
    for k, v in (opts or {}).items():
        h.set_option(k, v)
    assert h.fit(c["theta"], c["jitter"] if jitter is None else jitter) == 0
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
    c = pg.sparse_case_reference(name, d, mean)
    h = _fitted(c)
    pm, pv = h.predict(c["Xs"])
    out = h.predict_grad(c["Xs"])
    h.close()
    assert out[2].shape == (pg.M, d) and out[3].shape == (pg.M, d)
    _check(c, out, f"{name} d={d} {mean} m={pg.SPARSE_M}")
    assert _err(out[0], pm) <= 1e-13 and _err(out[1], pv) <= 1e-13          # gphip_sparse_predict's, to rounding
    assert _err(out[0], c["mean"]) <= BAR and _err(out[1], c["var"]) <= BAR


def test_two_tiles_of_inducing_points_one_point_and_no_variance():
    name, d, mean, m = pg.SPARSE_TWO_TILES
    c = pg.sparse_case_reference(name, d, mean, m)
    h = _fitted(c)
    full = h.predict_grad(c["Xs"])
    one = h.predict_grad(c["Xs"][:1])
    mean_only = h.predict_grad(c["Xs"], variance=False)
    h.close()
    _check(c, full, f"{name} m={m}")
    _check(c, one, "M = 1")
    assert mean_only[3] is None and np.array_equal(mean_only[2], full[2])   # dvar = NULL: dmean is the same bytes


def test_default_jitter_against_extended_precision():
    """cond(K_uu) = 1.6e11.  The float64 reference differs from the 30-digit evaluation by 2.6e-11 (dmean) and 3.5e-11 (dvar) of
    max |.| (stored in the fixture); the device's bar is 10 x that.  Measured on an MI355X: see DESIGN.md section 8j."""
    g = np.load(GOLDEN)
    name, d, mean = pg.CASES[0]
    assert str(g["kernel"]) == name and int(g["d"]) == d and int(g["m"]) == pg.SPARSE_M
    c = pg.sparse_case_reference(name, d, mean, pg.SPARSE_M, None)
    assert abs(c["jitter"] - float(g["jitter"])) <= 1e-15 * c["jitter"]
    h = _fitted(c, jitter=-1.0)
    assert abs(h.get_option("last_jitter") - c["jitter"]) <= 1e-12 * c["jitter"]
    out = h.predict_grad(c["Xs"])
    h.set_option("sparse_pgrad_refine", 0)
    plain = h.predict_grad(c["Xs"])
    h.close()
    em, ev = _err(out[2], g["dmean"]), _err(out[3], g["dvar"])
    pm, pv = _err(plain[2], g["dmean"]), _err(plain[3], g["dvar"])
    bm, bv = 10.0 * float(g["float64_dmean_error"]), 10.0 * float(g["float64_dvar_error"])
    print(f"cond(K_uu) {float(g['cond_kuu']):.3e}: device against {g['arithmetic']}: dmean {em:.3e} (bar {bm:.3e}) dvar {ev:.3e} (bar {bv:.3e}); "
          f"without the refined substitution: dmean {pm:.3e} dvar {pv:.3e}; float64 reference {float(g['float64_dmean_error']):.3e} "
          f"{float(g['float64_dvar_error']):.3e}")
    assert em <= bm and ev <= bv


def test_strips_and_chunks_agree_and_repeat_bit_for_bit():
    name, d, mean = pg.CASES[5]                                   # two terms
    c = pg.sparse_case_reference(name, d, mean)
    h = _fitted(c)
    F0, _ = h.bound(c["theta"], c["jitter"])
    assert h.fit(c["theta"], c["jitter"]) == 0
    p0 = h.predict(c["Xs"])
    base = h.predict_grad(c["Xs"])
    for key, opts, ns in (("split 1", {"predict_grad_split": 1}, 1), ("split 3", {"predict_grad_split": 3}, 1),
                          ("chunk 128", {"predict_grad_chunk": 128}, 1)):
        h.set_option("predict_grad_split", 0)
        h.set_option("predict_grad_chunk", 0)
        for k, v in opts.items():
            h.set_option(k, v)
        a = h.predict_grad(c["Xs"])
        b = h.predict_grad(c["Xs"])
        _check(c, a, key)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), key                 # the same bytes
        assert int(h.get_option("last_predict_grad_nsplit")) == ns                  # m = 40: one slab of 64 inducing points
        if "predict_grad_chunk" in opts:
            assert int(h.get_option("last_predict_grad_chunk")) == 128
        for x, y in zip(a, base):                                                   # to rounding: eps x cond(K_uu) ~ 1e-16 x 1e6
            assert np.abs(x - y).max() <= 1e-9 * np.abs(y).max(), key
    p1 = h.predict(c["Xs"])
    assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1])            # the fit is untouched
    h.close()
    h = _fitted(c)
    h.predict_grad(c["Xs"])
    assert h.bound(c["theta"], c["jitter"])[0] == F0                                # and so is the bound
    h.close()


def test_strips_over_two_tiles_of_inducing_points():
    name, d, mean, m = pg.SPARSE_TWO_TILES
    c = pg.sparse_case_reference(name, d, mean, m)
    h = _fitted(c)
    for split, want in ((0, 4), (1, 1), (3, 2)):                  # 200 inducing points: four slabs of 64; 3 strips -> 2 slabs each -> 2
        h.set_option("predict_grad_split", split)
        _check(c, h.predict_grad(c["Xs"]), f"m = {m}, split {split}")
        assert int(h.get_option("last_predict_grad_nsplit")) == want
    h.close()


@pytest.mark.parametrize("opts", [{}, {"dataflow": 0}], ids=["dataflow-fit", "lookahead-fit"])
def test_both_substitution_routes(opts):
    name, d, mean = pg.CASES[4]
    c = pg.sparse_case_reference(name, d, mean)
    h = _fitted(c, opts=opts)
    out = h.predict_grad(c["Xs"])
    h.close()
    _check(c, out, f"{name} {opts}")


def test_statuses():
    name, d, mean = pg.CASES[1]
    c = pg.sparse_case_reference(name, d, mean)
    Xs = c["Xs"]
    h = _lib.SparseHandle(c["X"], c["y"], c["Z"], name, mean)
    with pytest.raises(_lib.GphipError) as e:
        h.predict_grad(Xs)
    assert e.value.status == 4                                    # before a fit
    assert h.fit(c["theta"], c["jitter"]) == 0
    h.predict_grad(Xs)
    h.bound_batch(np.vstack([c["theta"], c["theta"]]), c["jitter"])
    with pytest.raises(_lib.GphipError) as e:
        h.predict_grad(Xs)
    assert e.value.status == 4                                    # the batch dropped the fit
    assert h.fit_pw(c["theta"], c["jitter"], nugget_train=np.full(pg.N, pg.SN ** 2)) == 0
    with pytest.raises(_lib.GphipError) as e:
        h.predict_grad(Xs)
    assert e.value.status == 6                                    # a fit with a point-dependent array
    assert h.fit_pw(c["theta"], c["jitter"]) == 0                 # both arrays NULL: the plain fit
    _check(c, h.predict_grad(Xs), "after fit_pw with both arrays NULL")
    h.close()
    custom = _lib.SparseHandle(c["X"], c["y"], c["Z"], _lib.CustomKernel(SE_ARD_BODY, d + 1), mean)
    assert custom.fit(c["theta"], c["jitter"]) == 0
    with pytest.raises(_lib.GphipError) as e:
        custom.predict_grad(Xs)
    assert e.value.status == 6
    custom.close()


def test_python_layer():
    name, d, mean = pg.CASES[0]                                   # se, d = 1, zero mean
    c = pg.sparse_case_reference(name, d, mean)
    obj = gp.defineSparseGaussianProcess((c["X"], c["y"][:, None]), "se", c["Z"], variables=[("l", 0.05, 2.0), ("sf", 0.1, 5.0), ("sn", 0.01, 1.0)],
                                         Jitter=c["jitter"])
    pts = c["Xs"][:40, 0]
    out = gp.predictGradientFromSparseGaussianProcess(obj, pts, c["theta"])
    marg = gp.predictFromSparseGaussianProcess(obj, pts, c["theta"])
    assert out["MeanGradient"].shape == (40, 1)
    assert _err(out["MeanGradient"], c["dmean"][:40]) <= BAR and _err(out["VarianceGradient"], c["dvar"][:40]) <= BAR
    np.testing.assert_allclose(out["Mean"], marg["Mean"][0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(out["StandardDeviation"], marg["StandardDeviation"][0], rtol=1e-10)
    obj = obj.append({"Samples": [{"Point": c["theta"], "CrudePosteriorWeight": 0.7},
                                  {"Point": np.array([0.6, 0.7, 0.2]), "CrudePosteriorWeight": 0.3}]})
    samp = gp.predictGradientFromSparseGaussianProcess(obj, pts)
    assert samp["VarianceGradient"].shape == (2, 40, 1) and np.allclose(samp["Weights"], [0.7, 0.3])
    assert _err(samp["MeanGradient"][0], c["dmean"][:40]) <= BAR
    want = pg.sparse("se", np.array([0.6, 0.7, 0.2]), c["X"], c["y"], c["Z"], c["jitter"], c["Xs"][:40], "zero")
    assert _err(samp["VarianceGradient"][1], want["dvar"]) <= BAR
