"""Gradients of the predictive mean and variance in the test inputs, the part that needs no GPU: pins the numpy references of
tests/predict_grad_reference.py (exact and sparse object) against torch's reverse mode through the prediction restated in torch
(float64, CPU), checks them against central differences of the numpy prediction, and checks the C ABI's boundary.

The two routes have to agree to 1e-10 of max |reference| on every pinned case: a case that does not is to be changed, not the
bar."""
import ctypes
import time

import numpy as np
import pytest

import predict_grad_reference as pg
import sparse_reference as ref
from bayesianinference_amd import _lib, build

ROUTE_BAR = 1e-10
# 4th-order central differences with a step of 1e-4 x max(|x|, 0.1): truncation ~h^4 f^(5) / 30 and rounding ~eps |f| / h of the
# prediction itself (|mean|, var ~ 1, K^-1 amplifies the rounding of var by cond(K) ~ (N sf^2 + sn^2) / sn^2 ~ 2e4), so the
# quotient is good to ~1e-16 x 2e4 / 1e-5 ~ 2e-7 absolute; gradients are O(1).  A sanity check at 1e-5 of max |gradient|, not the pin.
QUOTIENT_BAR = 1e-5

IDS = [pg.case_id(c) for c in pg.CASES]


def _err(g, want):
    return float(np.abs(g - want).max() / np.abs(want).max())


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


@pytest.mark.parametrize("name,d,mean", pg.CASES, ids=IDS)
def test_exact_routes_agree(name, d, mean):
    t0 = time.time()
    c = pg.case_reference(name, d, mean)
    ag = pg.exact_autograd(name, c["theta"], c["X"], c["y"], c["Xs"], mean)
    em, ev = _err(ag["dmean"], c["dmean"]), _err(ag["dvar"], c["dvar"])
    print(f"{name} d={d} {mean}: numpy against autograd, dmean {em:.3e} dvar {ev:.3e} of max |.| {np.abs(c['dmean']).max():.4g} / "
          f"{np.abs(c['dvar']).max():.4g} ({time.time() - t0:.1f} s)")
    assert c["dmean"].shape == (pg.M, d) and c["dvar"].shape == (pg.M, d)
    assert np.all(np.isfinite(c["dmean"])) and np.all(np.isfinite(c["dvar"]))
    assert np.array_equal(c["Xs"][pg.COINCIDE[0]], c["X"][pg.COINCIDE[1]])          # the coinciding test point is there
    assert em <= ROUTE_BAR and ev <= ROUTE_BAR


@pytest.mark.parametrize("name,d,mean", pg.CASES, ids=IDS)
def test_sparse_routes_agree(name, d, mean):
    c = pg.sparse_case_reference(name, d, mean)
    ag = pg.sparse_autograd(name, c["theta"], c["X"], c["y"], c["Z"], c["jitter"], c["Xs"], mean)
    em, ev = _err(ag["dmean"], c["dmean"]), _err(ag["dvar"], c["dvar"])
    print(f"sparse {name} d={d} {mean} m={pg.SPARSE_M}: numpy against autograd, dmean {em:.3e} dvar {ev:.3e}")
    assert em <= ROUTE_BAR and ev <= ROUTE_BAR


def test_sparse_routes_agree_with_two_tiles_of_inducing_points():
    name, d, mean, m = pg.SPARSE_TWO_TILES
    c = pg.sparse_case_reference(name, d, mean, m)
    ag = pg.sparse_autograd(name, c["theta"], c["X"], c["y"], c["Z"], c["jitter"], c["Xs"], mean)
    em, ev = _err(ag["dmean"], c["dmean"]), _err(ag["dvar"], c["dvar"])
    print(f"sparse {name} d={d} {mean} m={m}: numpy against autograd, dmean {em:.3e} dvar {ev:.3e}")
    assert em <= ROUTE_BAR and ev <= ROUTE_BAR


def _entries(d):
    rng = np.random.RandomState(0)
    return [(pg.COINCIDE[0], 0)] + [(int(rng.randint(pg.M)), int(rng.randint(d))) for _ in range(7)]


@pytest.mark.parametrize("name,d,mean", pg.CASES, ids=IDS)
def test_exact_reference_against_central_differences(name, d, mean):
    c = pg.case_reference(name, d, mean)
    quot = pg.differences(pg.exact_predict(name, c["theta"], c["X"], c["y"], mean), c["Xs"], _entries(d))
    em = max(abs(c["dmean"][e] - v[0]) for e, v in quot.items()) / np.abs(c["dmean"]).max()
    ev = max(abs(c["dvar"][e] - v[1]) for e, v in quot.items()) / np.abs(c["dvar"]).max()
    print(f"{name} d={d} {mean}: 8 difference quotients differ by {em:.3e} (dmean) {ev:.3e} (dvar)")
    assert em <= QUOTIENT_BAR and ev <= QUOTIENT_BAR


@pytest.mark.parametrize("name,d,mean", [pg.CASES[1], pg.CASES[3]], ids=[IDS[1], IDS[3]])
def test_sparse_reference_against_central_differences(name, d, mean):
    c = pg.sparse_case_reference(name, d, mean)

    def predict(P):
        return ref.predict_formulas(name, c["theta"], c["X"], c["y"], c["Z"], c["jitter"], P, mean)
    quot = pg.differences(predict, c["Xs"], _entries(d))
    em = max(abs(c["dmean"][e] - v[0]) for e, v in quot.items()) / np.abs(c["dmean"]).max()
    ev = max(abs(c["dvar"][e] - v[1]) for e, v in quot.items()) / np.abs(c["dvar"]).max()
    print(f"sparse {name} d={d} {mean}: 8 difference quotients differ by {em:.3e} (dmean) {ev:.3e} (dvar)")
    assert em <= QUOTIENT_BAR and ev <= QUOTIENT_BAR


def test_reference_mean_and_variance_are_the_oracles():
    name, d, mean = pg.CASES[1]
    c = pg.case_reference(name, d, mean)
    mu, sd = pg.orc.predict_internal(name, c["theta"], c["X"], c["y"], c["Xs"], mean)
    assert np.allclose(c["mean"], mu, rtol=0, atol=1e-12) and np.allclose(c["var"], sd * sd, rtol=0, atol=1e-12)


def test_entry_points_are_declared_exported_and_have_signatures(lib):
    for sym in ("gphip_predict_grad", "gphip_sparse_predict_grad"):
        assert sym in _lib.declared_symbols(), sym
        assert sym in _lib._SIGNATURES, sym
        assert hasattr(lib, sym), sym
    assert hasattr(_lib.Handle, "predict_grad") and hasattr(_lib.SparseHandle, "predict_grad")
    from bayesianinference_amd import gaussian_process as gp
    assert callable(gp.predictGradientFromGaussianProcess) and callable(gp.predictGradientFromSparseGaussianProcess)


def test_null_handles_come_back_before_any_device_work(lib):
    dp = ctypes.POINTER(ctypes.c_double)
    xs, g = np.zeros(6), np.zeros(6)
    assert lib.gphip_predict_grad(None, xs.ctypes.data, 2, None, None, g.ctypes.data_as(dp), None) == 1
    assert lib.gphip_sparse_predict_grad(None, xs.ctypes.data, 2, None, None, g.ctypes.data_as(dp), None) == 1
    assert lib.gphip_predict_grad(None, None, 2, None, None, None, None) == 1
    assert np.all(g == 0.0)
