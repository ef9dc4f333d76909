"""CPU side of the sparse object's joint predictive distribution (gphip_sparse_predict_cov / _draws / _logpdf): the two numpy
routes of tests/sparse_joint_reference.py agree on the cases the device test uses, the new symbols are exported and declared, the
argument checks that need no device, and the Python layer's refusals."""
import ctypes as C

import numpy as np
import pytest

import sparse_joint_reference as jref
import sparse_reference as ref
from bayesianinference_amd import _lib, gaussian_process as gp
from bayesianinference_amd.gaussian_process import inferenceObject

ERR_ARG = 1                                    # GPHIP_ERR_ARG (include/gphip.h)
NEW = ("gphip_sparse_predict_cov", "gphip_sparse_predict_draws", "gphip_sparse_predict_logpdf")


@pytest.mark.parametrize("case", jref.CASES + [jref.STRIPS, jref.DRAWS], ids=lambda c: c[0])
def test_the_two_routes_agree_and_the_diagonal_is_the_pointwise_variance(case):
    _, n, d, m, M, name, mean = case
    X, y, Z, Xs, _, kernel, th, jit = jref.case_data(n, d, m, M, name, mean)
    for latent in (False, True):
        mu_a, S_a = jref.case_reference(n, d, m, M, name, mean, latent)
        mu_b, S_b = jref.joint_definition(kernel, th, X, y, Z, jit, Xs, mean, latent)
        pm, pv = ref.predict_formulas(kernel, th, X, y, Z, jit, Xs, mean, latent)
        es, em = np.abs(S_a - S_b).max(), np.abs(mu_a - mu_b).max()
        print(f"{case[0]} latent={latent}: routes differ by {es:.1e} (Sigma) {em:.1e} (mu)")
        assert es <= 1e-12 and em <= 1e-12
        assert np.abs(np.diag(S_a) - pv).max() <= 1e-14 and np.abs(mu_a - pm).max() <= 1e-14
    sn2, _ = ref.noise_and_mean(kernel, th, d, mean)
    S_l = jref.case_reference(n, d, m, M, name, mean, True)[1]
    S_n = jref.case_reference(n, d, m, M, name, mean, False)[1]
    assert np.abs(S_n - S_l - sn2 * np.eye(M)).max() <= 1e-14


def test_new_symbols_are_exported_and_declared():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.declared_symbols()
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and fn.argtypes is not None
    assert len(lib.gphip_sparse_predict_cov.argtypes) == 6
    assert len(lib.gphip_sparse_predict_draws.argtypes) == 10
    assert len(lib.gphip_sparse_predict_logpdf.argtypes) == 6
    for meth in ("predict_cov", "predict_draws", "predict_logpdf"):
        assert callable(getattr(_lib.SparseHandle, meth))


def test_null_arguments_are_refused_without_a_device():
    lib = _lib.load()
    x, out, info = np.zeros((4, 2)), np.zeros(16), C.c_int(7)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))                         # noqa: E731
    assert lib.gphip_sparse_predict_cov(None, x.ctypes.data, 4, 0, dp(out), dp(out)) == ERR_ARG
    assert lib.gphip_sparse_predict_draws(None, x.ctypes.data, 4, 1, 2, 0, None, -1.0, dp(out), C.byref(info)) == ERR_ARG
    assert lib.gphip_sparse_predict_logpdf(None, x.ctypes.data, 4, dp(out), dp(out), C.byref(info)) == ERR_ARG
    assert info.value == 7 and not out.any()


def test_python_layer_refuses_what_is_not_a_sampled_sparse_object():
    pts = np.linspace(-1.0, 1.0, 5)
    th = np.array([0.3, 1.0, 0.1])
    failed = inferenceObject(None)
    plain = inferenceObject({"Data": (np.zeros((3, 1)), np.zeros((3, 1)))})            # neither a GP nor a sparse GP object
    unsampled = inferenceObject({"Data": (np.zeros((3, 1)), np.zeros((3, 1))), "Jitter": -1.0,
                                 "SparseGaussianProcessData": {"HIPHandle": None}})
    for obj in (None, failed, plain):
        assert gp.predictJointFromSparseGaussianProcess(obj, pts, th) is None
        assert gp.sparsePredictiveLogDensity(obj, (pts, np.sin(pts)), th) is None
        assert gp.gaussianProcessFunctionSamples(obj, pts, 3) is None
    assert gp.gaussianProcessFunctionSamples(unsampled, pts, 3) is None
    # bad points / outputs of the wrong length are refused before the handle is touched
    assert gp.predictJointFromSparseGaussianProcess(unsampled, None, th) is None
    assert gp.sparsePredictiveLogDensity(unsampled, (pts, np.sin(pts)[:3]), th) is None
