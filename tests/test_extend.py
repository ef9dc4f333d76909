"""gphip_extend without a device: the block identity it rests on, in numpy (tests/extend_reference.py), on the shapes of the device
tests; the refusal case under the library's pivot rule; the symbol and the argument checks that come before any device work."""
import ctypes

import numpy as np
import pytest

import extend_reference as er
from bayesianinference_amd import _lib, build, gaussian_process as gp
from oracle import gp_oracle as orc

CASES = [(k, d, mean, 300, 130) for (k, d, mean) in er.KERNELS] + [("se_ard", 3, "zero", n, m) for (n, m) in er.SHAPES[1:]] + \
        [("se_ard", 3, "zero", er.CHAIN[0], er.CHAIN[1])]


@pytest.mark.parametrize("kname,d,mean,n,m", CASES)
def test_assembled_factor_is_the_cholesky_factor_of_the_concatenated_data(kname, d, mean, n, m):
    kernel, th = er.kernel_of(kname, d), er.theta_of(kname, d, mean)
    X, y, Xn, yn, _ = er.case_data(n, m, d)
    a, b = er.assembled(kernel, th, X, y, Xn, yn, mean), er.direct(kernel, th, X, y, Xn, yn, mean)
    assert a["info"] == 0
    # eps x cond(K) ~ 2e-16 x (N sf^2 / sn^2 = 4e4), over sums of up to 430 terms
    np.testing.assert_allclose(a["L"], b["L"], rtol=0, atol=1e-10)
    np.testing.assert_allclose(a["z"], b["z"], rtol=0, atol=1e-10 * np.abs(b["z"]).max())
    assert abs(a["logdet"] - b["logdet"]) <= 1e-12 * abs(b["logdet"])
    assert abs(a["logp"] - (b["loglik"] - b["loglik_parent"])) <= 1e-10 * abs(b["loglik"])


def test_chain_of_single_points_assembles_the_same_factor():
    n, m = er.CHAIN
    th = er.theta_of("se_ard", 3)
    X, y, Xn, yn, _ = er.case_data(n, m, 3)
    once = er.assembled("se_ard", th, X, y, Xn, yn)
    Xc, yc, logp = X, y, 0.0
    for i in range(m):
        step = er.assembled("se_ard", th, Xc, yc, Xn[i:i + 1], yn[i:i + 1])
        Xc, yc, logp = np.vstack([Xc, Xn[i:i + 1]]), np.concatenate([yc, yn[i:i + 1]]), logp + step["logp"]
    np.testing.assert_allclose(step["L"], once["L"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(step["z"], once["z"], rtol=0, atol=1e-11 * np.abs(once["z"]).max())
    assert abs(logp - once["logp"]) <= 1e-11 * abs(once["logp"])


def test_refusal_case_under_the_pivot_rule():
    kernel, mean, th, X, y, Xn, yn = er.refusal_case()
    tol = er.pivot_tolerance(th[1] ** 2, th[2] ** 2)
    assert tol < 2e-14
    K = orc.covariance_matrix(kernel, th, X, mean)
    assert np.array_equal(K, np.eye(64))                          # K = I to the last bit: the parent factors
    assert er.pivot_cholesky(K, tol)[1] == 0
    assert er.assembled(kernel, th, X, y, Xn, yn, mean)["info"] == 1          # Sigma: second pivot 0 <= tol
    _, S, _ = er.reference(kernel, th, X, y, Xn, mean)
    assert S[1, 1] - S[1, 0] ** 2 / S[0, 0] <= tol
    Kc = orc.covariance_matrix(kernel, th, np.vstack([X, Xn]), mean)
    assert er.pivot_cholesky(Kc, tol)[1] == 1                     # and so does the fresh handle's K on the concatenated data
    # one new point alone passes
    assert er.assembled(kernel, th, X, y, Xn[:1], yn[:1], mean)["info"] == 0


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_symbol_and_null_arguments(lib):
    assert "gphip_extend" in _lib.declared_symbols() and "gphip_extend" in _lib._SIGNATURES and hasattr(lib, "gphip_extend")
    X, y = np.zeros((3, 1)), np.zeros(3)
    out, logp, info = ctypes.c_void_p(7), ctypes.c_double(5.0), ctypes.c_int(-1)
    dp = ctypes.POINTER(ctypes.c_double)
    assert lib.gphip_extend(None, X.ctypes.data, y.ctypes.data_as(dp), 3, ctypes.byref(out), ctypes.byref(logp), ctypes.byref(info)) == 1
    assert out.value == 7 and logp.value == 5.0 and info.value == -1          # nothing written


def test_python_layer_validates_before_device_work(lib):
    h = object.__new__(_lib.Handle)
    h._lib, h._h, h.d, h.N, h.p = lib, None, 2, 5, 4
    for Xn, yn in ((np.zeros((0, 2)), np.zeros(0)), (np.zeros((4, 3)), np.zeros(4)), (np.zeros((4, 2)), np.zeros(3))):
        with pytest.raises(_lib.GphipError) as e:
            h.extend(Xn, yn)
        assert e.value.status == 2
    assert gp.extendGaussianProcess(h, "not data") is None
    assert gp.extendGaussianProcess(h, (np.zeros((4, 3)), np.zeros(4))) is None       # wrong input dimension
    assert gp.extendGaussianProcess(h, (np.zeros((4, 2)), np.zeros((4, 2)))) is None  # two output columns
