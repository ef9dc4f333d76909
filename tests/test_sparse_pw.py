"""The numpy references of the sparse GP with point-dependent noise and mean (tests/sparse_pw_reference.py), pinned on the CPU:
the two routes against each other on every device case of tests/test_gpu_sparse_pw.py at the bars of tests/test_gpu_sparse.py
(cond(K_uu) <= 1e10, routes <= 1e-10), constant arrays against the constant reference (<= 1e-12), a chunked sum, and the guards of
the Python layer that need no device."""
import numpy as np
import pytest

import sparse_pw_reference as pw
import sparse_reference as ref
from bayesianinference_amd import _lib, gaussian_process as gp, synthetic as syn


def _rel(a, b):
    return abs(a - b) / abs(b)


def _case(name, n, d, m, mean):
    X, y = syn.make_dataset(n, d)
    kernel, th = pw.kernel_of(name, d), pw.theta(name, d, mean)
    Z = pw.inducing(X, m, syn.make_test_points(max(m - n, 1), d))
    sn2, _ = ref.noise_and_mean(kernel, th, d, mean)
    return X, y, kernel, th, Z, sn2


@pytest.mark.parametrize("name,n,d,m,mean", pw.CASES)
def test_routes_agree_on_the_device_cases(name, n, d, m, mean):
    X, y, kernel, th, Z, sn2 = _case(name, n, d, m, mean)
    nu, mv = pw.noise(X, sn2), pw.trend(X)
    assert nu.min() >= 0.25 * sn2 * (1 - 1e-12) and nu.max() <= 4.0 * sn2 * (1 + 1e-12) and nu.max() / nu.min() > 8.0
    assert np.all(np.diff(nu[:64]) != 0.0)                       # the weight differs from index to index inside a 16-wide stage
    cond = np.linalg.cond(ref.kuu_factor(kernel, th, Z, pw.JITTER, mean)[1])
    a = pw.bound_formulas(kernel, th, X, y, Z, pw.JITTER, mv, nu, mean)
    b = pw.bound_definition(kernel, th, X, y, Z, pw.JITTER, mv, nu, mean)
    ch = pw.bound_formulas(kernel, th, X, y, Z, pw.JITTER, mv, nu, mean, chunk=512)
    Xs = syn.make_test_points(77, d)
    errs = []
    for latent in (False, True):
        m1, v1 = pw.predict_formulas(kernel, th, X, y, Z, pw.JITTER, Xs, mv, nu, pw.trend(Xs), pw.noise(Xs, sn2), mean, latent)
        m2, v2 = pw.predict_definition(kernel, th, X, y, Z, pw.JITTER, Xs, mv, nu, pw.trend(Xs), pw.noise(Xs, sn2), mean, latent)
        errs += [np.abs(m1 - m2).max() / np.abs(y).max(), np.abs(v1 - v2).max() / float(ref.kdiag(kernel, th, X, mean).max())]
    print(f"{name} N={n} d={d} m={m}: cond(K_uu) {cond:.2e} routes {_rel(a['F'], b):.1e} chunked {_rel(ch['F'], a['F']):.1e} "
          f"prediction routes {max(errs):.1e}")
    assert cond <= 1e10 and _rel(a["F"], b) <= 1e-10
    assert _rel(ch["F"], a["F"]) <= 1e-12 and np.allclose(ch["parts"], a["parts"], rtol=1e-12, atol=0.0)
    assert max(errs) <= 1e-10
    # each array alone: the other is the constant of theta
    for ma, na in ((mv, None), (None, nu)):
        assert _rel(pw.bound_formulas(kernel, th, X, y, Z, pw.JITTER, ma, na, mean)["F"],
                    pw.bound_definition(kernel, th, X, y, Z, pw.JITTER, ma, na, mean)) <= 1e-10


@pytest.mark.parametrize("name,n,d,m,mean", pw.CASES)
def test_constant_arrays_reproduce_the_constant_reference(name, n, d, m, mean):
    X, y, kernel, th, Z, sn2 = _case(name, n, d, m, mean)
    _, mu = ref.noise_and_mean(kernel, th, d, mean)
    want = ref.bound_formulas(kernel, th, X, y, Z, pw.JITTER, mean)
    for ma, na in ((None, None), (np.full(n, mu), np.full(n, sn2))):
        got = pw.bound_formulas(kernel, th, X, y, Z, pw.JITTER, ma, na, mean)
        assert _rel(got["F"], want["F"]) <= 1e-12
        # B here = B there / sn^2: the six parts are the five converted
        ld, ctc, rtr, tr, skk = want["parts"]
        conv = np.array([ld - m * np.log(sn2), ctc / sn2, rtr / sn2, tr / sn2, skk / sn2, n * np.log(sn2)])
        assert np.allclose(got["parts"], conv, rtol=1e-10, atol=0.0)
    Xs = syn.make_test_points(77, d)
    for latent in (False, True):
        m1, v1 = pw.predict_formulas(kernel, th, X, y, Z, pw.JITTER, Xs, mean=mean, latent=latent)
        m2, v2 = ref.predict_formulas(kernel, th, X, y, Z, pw.JITTER, Xs, mean, latent)
        assert np.abs(m1 - m2).max() <= 1e-12 * np.abs(y).max() and np.abs(v1 - v2).max() <= 1e-12 * pw.SF ** 2 * 4


def test_four_decades_of_noise_keep_the_routes_together():
    for name, n, d, m, mean in (("se_ard", 1333, 3, 150, "zero"), ("se_ard", 900, 2, 100, "zero")):
        X, y, kernel, th, Z, sn2 = _case(name, n, d, m, mean)
        nu = pw.noise_decades(X, sn2)
        assert nu.max() / nu.min() > 5e3
        a = pw.bound_formulas(kernel, th, X, y, Z, pw.JITTER, None, nu, mean)
        b = pw.bound_definition(kernel, th, X, y, Z, pw.JITTER, None, nu, mean)
        print(f"N={n}: routes {_rel(a['F'], b):.1e}, cond(B) {np.linalg.cond(a['LB']) ** 2:.1e}")
        assert _rel(a["F"], b) <= 1e-10


def test_parameter_count_is_host_logic():
    assert _lib.num_params("se_ard", 2, "zero") == 4 and _lib.num_params("se_ard", 3, "const") == 6
    assert _lib.num_params("se_ard*matern52_ard+const", 2, "zero") == 8 and _lib.num_params("rq_ard", 4, "const") == 8
    assert _lib.num_params(pw.kernel_of("custom", 3), 3, "const") == 6
    with pytest.raises(_lib.GphipError):
        _lib.num_params("no_such_kernel", 2, "zero")


def test_define_sparse_gaussian_process_refuses_a_wrong_count_for_callables_without_a_device():
    X, y = np.zeros((4, 2)), np.zeros(4)
    three = [("l1", 0, 1), ("l2", 0, 1), ("sf", 0, 1)]
    for kw in ({"nugget": lambda P, th: np.ones(len(P))}, {"meanFunction": lambda P, th: np.zeros(len(P))}):
        with pytest.raises(ValueError, match="needs 4"):
            gp.defineSparseGaussianProcess((X, y), "SEARD", 2, variables=three, **kw)
    with pytest.raises(ValueError, match="needs 5"):                # the constant mean keeps its mu
        gp.defineSparseGaussianProcess((X, y), "SEARD", 2, meanFunction="Constant", variables=three)
    with pytest.raises(ValueError):
        gp.defineSparseGaussianProcess((X, y), "SEARD", 2, nugget="Linear", variables=three)
    with pytest.raises(ValueError):
        gp.defineSparseGaussianProcess((X, y), "SEARD", 2, nugget=3.0, variables=three)
