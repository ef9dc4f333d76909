"""The batched likelihood gradient on the device (gphip_loglik_grad_batch): every row against the one-theta call on the same
handle and against the CPU oracle, for every reduction kernel the batch carries the slot through (the specialised SE / Matern
forms, DD = 0, the general form and its windows beyond KB_LDS_MAXD dimensions, a run-time compiled function); ragged groups, row
isolation, repeatability, state and statuses, and the use laplace.approximateEvidence makes of the 2-D closure.

Tolerances.  Batch against one-theta, fp64: 1e-9 (the bar tests/test_gpu_parity.py sets between two routes to U = L^-T: the two
calls differ in the factorisation schedule and the U route only); fp32: 2e-3, the same test's.  Batch against the oracle: what
the existing one-theta test of the family uses at these shapes (1e-7 in test_loglik_gradient_matches_oracle, 2e-6 in
tests/test_gpu_kernels.py); the shapes no existing test holds the oracle's difference quotient to (one tile exactly, d = 40) are
checked against the one-theta call only."""
import functools

import numpy as np
import pytest

from bayesianinference_amd import _lib, gaussian_process as gp, laplace, synthetic as syn
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

SE_ARD_BODY = "T s = 0; for (int k = 0; k < D; ++k) { const T u = (X(k) - Y(k)) / P(k); s += u * u; } return P(D) * P(D) * exp((T)-0.5 * s);"


def se_ard_fn(A, B, p):
    d = A.shape[-1]
    return p[d] ** 2 * np.exp(-0.5 * (((A - B) / p[:d]) ** 2).sum(-1))


def close(a, b, n=1, rtol=1e-8):                     # the suite's bar for values (tests/test_gpu_parity.py)
    return abs(a - b) <= rtol * max(abs(b), float(n))


# (kernel, d, N, mean, theta or None = default_theta, leading length scales, oracle tolerance or None = one-theta call only)
CASES = {
    "se_ard_d3": ("se_ard", 3, 300, "zero", None, 3, 1e-7),
    "matern52_second_tile_one_row": ("matern52", 2, 129, "zero", None, 1, 1e-7),
    "se_const_mean": ("se", 1, 200, "const", None, 1, 1e-7),
    "se_ard_d11_dd0": ("se_ard", 11, 150, "zero", None, 11, 1e-7),
    "se_ard_d16_one_tile": ("se_ard", 16, 128, "zero", None, 16, None),
    "composed_general": ("se_ard+matern32", 2, 120, "zero", [0.6, 1.4, 0.8, 1.9, 0.7, 0.2], 2, 2e-6),
    "rq_ard_general": ("rq_ard", 3, 120, "zero", [0.8, 1.1, 1.5, 0.6, 0.9, 0.2], 3, 2e-6),
    "se_ard_d40_windows": ("se_ard", 40, 150, "zero", None, 40, None),
}
B_MAX = 5


def theta_rows(kernel, d, mean, theta, nl, B=B_MAX, dtype="f64"):
    th = np.array(theta, dtype=np.float64) if theta is not None else syn.default_theta(kernel, d, dtype=dtype)
    if theta is None and mean == "const":
        th = np.append(th, 0.2)
    rows = np.tile(th, (B, 1))
    for s in range(B):
        rows[s, :nl] *= 1.0 + 0.07 * s               # row s: the length scales times 1 + 0.07 s
    return rows


@functools.lru_cache(maxsize=None)
def reference(name):
    """data, the theta rows and the oracle's values (and gradients where the oracle is the bar), computed once per case"""
    kernel, d, n, mean, theta, nl, otol = CASES[name]
    X, y = syn.make_dataset(n, d)
    Th = theta_rows(kernel, d, mean, theta, nl)
    ll = np.array([orc.log_likelihood(kernel, t, X, y, mean) for t in Th])
    grads = np.array([orc.log_likelihood_grad(kernel, t, X, y, mean) for t in Th]) if otol is not None else None
    for a in (X, y, Th, ll) + (() if grads is None else (grads,)):
        a.setflags(write=False)
    return X, y, Th, ll, grads


# (rows, "grad_batch_slots", groups): 2 + 2 + 1 rows (a ragged last group), the group rule alone, one row
MODES = {"slots2": (5, 2, [2, 2, 1]), "default": (5, 0, [5]), "one_row": (1, 0, [1])}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CASES))
def test_batch_matches_one_theta_call_and_oracle(name, mode):
    kernel, d, n, mean, _, _, otol = CASES[name]
    X, y, Th, want_ll, want_grad = reference(name)
    B, slots, groups = MODES[mode]
    h = _lib.Handle(X, y, kernel, mean)
    h.set_option("grad_batch_slots", slots)
    out, grad, info = h.loglik_grad_batch(Th[:B])
    assert out.shape == (B,) and grad.shape == (B, h.p) and np.all(info == 0)
    assert h.get_option("last_grad_batch_route") == 1 and h.get_option("last_grad_batch_slots") == groups[-1]
    assert h.get_option("grad_analytic") == 1
    for s in range(B):
        ll1, g1, i1 = h.loglik_grad(Th[s])
        assert i1 == 0
        print(name, mode, s, "one-theta:", np.abs(grad[s] - g1).max() / np.abs(g1).max(),
              "" if otol is None else ("oracle:", np.abs(grad[s] - want_grad[s]).max() / np.abs(want_grad[s]).max()))
        assert close(out[s], ll1, n) and close(out[s], want_ll[s], n)
        np.testing.assert_allclose(grad[s], g1, rtol=1e-9, atol=1e-9 * np.abs(g1).max())
        if otol is not None:
            np.testing.assert_allclose(grad[s], want_grad[s], rtol=otol, atol=otol * np.abs(want_grad[s]).max())
    h.close()


@pytest.mark.parametrize("kernel,d,n", [("se_ard", 3, 300), ("matern52_ard", 2, 257)])
def test_batch_fp32_matches_one_theta_call(kernel, d, n):
    X, y = syn.make_dataset(n, d)
    Th = theta_rows(kernel, d, "zero", None, d, dtype="f32")
    h = _lib.Handle(X, y, kernel, dtype=32)
    h.set_option("grad_batch_slots", 2)
    out, grad, info = h.loglik_grad_batch(Th)
    assert np.all(info == 0) and h.get_option("last_grad_batch_route") == 1
    for s in range(len(Th)):
        ll1, g1, _ = h.loglik_grad(Th[s])
        assert abs(out[s] - ll1) <= 2e-3 * max(abs(ll1), n)
        np.testing.assert_allclose(grad[s], g1, rtol=2e-3, atol=2e-3 * np.abs(g1).max())
    h.close()


def test_run_time_compiled_kernel():
    d, n = 3, 300
    X, y = syn.make_dataset(n, d)
    Th = theta_rows("se_ard", d, "zero", None, d, B=3)
    h = _lib.Handle(X, y, _lib.CustomKernel(SE_ARD_BODY, d + 1, fn=se_ard_fn))
    h.set_option("grad_batch_slots", 2)              # groups of 2 + 1: custom_grad_kernel once per slot
    out, grad, info = h.loglik_grad_batch(Th)
    assert np.all(info == 0) and h.get_option("grad_analytic") == 1 and h.get_option("last_grad_batch_route") == 1
    for s in range(3):
        ll1, g1, i1 = h.loglik_grad(Th[s])
        assert i1 == 0 and close(out[s], ll1, n)
        np.testing.assert_allclose(grad[s], g1, rtol=1e-9, atol=1e-9 * np.abs(g1).max())
    # no gradient program: the rows one by one through the central differences of the one-theta call, bit for bit
    h.set_option("custom_grad", 0)
    out, grad, info = h.loglik_grad_batch(Th)
    assert h.get_option("grad_analytic") == 0 and h.get_option("last_grad_batch_route") == 0
    for s in range(3):
        ll1, g1, i1 = h.loglik_grad(Th[s])
        assert info[s] == i1 == 0 and out[s] == ll1 and np.array_equal(grad[s], g1)
    h.close()


def test_failing_rows_disturb_no_other_row():
    n, d = 300, 3
    X, y = syn.make_dataset(n, d)
    X, y = X.copy(), y.copy()
    X[n - 1], y[n - 1] = X[17], y[17]                # one duplicated point: K is singular without the nugget
    healthy = theta_rows("se_ard", d, "zero", None, d)
    Th = healthy.copy()
    Th[1, 1] = np.nan
    Th[3, -1] = 0.0                                  # sn = 0
    h = _lib.Handle(X, y, "se_ard")
    assert h.loglik(Th[3])[1] == 1 and h.loglik(Th[1])[1] == 2
    h.set_option("grad_batch_slots", 2)
    out, grad, info = h.loglik_grad_batch(Th)
    assert list(info) == [0, 2, 0, 1, 0]
    assert np.all(np.isnan(grad[[1, 3]])) and np.all(np.isfinite(grad[[0, 2, 4]]))
    out_h, grad_h, info_h = h.loglik_grad_batch(healthy)
    assert np.all(info_h == 0)
    assert np.array_equal(out[[0, 2, 4]], out_h[[0, 2, 4]]) and np.array_equal(grad[[0, 2, 4]], grad_h[[0, 2, 4]])
    h.close()


def test_repeatable_and_independent_of_row_order():
    n, d = 300, 3
    X, y = syn.make_dataset(n, d)
    Th = theta_rows("matern52_ard", d, "const", None, d, B=4)
    h = _lib.Handle(X, y, "matern52_ard", "const")
    h.set_option("grad_batch_slots", 2)
    a, b = h.loglik_grad_batch(Th), h.loglik_grad_batch(Th)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    r = h.loglik_grad_batch(Th[::-1])
    assert all(np.array_equal(u, v[::-1]) for u, v in zip(a, r))
    h.close()


def test_state_statuses_and_routes():
    n, d = 300, 2
    X, y = syn.make_dataset(n, d)
    Th = theta_rows("se_ard", d, "zero", None, d, B=3)
    h = _lib.Handle(X, y, "se_ard")
    # the one-theta call returns the same bytes before and after a batch call on the same handle
    before = h.loglik_grad(Th[1])
    assert h.fit(Th[0]) == 0
    h.predict(X[:2])
    out, grad, info = h.loglik_grad_batch(Th)
    assert h.get_option("last_grad_batch_route") == 1 and h.get_option("last_grad_batch_slots") == 3
    with pytest.raises(_lib.GphipError) as e:        # the batch dropped the resident fit
        h.predict(X[:2])
    assert e.value.status == 4
    after = h.loglik_grad(Th[1])
    assert before[0] == after[0] and np.array_equal(before[1], after[1])
    # statuses: a wrong p (past the wrapper's own check), B = 0
    z, inf = np.zeros(3 * (h.p + 1)), np.zeros(3, dtype=np.int32)
    assert h._lib.gphip_loglik_grad_batch(h._h, _lib._d(z), 3, h.p + 1, _lib._d(z), _lib._d(z), inf.ctypes.data_as(_lib._ip)) == 2
    assert h._lib.gphip_loglik_grad_batch(h._h, None, 3, h.p, _lib._d(z), _lib._d(z), inf.ctypes.data_as(_lib._ip)) == 1
    o0, g0, i0 = h.loglik_grad_batch(np.zeros((0, h.p)))
    assert o0.shape == (0,) and g0.shape == (0, h.p) and i0.shape == (0,)
    # "grad_potri" = 0 (no K^-1 buffers): the per-row loop, bit for bit; so does a limit of one row per group
    # and a handle with more training points than "grad_batch_max_n"
    for name, value in (("grad_potri", 0), ("grad_batch_slots", 1), ("grad_batch_max_n", n - 1)):
        h.set_option(name, value)
        out0, grad0, info0 = h.loglik_grad_batch(Th)
        assert h.get_option("last_grad_batch_route") == 0
        for s in range(3):
            ll1, g1, i1 = h.loglik_grad(Th[s])
            assert info0[s] == i1 == 0 and out0[s] == ll1 and np.array_equal(grad0[s], g1)
        h.loglik_grad_batch(Th)
        with pytest.raises(_lib.GphipError):         # (no fit stays resident on this route either)
            h.predict(X[:2])
        h.set_option("grad_potri", 1)
        h.set_option("grad_batch_slots", 0)
        h.set_option("grad_batch_max_n", n)
    h.loglik_grad_batch(Th)
    assert h.get_option("last_grad_batch_route") == 1
    h.close()
    # the null kernel answers on the host
    hn = _lib.Handle(X, y, "null", "const")
    Tn = np.array([[0.3, 0.1], [0.5, -0.2], [np.nan, 0.0]])
    out, grad, info = hn.loglik_grad_batch(Tn)
    for s in range(3):
        ll1, g1, i1 = hn.loglik_grad(Tn[s])
        assert info[s] == i1 and np.array_equal(out[s], ll1, equal_nan=True) and np.array_equal(grad[s], g1, equal_nan=True)
    hn.close()


def test_laplace_hessian_is_one_batched_call():
    X, y = syn.make_dataset(400, 1)
    variables = [("l", 0.1, 1.0), ("sf", 0.3, 3.0), ("sn", 0.05, 0.3)]
    obj = gp.defineGaussianProcess((X, y), "SE", variables=variables, variablePrior="Uniform")
    assert not obj.failed
    inner = obj["LogLikelihoodGradientFunction"]
    assert inner.batched is True
    calls = []

    def counted(theta):
        calls.append(np.shape(theta))
        return inner(theta)

    res = {}
    for batched in (True, False):
        calls.clear()
        counted.batched = batched
        res[batched] = laplace.approximateEvidence(obj.append({"LogLikelihoodGradientFunction": counted}), Starts=3, Seed=2)
        two_d = [c for c in calls if len(c) == 2]
        assert two_d == ([(6, 3)] if batched else []) and res[batched] is not None
    assert np.array_equal(res[True]["Mean"], res[False]["Mean"])
    print("precision matrices:", res[True]["PrecisionMatrix"], res[False]["PrecisionMatrix"], sep="\n")
    np.testing.assert_allclose(res[True]["PrecisionMatrix"], res[False]["PrecisionMatrix"], rtol=1e-6)
    obj["GaussianProcessData"]["HIPHandle"].close()
