"""Sparse inducing-point GP, the part that needs no GPU: pins the numpy reference (tests/sparse_reference.py) by two algebraically
different routes, by 40-digit arithmetic and by the inequalities that hold in exact arithmetic, and checks the C ABI's boundary."""
import ctypes
import os

import numpy as np
import pytest

import sparse_reference as ref
from bayesianinference_amd import _lib, build, gaussian_process as gp, synthetic
from oracle import gp_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["gphip_sparse_create", "gphip_sparse_create_custom", "gphip_sparse_destroy", "gphip_sparse_set_inducing", "gphip_sparse_num_params",
         "gphip_sparse_bound", "gphip_sparse_fit", "gphip_sparse_predict", "gphip_sparse_set_option", "gphip_sparse_get_option",
         "gphip_sparse_last_error"]
SF = 1.1
# (N, d, m, jitter / sf^2): SE-ARD, l = linspace(0.8, 1.3, d) (d = 1: 0.3), sf = 1.1, sn = 0.15, mu = 0.2, Z = X[::N // m][:m]
CASES = [(1500, 3, 100, 1e-10), (1500, 3, 300, 1e-10), (1500, 3, 300, 1e-6), (2000, 8, 300, 1e-10), (1500, 1, 60, 1e-10), (1500, 1, 60, 1e-6)]


def case(N, d, m):
    X, y = synthetic.make_dataset(N, d)
    return X, y, X[::N // m][:m], ref.case_theta(d, mu=0.2)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


@pytest.mark.parametrize("N,d,m,jrel", CASES)
def test_formulas_agree_with_the_definition_and_stay_below_the_exact_likelihood(N, d, m, jrel):
    X, y, Z, th = case(N, d, m)
    jit = jrel * SF ** 2
    a = ref.bound_formulas("se_ard", th, X, y, Z, jit, "const")
    b = ref.bound_definition("se_ard", th, X, y, Z, jit, "const")
    print(f"routes: {a['F']:.10f} {b:.10f} rel {abs(a['F'] - b) / abs(b):.2e}")
    assert abs(a["F"] - b) <= 1e-10 * abs(b)
    chunked = ref.bound_formulas("se_ard", th, X, y, Z, jit, "const", chunk=400)
    assert abs(chunked["F"] - a["F"]) <= 1e-11 * abs(a["F"])
    exact = orc.log_likelihood("se_ard", th, X, y, "const")
    print(f"F {a['F']:.4f} exact {exact:.4f}")
    assert a["F"] <= exact                                  # a lower bound in exact arithmetic, jitter included


def test_prediction_formulas_agree_with_the_definition():
    X, y = synthetic.make_dataset(800, 3)
    Z, th = X[::800 // 120][:120], ref.case_theta(3, mu=0.2)
    Xs = synthetic.make_test_points(50, 3)
    for latent in (False, True):
        ma, va = ref.predict_formulas("se_ard", th, X, y, Z, 1e-6 * SF ** 2, Xs, "const", latent)
        mb, vb = ref.predict_definition("se_ard", th, X, y, Z, 1e-6 * SF ** 2, Xs, "const", latent)
        print(f"latent={latent}: mean {np.max(np.abs(ma - mb)):.2e} var {np.max(np.abs(va - vb)):.2e}")
        assert np.max(np.abs(ma - mb)) <= 1e-10 * np.max(np.abs(y))
        assert np.max(np.abs(va - vb)) <= 1e-10 * SF ** 2


def test_formulas_against_40_digit_arithmetic():
    """scripts/make_sparse_golden.py mpmath: the bound by the same formulas in 40-digit mpmath at N = 300 (the two float64 routes
    share the Cholesky of K_uu, so their agreement alone would not see an error made there)."""
    g = np.load(os.path.join(GOLDEN, "sparse_mpmath.npz"))
    for d, m, jrel in ((1, 60, 1e-10), (3, 100, 1e-10), (3, 100, 1e-6)):
        X, y, Z, th = case(300, d, m)
        F = ref.bound_formulas("se_ard", th, X, y, Z, jrel * SF ** 2, "const")["F"]
        hp = float(g[f"F_d{d}_m{m}_j{jrel:g}"])
        print(f"d={d} m={m} j={jrel:g}: float64 {F:.12f} mpmath {hp:.12f} rel {abs(F - hp) / abs(hp):.2e}")
        assert abs(F - hp) <= 1e-10 * abs(hp)


def test_bound_is_monotone_in_nested_inducing_sets():
    X, y = synthetic.make_dataset(1200, 3)
    th = ref.case_theta(3, mu=0.2)
    exact = orc.log_likelihood("se_ard", th, X, y, "const")
    vals = [ref.bound_formulas("se_ard", th, X, y, X[:m], 1e-6 * SF ** 2, "const")["F"] for m in (50, 100, 200, 400, 1200)]
    print(vals, exact)
    assert all(a <= b for a, b in zip(vals, vals[1:])) and vals[-1] <= exact


def test_gap_to_the_exact_likelihood_at_z_equal_x_shrinks_with_the_jitter():
    X, y = synthetic.make_dataset(1024, 3)
    th = ref.case_theta(3, mu=0.2)
    exact = orc.log_likelihood("se_ard", th, X, y, "const")
    gaps = [(exact - ref.bound_formulas("se_ard", th, X, y, X, j * SF ** 2, "const")["F"]) / abs(exact) for j in (1e-6, 1e-8, 1e-10)]
    print(gaps)
    assert gaps[0] > gaps[1] > gaps[2] > 0.0 and gaps[0] < 1e-4


def test_sparse_symbols_are_declared_and_exported(lib):
    names = _lib.declared_symbols()
    for name in NAMES:
        assert name in names and name in _lib._SIGNATURES
        assert hasattr(lib, name)
    text = open(_lib.HEADER).read()
    assert "#define GPHIP_SPARSE_MAX_M 16384" in text and _lib.SPARSE_MAX_M == 16384


def test_argument_errors_come_back_before_any_device_work(lib):
    X, y, Z = np.zeros((4, 2)), np.zeros(4), np.zeros((2, 2))
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    assert lib.gphip_sparse_create(None, y.ctypes.data, 4, 2, Z.ctypes.data, 2, 1, 0, 64, -1, out) == 1
    assert lib.gphip_sparse_create(X.ctypes.data, None, 4, 2, Z.ctypes.data, 2, 1, 0, 64, -1, out) == 1
    assert lib.gphip_sparse_create(X.ctypes.data, y.ctypes.data, 4, 2, None, 2, 1, 0, 64, -1, out) == 1
    assert lib.gphip_sparse_create(X.ctypes.data, y.ctypes.data, 4, 2, Z.ctypes.data, 2, 1, 0, 64, -1, None) == 1
    for N, d, m in ((0, 2, 2), (4, 0, 2), (4, 2, 0), (4, 2, _lib.SPARSE_MAX_M + 1)):
        assert lib.gphip_sparse_create(X.ctypes.data, y.ctypes.data, N, d, Z.ctypes.data, m, 1, 0, 64, -1, out) == 2
    assert lib.gphip_sparse_create(X.ctypes.data, y.ctypes.data, 4, 2, Z.ctypes.data, 2, _lib.KERNEL_IDS["null"], 0, 64, -1, out) == 6
    assert lib.gphip_sparse_create_custom(X.ctypes.data, y.ctypes.data, 4, 2, Z.ctypes.data, 2, None, 1, 0, 64, -1, out) == 1
    assert h.value is None
    assert lib.gphip_sparse_destroy(None) == 0
    dp = ctypes.POINTER(ctypes.c_double)
    th, val, info = np.ones(4), ctypes.c_double(0.0), ctypes.c_int(-1)
    assert lib.gphip_sparse_bound(None, th.ctypes.data_as(dp), 4, -1.0, ctypes.byref(val), None, ctypes.byref(info)) == 1
    assert lib.gphip_sparse_fit(None, th.ctypes.data_as(dp), 4, -1.0, ctypes.byref(info)) == 1
    assert lib.gphip_sparse_predict(None, X.ctypes.data, 4, 0, th.ctypes.data_as(dp), th.ctypes.data_as(dp)) == 1
    assert lib.gphip_sparse_set_inducing(None, Z.ctypes.data, 2) == 1
    assert lib.gphip_sparse_num_params(None, None) == 1
    assert lib.gphip_sparse_set_option(None, b"sparse_chunk", 1.0) == 1
    assert lib.gphip_sparse_get_option(None, b"sparse_chunk", None) == 1
    assert lib.gphip_sparse_last_error(None) == b"null handle"


def test_select_inducing_points_is_deterministic_and_distinct():
    X, _ = synthetic.make_dataset(500, 3)
    Z = gp.selectInducingPoints(X, 120)
    assert Z.shape == (120, 3) and np.array_equal(Z, gp.selectInducingPoints(X, 120, seed=0))
    rows = {tuple(r) for r in X}
    assert len({tuple(z) for z in Z}) == 120 and all(tuple(z) in rows for z in Z)
    assert not np.array_equal(Z, gp.selectInducingPoints(X, 120, seed=1))
    assert len({tuple(z) for z in gp.selectInducingPoints(X, 500)}) == 500
    with pytest.raises(ValueError):
        gp.selectInducingPoints(X, 501)


def test_define_sparse_gaussian_process_argument_guards_need_no_gpu():
    X = np.zeros((4, 2))
    assert gp.defineSparseGaussianProcess((X, np.zeros((4, 2))), "SEARD", 2, variables=[("l", 0, 1)]).failed
    assert gp.defineSparseGaussianProcess((X, np.zeros(3)), "SEARD", 2, variables=[("l", 0, 1)]).failed
    assert gp.defineSparseGaussianProcess("junk", "SEARD", 2, variables=[("l", 0, 1)]).failed
    assert gp.defineSparseGaussianProcess((X, np.zeros(4)), "SEARD", 2, variables=[]).failed
    assert gp.defineSparseGaussianProcess((X, np.zeros(4)), "SEARD", np.zeros((2, 3)), variables=[("l", 0, 1)]).failed
    with pytest.raises(ValueError):
        gp.defineSparseGaussianProcess((X, np.zeros(4)), "SEARD", 2, nugget=lambda P, th: 1.0, variables=[("l", 0, 1)])
    with pytest.raises(ValueError):
        gp.defineSparseGaussianProcess((X, np.zeros(4)), None, 2, variables=[("l", 0, 1)])
    assert gp.predictFromSparseGaussianProcess(gp.inferenceObject(None), X) is None
