"""The gradient of the sparse GP bound, the part that needs no GPU: pins the numpy references of tests/sparse_grad_reference.py
against each other (the analytic formulas of include/gphip.h against 4th-order differences of the bound, differences of the two
algebraically different routes of the bound against each other) and checks the C ABI's boundary."""
import ctypes
import time

import numpy as np
import pytest

import sparse_grad_reference as sg
from bayesianinference_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


@pytest.mark.parametrize("name,n,d,m,mean", sg.CASES)
def test_reference_routes_agree(name, n, d, m, mean):
    """Analytic formulas against differences of bound_formulas (SE-ARD, Matern-5/2-ARD); differences of bound_formulas against
    differences of bound_definition (every other family).  Measured: at most 7e-11 of max |grad|."""
    t0 = time.time()
    c = sg.case_reference(name, n, d, m, mean)
    print(f"{name} N={n} d={d} m={m} {mean}: cond(K_uu) {c['cond']:.2e} routes differ by {c['consistency']:.2e} of max |grad| "
          f"{np.abs(c['grad']).max():.4g} ({time.time() - t0:.1f} s)")
    assert c["cond"] <= 1e10
    assert c["consistency"] <= 1e-9


@pytest.mark.parametrize("name,n,d,m,mean", [c for c in sg.CASES if c[0] in sg.ANALYTIC])
def test_differences_of_the_two_bound_routes_agree(name, n, d, m, mean):
    """Differences of bound_formulas against differences of bound_definition where the analytic formulas are the reference too
    (the other families have this comparison in test_reference_routes_agree): the bound the formulas differentiate is the bound
    of the definition.  The same 1e-9 bar."""
    c = sg.case_reference(name, n, d, m, mean)
    other = sg.differences(c["kernel"], c["theta"], c["X"], c["y"], c["Z"], c["jitter"], mean,
                           bound=lambda t: sg.ref.bound_definition(c["kernel"], t, c["X"], c["y"], c["Z"], c["jitter"], mean))
    err = float(np.abs(c["differences"] - other).max() / np.abs(other).max())
    print(f"{name} N={n} d={d} m={m} {mean}: differences of the two routes differ by {err:.2e}")
    assert err <= 1e-9


def test_explicit_inverse_factor_route_matches_substitutions_when_ill_conditioned():
    """N 1500, d 1, m 60, j = 1e-10 sf^2 (cond(K_uu) ~ 2e11): products with the explicit triangular U = L_u^-T against
    substitutions -- the two ways of applying L_u^-1 factor by factor that stay accurate at that conditioning."""
    from bayesianinference_amd import synthetic as syn
    X, y = syn.make_dataset(1500, 1)
    th, Z, jit = sg.theta_of("se_ard", 1, "const"), sg.inducing_of(X, 60), 1e-10 * sg.SF ** 2
    a = sg.analytic("se_ard", th, X, y, Z, jit, "const")
    b = sg.analytic("se_ard", th, X, y, Z, jit, "const", explicit_u=True)
    err = np.abs(a - b).max() / np.abs(a).max()
    print(f"explicit U against substitutions: {err:.2e}")
    assert err <= 1e-10


def test_bound_grad_is_declared_exported_and_has_a_signature(lib):
    assert "gphip_sparse_bound_grad" in _lib.declared_symbols()
    assert "gphip_sparse_bound_grad" in _lib._SIGNATURES
    assert hasattr(lib, "gphip_sparse_bound_grad")
    assert hasattr(_lib.SparseHandle, "bound_grad")


def test_null_arguments_come_back_before_any_device_work(lib):
    dp = ctypes.POINTER(ctypes.c_double)
    th, g, val, info = np.ones(4), np.zeros(4), ctypes.c_double(0.0), ctypes.c_int(-1)
    assert lib.gphip_sparse_bound_grad(None, th.ctypes.data_as(dp), 4, -1.0, ctypes.byref(val), g.ctypes.data_as(dp), None,
                                       ctypes.byref(info)) == 1
    assert lib.gphip_sparse_bound_grad(None, None, 4, -1.0, None, None, None, None) == 1
    assert info.value == -1 and np.all(g == 0.0)
