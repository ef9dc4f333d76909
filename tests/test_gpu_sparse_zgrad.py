"""The gradient of the sparse GP bound in the inducing locations on the device (gphip_sparse_bound_grad_inducing), the in-place
gphip_sparse_set_inducing and gaussian_process.optimizeInducingPoints, against the CPU references of
tests/sparse_zgrad_reference.py (pinned by tests/test_sparse_zgrad.py).

The bar is the project's own for gradients, 1e-7 of max |gradient|, wherever the two CPU routes of a case (numpy analytic,
torch autograd) agree to 1e-8; elsewhere max(1e-7, 4 x the routes' difference): the sums over the data and over the inducing
points cancel by a factor of up to 4e4 (6e7 in the ill-conditioned sets), so dF/dZ carries rounding x cond(K_uu) x that factor
whoever computes it.  Errors measured on an MI355X are in DESIGN.md section 8e."""
import ctypes

import numpy as np
import pytest

import sparse_grad_reference as sg
import sparse_reference as ref
import sparse_zgrad_reference as zg
from bayesianinference_amd import _lib, gaussian_process as gp, synthetic as syn

pytestmark = pytest.mark.gpu

SF = sg.SF


def _err(g, want):
    return float(np.abs(g - want).max() / np.abs(want).max())


def _bar(route_difference):
    return 1e-7 if route_difference <= 1e-8 else max(1e-7, 4.0 * route_difference)


@pytest.mark.parametrize("name,n,d,m,mean,opts", [c + (None,) for c in zg.CASES] + [("se_ard", 1333, 3, 150, "const", {"dataflow": 0})])
def test_gradient_in_z_matches_the_reference(name, n, d, m, mean, opts):
    """Measured on an MI355X, in the order of zg.CASES: 7.2e-10, 1.6e-13, 4.7e-9, 4.6e-8 (bar 1.3e-7 .. 2.6e-7: the routes differ by
    3.3e-8 .. 6.5e-8, by machine), 2.2e-15, 5.2e-12, 6.3e-13, 2.1e-10, 5.2e-10."""
    c = zg.case_reference(name, n, d, m, mean)
    label = f"{name} N={n} d={d} m={m} {mean} {opts}"
    h = _lib.SparseHandle(c["X"], c["y"], c["Z"], name, mean)
    for k, v in (opts or {}).items():
        h.set_option(k, v)
    F, grad, gz, info = h.bound_grad_inducing(c["theta"], c["jitter"])
    analytic = h.get_option("grad_analytic")
    F3, none, gz3, info3 = h.bound_grad_inducing(c["theta"], c["jitter"], with_theta=False)
    F2, grad2, info2 = h.bound_grad(c["theta"], c["jitter"])
    Fb, infob = h.bound(c["theta"], c["jitter"])
    h.close()
    bar = _bar(c["route_difference"])
    print(f"{label}: gradient error {_err(gz, c['gradZ']):.3e} of max |dF/dZ| {np.abs(c['gradZ']).max():.4g}; the CPU routes differ by "
          f"{c['route_difference']:.3e}; bar {bar:.2e}")
    assert info == 0 and info2 == 0 and info3 == 0 and infob == 0 and analytic == 1
    assert gz.shape == (m, d) and none is None
    assert F == Fb and F == F2 and F == F3                         # the same bytes as gphip_sparse_bound
    assert np.array_equal(grad, grad2)                             # the same bytes as gphip_sparse_bound_grad
    assert np.array_equal(gz, gz3)                                 # skipping the theta reductions changes nothing
    assert _err(gz, c["gradZ"]) <= bar


# Across chunk and strip settings the forward pass sums V V^T in another order; dF/dZ follows that rounding through the
# cancellation.  Measured on an MI355X against the default setting: 1.6e-8 (chunk 128), 3.4e-9, 3.1e-9, 5.1e-9, 3.6e-9 of
# max |dF/dZ| (the theta gradient: 1.2e-13).  That argues against 1e-10; the bar is the gradient bar itself, which every setting
# also has to hold against the reference (errors 3.9e-9 .. 1.1e-8; the CPU routes differ by 4.1e-9 here).
ACROSS_SETTINGS_BAR = 1e-7


def test_chunking_and_strips_agree_and_repeat_bit_for_bit():
    name, n, d, m, mean = "se_ard", 1333, 3, 300, "const"
    c = zg.case_reference(name, n, d, m, mean)
    h = _lib.SparseHandle(c["X"], c["y"], c["Z"], name, mean)
    grads = {}
    for key, opts in (("default", {}), ("chunk128", {"sparse_chunk": 128}), ("chunk512", {"sparse_chunk": 512}),
                      ("two chunks", {"sparse_chunk": 768}), ("split1", {"sparse_split": 1}), ("split4", {"sparse_split": 4})):
        h.set_option("sparse_chunk", 0)
        h.set_option("sparse_split", 0)
        for k, v in opts.items():
            h.set_option(k, v)
        F1, g1, z1, i1 = h.bound_grad_inducing(c["theta"], c["jitter"])
        F2, g2, z2, i2 = h.bound_grad_inducing(c["theta"], c["jitter"])
        assert i1 == 0 and i2 == 0 and F1 == F2 and np.array_equal(g1, g2) and np.array_equal(z1, z2), key     # the same bytes
        grads[key] = z1
        print(f"{key}: chunk {h.get_option('last_sparse_chunk'):.0f}, against the reference {_err(z1, c['gradZ']):.3e}, "
              f"against the default setting {_err(z1, grads['default']):.3e}")
    h.close()
    print(f"the CPU routes differ by {c['route_difference']:.3e}")
    for key, z in grads.items():
        assert _err(z, grads["default"]) <= ACROSS_SETTINGS_BAR, key
        assert _err(z, c["gradZ"]) <= _bar(c["route_difference"]), key


# (N, d, m, Z = X): the two ill-conditioned sets of test_gpu_sparse_grad.ILL
ILL = [(1500, 1, 60, False), (1024, 3, 1024, True)]


@pytest.mark.parametrize("n,d,m,zx", ILL)
def test_ill_conditioned_inducing_sets(n, d, m, zx):
    """j = 1e-10 sf^2, cond(K_uu) = 2e11 and 4.8e12; the G and H sums cancel by 6e7 and max |dF/dZ| is 1.2e-4 / 2.7e-7.
    Reference: numpy analytic; bar: max(1e-7, 4 x the CPU routes' difference).  Measured on an MI355X:

        (1500, 1, 60)       device error 4.2e-5, CPU routes differ by 3.5e-5 .. 4.1e-5 (by machine), bar 1.4e-4 .. 1.6e-4
        (1024, 3, 1024)     device error 2.2e-3, CPU routes differ by 1.4e-3 .. 1.6e-3, bar 5.5e-3 .. 6.3e-3

    The first set is what the refined diagonal solves of the backward substitution are for: with bare
    products by the explicit inverses of L_u's diagonal 128-blocks -- m = 60 is one block -- its error was 6.4e-3."""
    X, y = syn.make_dataset(n, d)
    th, Z, jit = sg.theta_of("se_ard", d, "const"), (X if zx else sg.inducing_of(X, m)), 1e-10 * SF ** 2
    want = zg.analytic("se_ard", th, X, y, Z, jit, "const")
    routes = _err(zg.autograd("se_ard", th, X, y, Z, jit, "const")[2], want)
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const")
    F, grad, gz, info = h.bound_grad_inducing(th, jit)
    h.close()
    bar = max(1e-7, 4.0 * routes)
    print(f"N={n} d={d} m={m} Z=X {zx}: gradient error {_err(gz, want):.3e} of max |dF/dZ| {np.abs(want).max():.4g}; the CPU routes differ by "
          f"{routes:.3e}; bar {bar:.2e}")
    assert info == 0
    assert _err(gz, want) <= bar


# fp32 object against the fp64 reference at N = 2000, d = 3, m = 300, default fp32 jitter (1e-4 k(x, x)).  Measured on an MI355X:
# 6.149e-2 .. 6.155e-2 of max |dF/dZ| (the theta gradient of the same call: 4.8e-5; the fp32 weights G and H cancel by three more digits in Z);
# the bar is 4 x that, the rule of DESIGN.md section 8c.
FP32_BAR = 4 * 6.149e-2


def test_fp32_object_against_the_fp64_reference():
    X, y = syn.make_dataset(2000, 3)
    th, Z = sg.theta_of("se_ard", 3, "const"), sg.inducing_of(X, 300)
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const", dtype=32)
    F, grad, gz, info = h.bound_grad_inducing(th)
    jit = h.get_option("last_jitter")
    F2, grad2, info2 = h.bound_grad(th)
    h.close()
    assert info == 0 and info2 == 0 and jit == pytest.approx(1e-4 * SF ** 2, rel=1e-12)
    assert F == F2 and np.array_equal(grad, grad2)
    want = zg.analytic("se_ard", th, X, y, Z, jit, "const")
    print(f"fp32: gradient error {_err(gz, want):.3e} of max |dF/dZ| {np.abs(want).max():.4g}")
    assert _err(gz, want) <= FP32_BAR


def test_statuses_and_failure_semantics():
    X, y = syn.make_dataset(900, 2)
    th, jit = sg.theta_of("se_ard", 2, "zero"), 1e-6 * SF ** 2
    Z = sg.inducing_of(X, 100)
    # a run-time compiled covariance function: unsupported
    custom = _lib.SparseHandle(X, y, Z, sg.kernel_of("custom", 2), "zero")
    with pytest.raises(_lib.GphipError) as e:
        custom.bound_grad_inducing(th, jit)
    assert e.value.status == 6
    assert custom.bound(th, jit)[1] == 0                             # (the object is untouched)
    custom.close()
    h = _lib.SparseHandle(X, y, Z, "se_ard", "zero")
    with pytest.raises(_lib.GphipError) as e:
        h.bound_grad_inducing(th[:-1], jit)
    assert e.value.status == 2
    with pytest.raises(_lib.GphipError) as e:
        h.bound_grad_inducing(th, float("nan"))
    assert e.value.status == 1
    dp = ctypes.POINTER(ctypes.c_double)
    val, info, g = ctypes.c_double(0.0), ctypes.c_int(0), np.zeros(len(th))
    assert h._lib.gphip_sparse_bound_grad_inducing(h._h, th.ctypes.data_as(dp), len(th), jit, ctypes.byref(val), g.ctypes.data_as(dp), None, None,
                                                   ctypes.byref(info)) == 1
    bad = th.copy()
    bad[0] = np.nan
    F, grad, gz, info = h.bound_grad_inducing(bad, jit)
    assert info == _lib.INFO_NAN and np.isnan(F) and np.all(np.isnan(grad)) and np.all(np.isnan(gz)) and gz.shape == (100, 2)
    # prediction from the fit a successful call leaves, without gphip_sparse_fit
    F, grad, gz, info = h.bound_grad_inducing(th, jit, with_theta=False)
    assert info == 0 and grad is None and np.all(np.isfinite(gz))
    Xs = syn.make_test_points(77, 2)
    mu, var = h.predict(Xs)
    wm, wv = ref.predict_formulas("se_ard", th, X, y, Z, jit, Xs, "zero")
    assert np.abs(mu - wm).max() <= 1e-7 * np.abs(y).max() and np.abs(var - wv).max() <= 1e-7 * SF ** 2
    # duplicate inducing points without jitter: K_uu is singular (same m: the in-place route)
    Zd = Z.copy()
    Zd[-7:] = Z[:7]
    h.set_inducing(Zd)
    F, grad, gz, info = h.bound_grad_inducing(th, 0.0)
    assert info == _lib.INFO_NOT_SPD and np.isnan(F) and np.all(np.isnan(grad)) and np.all(np.isnan(gz))
    # the object stays usable
    h.set_inducing(Z)
    F2, grad2, gz2, info = h.bound_grad_inducing(th, jit)
    assert info == 0 and np.isfinite(F2)
    assert _err(gz2, zg.analytic("se_ard", th, X, y, Z, jit, "zero")) <= 1e-7
    h.close()


@pytest.mark.parametrize("m2", [150, 200], ids=["same m", "changed m"])
def test_set_inducing_gives_the_bytes_of_a_fresh_object(m2):
    X, y = syn.make_dataset(1333, 3)
    th, jit = sg.theta_of("se_ard", 3, "const"), 1e-6 * SF ** 2
    Z1 = sg.inducing_of(X, 150)
    Z2 = X[5::6][:m2] + 0.01                                         # other locations, off the data
    Xs = syn.make_test_points(50, 3)
    h = _lib.SparseHandle(X, y, Z1, "se_ard", "const")
    h.set_option("dataflow", 0)                                      # (options survive both routes)
    assert h.bound_grad(th, jit)[2] == 0
    h.set_inducing(Z2)
    with pytest.raises(_lib.GphipError) as e:                        # the fit is dropped
        h.predict(Xs)
    assert e.value.status == 4
    fresh = _lib.SparseHandle(X, y, Z2, "se_ard", "const")
    fresh.set_option("dataflow", 0)
    a = (h.bound(th, jit), h.bound_grad(th, jit), h.bound_grad_inducing(th, jit), h.predict(Xs))
    b = (fresh.bound(th, jit), fresh.bound_grad(th, jit), fresh.bound_grad_inducing(th, jit), fresh.predict(Xs))
    assert h.get_option("dataflow") == 0
    h.close()
    fresh.close()
    assert a[0] == b[0]
    assert a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2] == b[1][2] == 0
    assert a[2][0] == b[2][0] and np.array_equal(a[2][1], b[2][1]) and np.array_equal(a[2][2], b[2][2])
    assert np.array_equal(a[3][0], b[3][0]) and np.array_equal(a[3][1], b[3][1])


VARIABLES = [("l1", 0.2, 3.0), ("l2", 0.2, 3.0), ("sf", 0.3, 3.0), ("sn", 0.01, 0.5)]
THETA = np.array([0.9, 1.1, 1.0, 0.12])


def test_optimize_inducing_points():
    """N = 2000, d = 2, m = 20: the numpy reference alone reaches the tolerance in 32 iterations (F 1613.51 -> 1651.99,
    max |dF/dZ| 168 -> 1.7e-3); the device run measured the same 32 iterations and 34 evaluations."""
    X, y = syn.make_dataset(2000, 2)
    obj = gp.defineSparseGaussianProcess((X, y), "SEARD", 20, variables=VARIABLES, Jitter=1e-6)
    handle = obj["SparseGaussianProcessData"]["HIPHandle"]
    Z0 = obj["InducingPoints"].copy()
    F0, _, gz0, info = handle.bound_grad_inducing(THETA, 1e-6, with_theta=False)
    assert info == 0 and _err(gz0, zg.analytic("se_ard", THETA, X, y, Z0, 1e-6, "zero")) <= 1e-7
    tol = 1e-5 * np.abs(gz0).max()
    new = gp.optimizeInducingPoints(obj, THETA, Tolerance=tol)
    io, Z1 = new["InducingOptimisation"], new["InducingPoints"]
    F1, _, gz1, info = handle.bound_grad_inducing(THETA, 1e-6, with_theta=False)      # the handle is left at the best Z
    print(f"optimizeInducingPoints: F {io['Start']:.4f} -> {io['Maximum']:.4f} in {io['Iterations']} iterations, {io['Evaluations']} evaluations "
          f"({io['Message']}); max |dF/dZ| {np.abs(gz0).max():.4g} -> {np.abs(gz1).max():.4g} (tolerance {tol:.4g})")
    assert info == 0 and io["Start"] == F0 and io["Maximum"] == F1 and np.array_equal(io["Theta"], THETA)
    assert F1 > F0
    assert np.abs(gz1).max() <= tol
    assert Z1.shape == Z0.shape and np.abs(Z1 - Z0).max() > 1e-3 and np.array_equal(obj["InducingPoints"], Z0)
    Xs = syn.make_test_points(60, 2)
    pred = gp.predictFromSparseGaussianProcess(new, Xs, THETA)
    wm, wv = ref.predict_formulas("se_ard", THETA, X, y, Z1, 1e-6, Xs, "zero")
    assert np.abs(pred["Mean"][0] - wm).max() <= 1e-7 * np.abs(y).max()
    assert np.abs(pred["StandardDeviation"][0] ** 2 - wv).max() <= 1e-7 * SF ** 2
    # jointly over (theta, Z) from the same start
    handle.set_inducing(Z0)
    joint = gp.optimizeInducingPoints(obj, THETA, Joint=True)
    jo = joint["InducingOptimisation"]
    print(f"joint: F {jo['Start']:.4f} -> {jo['Maximum']:.4f} at theta {jo['Theta']} in {jo['Iterations']} iterations")
    lo, hi = np.array([v[1] for v in VARIABLES]), np.array([v[2] for v in VARIABLES])
    assert jo["Start"] == F0 and jo["Maximum"] >= F0
    assert np.all(jo["Theta"] >= lo) and np.all(jo["Theta"] <= hi)
    handle.close()


def test_optimize_inducing_points_refuses_what_it_cannot_do():
    X, y = syn.make_dataset(300, 2)
    custom = sg.kernel_of("custom", 2)
    obj = gp.defineSparseGaussianProcess((X, y), custom, 10, variables=[("l1", 0.2, 3.0), ("l2", 0.2, 3.0), ("sf", 0.3, 3.0), ("sn", 0.01, 0.5)])
    with pytest.raises(ValueError):
        gp.optimizeInducingPoints(obj, THETA)
    obj["SparseGaussianProcessData"]["HIPHandle"].close()
    exact = gp.defineGaussianProcess((X, y), "SEARD", variables=VARIABLES)
    assert gp.optimizeInducingPoints(exact, THETA) is None
