"""The analytic gradient of the sparse GP bound on the device (gphip_sparse_bound_grad) against the numpy references of
tests/sparse_grad_reference.py (pinned on the CPU by tests/test_sparse_grad.py).  The bar is the project's own for gradients
(tests/test_gpu_parity.py, tests/test_gpu_loo.py): 1e-7 of max |grad|; 2e-6 for difference quotients (tests/test_gpu_custom_kernel.py)."""
import numpy as np
import pytest

import sparse_grad_reference as sg
import sparse_reference as ref
from bayesianinference_amd import _lib, gaussian_process as gp, laplace, synthetic as syn

pytestmark = pytest.mark.gpu

SF = sg.SF
# a body whose dual-number instantiation cannot compile: an intermediate that depends on P is declared double
NODUAL_BODY = ("double s = 0; for (int k = 0; k < D; ++k) { const double u = (double)(X(k) - Y(k)) / (double)P(k); s += u * u; } "
               "return (T)((double)P(D) * (double)P(D) * exp(-0.5 * s));")


def _err(g, want):
    return float(np.abs(g - want).max() / np.abs(want).max())


def _device_case(c, mean, opts=None, dtype=64):
    h = _lib.SparseHandle(c["X"], c["y"], c["Z"], c["kernel"], mean, dtype=dtype)
    for k, v in (opts or {}).items():
        h.set_option(k, v)
    return h


@pytest.mark.parametrize("name,n,d,m,mean,opts", [c + (None,) for c in sg.CASES] + [("se_ard", 1333, 3, 150, "const", {"dataflow": 0})])
def test_gradient_matches_the_reference(name, n, d, m, mean, opts):
    c = sg.case_reference(name, n, d, m, mean)
    label = f"{name} N={n} d={d} m={m} {mean} {opts}"
    print(f"{label}: cond(K_uu) {c['cond']:.2e}, reference routes differ by {c['consistency']:.1e}")
    assert c["cond"] <= 1e10 and c["consistency"] <= 1e-9
    h = _device_case(c, mean, opts)
    assert h.p == len(c["theta"])
    F, grad, info = h.bound_grad(c["theta"], c["jitter"])
    analytic = h.get_option("grad_analytic")
    F2, _, info2 = h.bound_parts(c["theta"], c["jitter"])
    h.close()
    print(f"{label}: F rel {abs(F - c['F']) / abs(c['F']):.2e}, gradient error {_err(grad, c['grad']):.2e} of max |grad| {np.abs(c['grad']).max():.4g}")
    assert info == 0 and info2 == 0 and analytic == 1
    assert F == F2                                                   # the same bytes as gphip_sparse_bound
    assert _err(grad, c["grad"]) <= 1e-7


def test_chunking_and_strips_agree_and_repeat_bit_for_bit():
    """More than one chunk with a ragged last one, more than one tile of inducing points; a single chunk keeps V from the
    evaluation, two chunks rebuild it."""
    c = sg.case_reference("se_ard", 1333, 3, 300, "const")
    h = _device_case(c, "const")
    grads = {}
    for key, opts in (("default", {}), ("chunk128", {"sparse_chunk": 128}), ("chunk512", {"sparse_chunk": 512}),
                      ("two chunks", {"sparse_chunk": 768}), ("split1", {"sparse_split": 1}), ("split4", {"sparse_split": 4})):
        h.set_option("sparse_chunk", 0)
        h.set_option("sparse_split", 0)
        for k, v in opts.items():
            h.set_option(k, v)
        F1, g1, i1 = h.bound_grad(c["theta"], c["jitter"])
        F2, g2, i2 = h.bound_grad(c["theta"], c["jitter"])
        assert i1 == 0 and i2 == 0 and F1 == F2 and np.array_equal(g1, g2), key          # the same bytes
        grads[key] = g1
        print(key, h.get_option("last_sparse_chunk"), _err(g1, c["grad"]))
    h.close()
    for key, g in grads.items():
        assert _err(g, grads["default"]) <= 1e-11, key
        assert _err(g, c["grad"]) <= 1e-7, key


# (N, d, m, Z = X): the two ill-conditioned cases of DESIGN.md section 8c with small shapes, j = 1e-10 sf^2
ILL = [(1500, 1, 60, False), (1024, 3, 1024, True)]


@pytest.mark.parametrize("n,d,m,zx", ILL)
def test_ill_conditioned_inducing_sets(n, d, m, zx):
    """cond(K_uu) = 2e11 and 4.8e12, against the analytic reference (substitutions).  The device applies L_u^-1 by substitutions
    too, the route that is exact to rounding in numpy (products with the explicit U differ from it by 1e-11 there); the assertion
    is the 1e-7 bar of the well-conditioned cases, since the errors measured on an MI355X are below 1e-8: 7.5e-13 and 6.6e-13 of
    max |grad|."""
    X, y = syn.make_dataset(n, d)
    th, Z, jit = sg.theta_of("se_ard", d, "const"), (X if zx else sg.inducing_of(X, m)), 1e-10 * SF ** 2
    want = sg.analytic("se_ard", th, X, y, Z, jit, "const")
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const")
    F, grad, info = h.bound_grad(th, jit)
    h.close()
    print(f"N={n} d={d} m={m} Z=X {zx}: gradient error {_err(grad, want):.2e} of max |grad| {np.abs(want).max():.4g}")
    assert info == 0
    assert _err(grad, want) <= 1e-7


# fp32 object against the fp64 reference at N = 2000, d = 3, m = 300, default fp32 jitter (1e-4 k(x, x)).  Measured on an MI355X:
# 4.82e-5 of max |grad|; the bar is 4 x that, the rule of section 8c.
FP32_BAR = 4 * 4.82e-5


def test_fp32_object_against_the_fp64_reference():
    X, y = syn.make_dataset(2000, 3)
    th, Z = sg.theta_of("se_ard", 3, "const"), sg.inducing_of(X, 300)
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const", dtype=32)
    F, grad, info = h.bound_grad(th)
    jit = h.get_option("last_jitter")
    analytic = h.get_option("grad_analytic")
    h.close()
    assert info == 0 and analytic == 1 and jit == pytest.approx(1e-4 * SF ** 2, rel=1e-12)
    want = sg.analytic("se_ard", th, X, y, Z, jit, "const")
    print(f"fp32: gradient error {_err(grad, want):.2e} of max |grad| {np.abs(want).max():.4g}")
    assert _err(grad, want) <= FP32_BAR


@pytest.mark.parametrize("body,opts", [(NODUAL_BODY, {}), (sg.SE_ARD_BODY, {"custom_grad": 0})], ids=["no-dual-program", "custom_grad=0"])
def test_difference_fallback_of_a_run_time_compiled_kernel(body, opts):
    c = sg.case_reference("custom", 1333, 3, 150, "const")
    kernel = sg.kernel_of("custom", 3, body)
    h = _lib.SparseHandle(c["X"], c["y"], c["Z"], kernel, "const")
    for k, v in opts.items():
        h.set_option(k, v)
    F, grad, info = h.bound_grad(c["theta"], c["jitter"])
    analytic = h.get_option("grad_analytic")
    F2, info2 = h.bound(c["theta"], c["jitter"])
    mu, var = h.predict(c["X"][:5])                                  # the unperturbed fit stays resident
    wm, wv = ref.predict_formulas(c["kernel"], c["theta"], c["X"], c["y"], c["Z"], c["jitter"], c["X"][:5], "const")
    h.close()
    print(f"fallback {opts}: gradient error {_err(grad, c['grad']):.2e}")
    assert info == 0 and info2 == 0 and analytic == 0 and F == F2
    assert _err(grad, c["grad"]) <= 2e-6
    assert np.abs(mu - wm).max() <= 1e-7 * np.abs(c["y"]).max()


def test_failure_semantics_and_argument_errors():
    X, y = syn.make_dataset(900, 2)
    th, jit = sg.theta_of("se_ard", 2, "zero"), 1e-6 * SF ** 2
    Z = sg.inducing_of(X, 100)
    h = _lib.SparseHandle(X, y, Z, "se_ard", "zero")
    with pytest.raises(_lib.GphipError) as e:
        h.bound_grad(th[:-1], jit)
    assert e.value.status == 2
    with pytest.raises(_lib.GphipError) as e:
        h.bound_grad(th, float("nan"))
    assert e.value.status == 1
    import ctypes
    dp = ctypes.POINTER(ctypes.c_double)
    val, info = ctypes.c_double(0.0), ctypes.c_int(0)
    assert h._lib.gphip_sparse_bound_grad(h._h, th.ctypes.data_as(dp), len(th), jit, ctypes.byref(val), None, None, ctypes.byref(info)) == 1
    bad = th.copy()
    bad[0] = np.nan
    F, grad, info = h.bound_grad(bad, jit)
    assert info == _lib.INFO_NAN and np.isnan(F) and np.all(np.isnan(grad))
    # prediction from the fit a successful gradient call leaves, without gphip_sparse_fit
    F, grad, info = h.bound_grad(th, jit)
    assert info == 0 and np.all(np.isfinite(grad))
    Xs = syn.make_test_points(77, 2)
    mu, var = h.predict(Xs)
    wm, wv = ref.predict_formulas("se_ard", th, X, y, Z, jit, Xs, "zero")
    assert np.abs(mu - wm).max() <= 1e-7 * np.abs(y).max() and np.abs(var - wv).max() <= 1e-7 * SF ** 2
    # duplicate inducing points without jitter: K_uu is singular
    h.set_inducing(np.vstack([Z, Z[:7]]))
    F, grad, info = h.bound_grad(th, 0.0)
    assert info == _lib.INFO_NOT_SPD and np.isnan(F) and np.all(np.isnan(grad))
    # the object stays usable
    h.set_inducing(Z)
    F2, grad2, info = h.bound_grad(th, jit)
    assert info == 0 and np.isfinite(F2)
    assert np.array_equal(grad2, h.bound_grad(th, jit)[1])
    assert _err(grad2, sg.analytic("se_ard", th, X, y, Z, jit, "zero")) <= 1e-7
    h.close()


def test_host_object_gradient_and_hyperparameter_selection():
    X, y = syn.make_dataset(2000, 2)
    variables = [("l1", 0.2, 3.0), ("l2", 0.2, 3.0), ("sf", 0.3, 3.0), ("sn", 0.01, 0.5)]
    obj = gp.defineSparseGaussianProcess((X, y), "SEARD", 100, variables=variables, Jitter=1e-6)
    handle = obj["SparseGaussianProcessData"]["HIPHandle"]
    th = np.array([0.9, 1.1, 1.0, 0.12])
    val, grad = obj["LogLikelihoodGradientFunction"](th)
    F, g, info = handle.bound_grad(th, 1e-6)
    assert info == 0 and val == F and np.array_equal(grad, g) and val == obj["LogLikelihoodFunction"](th)
    v, gn = obj["LogLikelihoodGradientFunction"]([0.9, 1.1, 1.0, float("nan")])
    assert v == gp.MACHINE_LOG_ZERO and np.all(np.isnan(gn))
    quot = gp.defineSparseGaussianProcess((X, y), "SEARD", obj["InducingPoints"], variables=variables, Jitter=1e-6, Gradient="Differences")
    vq, gq = quot["LogLikelihoodGradientFunction"](th)
    quot["SparseGaussianProcessData"]["HIPHandle"].close()
    print(f"analytic against the difference quotient: {_err(grad, gq):.2e}")
    assert vq == val and _err(grad, gq) <= 2e-6
    # hyper-parameter selection from a start near the truth, to a tolerance of the test's own on L-BFGS-B's measure, the largest
    # component of the projected gradient |P(x + g) - x|: five orders below the start's largest gradient component.  (The device
    # gradient is right to 1e-7 of its largest term, so the tolerance asks nothing that the gradient cannot show.)  The maximum is
    # further than the tolerance from every face of the box, so there the measure is the gradient itself.
    lo, hi = np.array([v[1] for v in variables]), np.array([v[2] for v in variables])
    start = np.array([0.8, 0.8, 1.0, 0.25])
    v0, g0 = obj["LogLikelihoodGradientFunction"](start)
    tol = 1e-5 * np.abs(g0).max()
    sel = laplace.selectHyperparameters(obj, Criterion="MarginalLikelihood", InitialGuess=start, Tolerance=tol)
    assert sel is not None
    x1 = sel["Maximum"][1]
    v1, g1 = obj["LogLikelihoodGradientFunction"](x1)
    pg = np.clip(x1 + g1, lo, hi) - x1
    print(f"selectHyperparameters: F {v0:.4f} -> {v1:.4f} at {x1}, gradient {g1}, max |projected grad| {np.abs(g0).max():.3g} -> "
          f"{np.abs(pg).max():.3g} (tolerance {tol:.3g})")
    assert sel["Maximum"][0] == pytest.approx(v1, rel=1e-12)
    assert v1 >= v0 and np.abs(pg).max() <= tol
    assert np.all(np.minimum(x1 - lo, hi - x1) > tol) and np.abs(g1).max() <= tol
    handle.close()
