"""Every input-dimension instantiation of the dispatched kernels on the device: the table of tests/dim_dispatch_cases.py (both
sides of every threshold of every host-side `switch` / `if` chain on d, one interior d per interval, whole windows and
single-coordinate tails) through the public entry points, against the references the project already has.  The host half --
thresholds read from the sources, coverage of the table, conditioning of the inputs, the references against their own second
route at every d -- is tests/test_dim_dispatch.py.

Shapes are the smallest with more than one tile and a ragged last one: N = 150 for builds, likelihoods and theta-gradients; N = 300,
M = 130, m = 40 for the input gradients; n = 100, S = 5, F = 40, 70 points for the pathwise draws.  Every bar is the one the existing
test of the same entry point holds (imported where it is a module constant); the composed forms' theta-gradient is held to the
1e-7 of the named kernels, now that tests/loglik_grad_reference.py gives them an analytic reference (eps x cond(K) x N ~ 1e-10 at
the conditioning tests/test_dim_dispatch.py checks).  Errors measured on an MI355X are in DESIGN.md section 8p.

test_two_live_general_form_handles: the dynamic-LDS limit of kbuild_kernel<T, 0, 2> and of the two general gradient kernels is an
attribute of the FUNCTION; it used to be set from each handle's own d, so a later handle of fewer dimensions lowered it under an
earlier one.  It is now set once to the KB_LDS_MAXD maximum (found by reading, d = 32 then d = 2 is the case that would show it)."""
import numpy as np
import pytest

import dim_dispatch_cases as dc
import loglik_grad_reference as lgr
import loo_reference
import paths_own_reference as por
import paths_reference as pr
from bayesianinference_amd import _lib
from oracle import gp_oracle as orc
from test_gpu_paths import BAR as PATHS_BAR
from test_gpu_paths_own import BAR as PATHS_OWN_BAR
from test_gpu_predict_grad import BAR as XGRAD_BAR
from test_gpu_sparse_predict_grad import BAR as SPARSE_XGRAD_BAR
from test_gpu_sparse_zgrad import _bar as zgrad_bar

pytestmark = pytest.mark.gpu

EPS = 2.220446049250313e-16
SE_ARD_BODY = "T s = 0; for (int k = 0; k < D; ++k) { const T u = (X(k) - Y(k)) / P(k); s += u * u; } return P(D) * P(D) * exp((T)-0.5 * s);"
ANALYTIC_ORACLE = ("se_ard", "matern52_ard")
_refs = {}


def se_ard_fn(A, B, p):
    d = A.shape[-1]
    return p[d] ** 2 * np.exp(-0.5 * (((A - B) / p[:d]) ** 2).sum(-1))


def close(a, b, n=1, rtol=1e-8):                     # the suite's bar for values (tests/test_gpu_parity.py)
    return abs(a - b) <= rtol * max(abs(b), float(n))


def _err(g, want):
    return float(np.abs(g - want).max() / np.abs(want).max())


def _ids(cases):
    return [dc.case_id(c) for c in cases]


def _build_reference(kernel, d):
    """oracle K, k*, kappa and likelihood parts of a build case, once per process"""
    key = ("K", kernel, d)
    if key not in _refs:
        c = dc.build_data(kernel, d)
        ko, kapo = orc.k_and_kappa(kernel, c["theta"], c["X"], c["Xs"], c["mean_kind"])
        _refs[key] = (orc.covariance_matrix(kernel, c["theta"], c["X"], c["mean_kind"]), ko, kapo,
                      orc.log_likelihood(kernel, c["theta"], c["X"], c["y"], c["mean_kind"], parts=True))
    return _refs[key]


def _grad_reference(kernel, d, B=1):
    """(theta rows, oracle likelihoods, analytic gradients): the oracle's own formula for SE / Matern-5/2, autograd for the rest"""
    key = ("grad", kernel, d, B)
    if key not in _refs:
        c = dc.build_data(kernel, d)
        Th = dc.theta_rows(kernel, d, B, c["mean_kind"])
        fn = orc.log_likelihood_grad if kernel in ANALYTIC_ORACLE else lgr.log_likelihood_grad
        _refs[key] = (Th, np.array([orc.log_likelihood(kernel, t, c["X"], c["y"], c["mean_kind"]) for t in Th]),
                      np.array([fn(kernel, t, c["X"], c["y"], c["mean_kind"]) for t in Th]))
    return _refs[key]


def _check_likelihood(h, c, want, n, rtol, label):
    lo, ldo, qdo, _ = want
    ll, ld, qd, info = h.loglik_parts(c["theta"])
    print(f"{label}: loglik {abs(ll - lo) / max(abs(lo), n):.3e} logdet {abs(ld - ldo) / max(abs(ldo), n):.3e} "
          f"quad {abs(qd - qdo) / max(abs(qdo), n):.3e} of max(|.|, N)")
    assert info == 0 and close(ll, lo, n, rtol) and close(ld, ldo, n, rtol) and close(qd, qdo, n, rtol), label


# ---- builds ----
DIRECT = dc.cases("kbuild_direct") + dc.cases("general_two_term") + dc.cases("general_one_term")


@pytest.mark.parametrize("case", DIRECT, ids=_ids(DIRECT))
def test_direct_build(case):
    """kbuild_kernel<T, D, KT>: D = 1 .. 8 and 16, the generic form with LDS tiles (d <= 32) and from global memory (d > 32), and
    the general form kbuild_kernel<T, 0, 2> with its 4 d tiles (128 KiB at d = 32).  Bars of tests/test_gpu_kernels.py."""
    _, kernel, d = case
    c = dc.build_data(kernel, d)
    Ko, ko, kapo, want = _build_reference(kernel, d)
    h = _lib.Handle(c["X"], c["y"], kernel, c["mean_kind"])
    h.set_option("kbuild_mfma", 0)
    K = h.covariance(c["theta"])
    k, kappa = h.cross_covariance(c["theta"], c["Xs"])
    print(f"{dc.case_id(case)}: K {np.abs(K / Ko - 1).max():.3e} k* {np.abs(k - ko).max() / np.abs(ko).max():.3e}")
    np.testing.assert_allclose(K, Ko, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(k, ko, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(kappa, kapo, rtol=1e-13)
    assert np.array_equal(K, K.T)
    _check_likelihood(h, c, want, dc.N_BUILD, 1e-8, dc.case_id(case))
    h.set_option("fused_eval", 0)                                 # the tiles from the build kernel's own launch, not the fused one
    _check_likelihood(h, c, want, dc.N_BUILD, 1e-8, dc.case_id(case) + " fused_eval=0")
    h.close()


MFMA = dc.cases("kbuild_mfma") + dc.cases("general_one_term")


@pytest.mark.parametrize("case", MFMA, ids=_ids(MFMA))
def test_mfma_build(case):
    """kbuild_mfma_kernel<T, KS, KT>, KS = (d + 3) / 4 = 1 .. 4 and the generic form up to d = 32, forced (kbuild_mfma = 2).  Bar of
    test_entries_match_oracle_off_centre_inputs: max(1e-12, 8 eps sum (half range_k / l_k)^2)."""
    _, kernel, d = case
    c = dc.build_data(kernel, d)
    Ko, ko, kapo, want = _build_reference(kernel, d)
    bound = float(np.sum((np.ptp(c["X"], axis=0) / 2 / c["theta"][:d]) ** 2))
    tol = max(1e-12, 8 * EPS * bound)
    h = _lib.Handle(c["X"], c["y"], kernel, c["mean_kind"])
    h.set_option("kbuild_mfma", 0)
    K0 = h.covariance(c["theta"])
    h.set_option("kbuild_mfma", 2)
    K = h.covariance(c["theta"])
    k, kappa = h.cross_covariance(c["theta"], c["Xs"])
    print(f"{dc.case_id(case)}: K {np.abs(K / Ko - 1).max():.3e} k* {np.abs(k / ko - 1).max():.3e}; bar {tol:.2e}")
    np.testing.assert_allclose(K, Ko, rtol=tol, atol=1e-300)
    np.testing.assert_allclose(k, ko, rtol=tol, atol=1e-300)
    assert np.array_equal(K, K.T)
    assert not np.array_equal(K, K0)                              # (the forced mode really took the other kernel)
    h.set_option("fused_eval", 0)
    _check_likelihood(h, c, want, dc.N_BUILD, 1e-8, dc.case_id(case))
    h.close()


FP32 = dc.cases("kbuild_direct")


@pytest.mark.parametrize("case", FP32, ids=_ids(FP32))
def test_fp32_direct_build(case):
    """the fp32 body of the direct build at every D.  Bars of test_fp32_path_against_fp64_oracle."""
    _, kernel, d = case
    c = dc.build_data(kernel, d)
    Ko, ko, kapo, want = _build_reference(kernel, d)
    h = _lib.Handle(c["X"], c["y"], kernel, c["mean_kind"], dtype=32)
    h.set_option("kbuild_mfma", 0)
    K = h.covariance(c["theta"])
    print(f"{dc.case_id(case)} fp32: K {np.abs(K - Ko).max():.3e} absolute")
    np.testing.assert_allclose(K, Ko, rtol=2e-5, atol=1e-6)
    _check_likelihood(h, c, want, dc.N_BUILD, 1e-3, dc.case_id(case) + " fp32")
    h.close()


# ---- theta-gradients ----
GRAD = dc.cases("grad_reduce") + dc.cases("general_two_term") + dc.cases("general_one_term") + dc.cases("grad_rows")
ATOMICS_FROM = dc.SITES["grad_rows"]["edges"][0] + 1              # the accumulators on atomics: exempt from the same-bytes promise


@pytest.mark.parametrize("case", GRAD, ids=_ids(GRAD))
def test_theta_gradient(case):
    """grad_reduce_kernel<T, D, KT> (D = 1 .. 8, 16, generic) and grad_reduce_general_kernel (4 d + 1 LDS tiles up to d = 32, windows
    of 32 length-scale derivatives beyond: 64 = two whole windows, 65 = a third of one coordinate), per-workgroup rows up to d = 125
    and atomics from 126; gphip_loglik_grad_batch carries the slot through the _slots twins.  Bar of
    test_loglik_gradient_matches_oracle, for the composed forms too."""
    _, kernel, d = case
    c = dc.build_data(kernel, d)
    n = dc.N_BUILD
    Th, want_ll, want = _grad_reference(kernel, d, 3)
    h = _lib.Handle(c["X"], c["y"], kernel, c["mean_kind"])
    for potri in (1, 0):
        h.set_option("grad_potri", potri)
        ll, grad, info = h.loglik_grad(Th[0])
        print(f"{dc.case_id(case)} grad_potri={potri}: {_err(grad, want[0]):.3e} of max |gradient| {np.abs(want[0]).max():.4g}")
        assert info == 0 and close(ll, want_ll[0], n) and h.get_option("grad_analytic") == 1
        np.testing.assert_allclose(grad, want[0], rtol=1e-7, atol=1e-7 * np.abs(want[0]).max())
        if d < ATOMICS_FROM:
            ll2, grad2, _ = h.loglik_grad(Th[0])
            assert ll2 == ll and np.array_equal(grad2, grad)
    h.set_option("grad_potri", 1)
    h.set_option("grad_batch_slots", 2)                           # groups of 2 + 1
    out, gb, info = h.loglik_grad_batch(Th)
    assert np.all(info == 0) and h.get_option("last_grad_batch_route") == 1 and h.get_option("last_grad_batch_slots") == 1
    for s in range(3):
        print(f"{dc.case_id(case)} batch row {s}: {_err(gb[s], want[s]):.3e}")
        assert close(out[s], want_ll[s], n)
        np.testing.assert_allclose(gb[s], want[s], rtol=1e-7, atol=1e-7 * np.abs(want[s]).max())
    if d < ATOMICS_FROM:
        out2, gb2, _ = h.loglik_grad_batch(Th)
        assert np.array_equal(out, out2) and np.array_equal(gb, gb2)
    h.close()


# the two ends of every interval of launch_grad_kt: D = 1 .. 8 | generic 9 .. 15 | 16 | generic 17 .. 32 | windows beyond
LOO = [c for c in dc.cases("grad_reduce") if c[2] in (1, 8, 9, 15, 16, 17, 32, 33)]


@pytest.mark.parametrize("case", LOO, ids=_ids(LOO))
def test_loo_gradient(case):
    """gphip_loo_grad runs the same reductions with other weights.  Bar of test_loo_gradient_matches_numpy."""
    _, kernel, d = case
    c = dc.build_data(kernel, d)
    want = loo_reference.loo_grad_formula(kernel, c["theta"], c["X"], c["y"], c["mean_kind"])
    h = _lib.Handle(c["X"], c["y"], kernel, c["mean_kind"])
    total, g, info = h.loo_grad(c["theta"])
    print(f"{dc.case_id(case)} loo: {_err(g, want):.3e} of max |gradient| {np.abs(want).max():.4g}")
    assert info == 0 and h.get_option("grad_analytic") == 1
    assert _err(g, want) <= 1e-7
    t2, g2, _ = h.loo_grad(c["theta"])
    assert t2 == total and np.array_equal(g, g2)
    h.close()


# ---- theta as kernel arguments ----
@pytest.mark.parametrize("B,d", dc.SITES["theta_packed"]["Bd"], ids=["theta_packed-se_ard-B%d-d%d" % bd for bd in dc.SITES["theta_packed"]["Bd"]])
def test_theta_as_kernel_arguments(B, d):
    """B (d + SLOTP) <= THETA_PACK: theta travels as kernel arguments and the evaluation may be one fused launch; one past the edge
    it is copied.  Both sides against the oracle (1e-8) and against fused_eval = 0 (1e-10)."""
    kernel, n = "se_ard", dc.N_BUILD
    c = dc.build_data(kernel, d)
    Th = dc.theta_rows(kernel, d, B)
    want = np.array([orc.log_likelihood(kernel, t, c["X"], c["y"]) for t in Th])
    h = _lib.Handle(c["X"], c["y"], kernel)
    got = {}
    for fused in (1, 0):
        h.set_option("fused_eval", fused)
        if B == 1:
            ll, info = h.loglik(Th[0])
            got[fused] = np.array([ll])
            assert info == 0
        else:
            got[fused], info = h.loglik_batch(Th)
            assert np.all(info == 0)
        print(f"theta_packed B={B} d={d} fused_eval={fused}: {np.max(np.abs(got[fused] - want) / np.maximum(np.abs(want), n)):.3e}")
        assert all(close(a, b, n) for a, b in zip(got[fused], want))
    h.close()
    assert all(close(a, b, n, 1e-10) for a, b in zip(got[1], got[0]))


# ---- input gradients ----
XGRAD = dc.cases("predict_xgrad_one_term") + dc.cases("predict_xgrad_two_terms")


@pytest.mark.parametrize("case", XGRAD, ids=_ids(XGRAD))
def test_predict_grad(case):
    """predict_xgrad_kernel<T, DW, GLB, TWO, VAR>: DW = 2, 4, 8, 16, 32 (one term) and the global-memory windows of 16 coordinates
    (one term beyond 32, two terms beyond 16 dimensions), with and without the variance.  Bar of tests/test_gpu_predict_grad.py."""
    _, kernel, d = case
    c = dc.xgrad_reference(kernel, d)
    h = _lib.Handle(c["X"], c["y"], kernel, c["mean_kind"])
    assert h.fit(c["theta"]) == 0
    full = h.predict_grad(c["Xs"])
    mean_only = h.predict_grad(c["Xs"], variance=False)
    h.close()
    em, ev = _err(full[2], c["dmean"]), _err(full[3], c["dvar"])
    print(f"{dc.case_id(case)}: dmean {em:.3e} dvar {ev:.3e} of max |reference|; without the variance {_err(mean_only[2], c['dmean']):.3e}")
    assert full[2].shape == (dc.M_XGRAD, d) and full[3].shape == (dc.M_XGRAD, d) and mean_only[3] is None
    assert em <= XGRAD_BAR and ev <= XGRAD_BAR and _err(mean_only[2], c["dmean"]) <= XGRAD_BAR
    assert _err(full[0], c["mean"]) <= XGRAD_BAR and _err(full[1], c["var"]) <= XGRAD_BAR
    assert np.array_equal(mean_only[2], full[2])                  # dvar = NULL: dmean is the same bytes


SPARSE = dc.cases("sparse_zgrad_one_term") + dc.cases("sparse_zgrad_two_terms")


@pytest.mark.parametrize("case", SPARSE, ids=_ids(SPARSE))
def test_sparse_inducing_gradient_and_predict_grad(case):
    """sparse_zgrad_kernel<T, DW, GLB, TWO> and the sparse object's predict_xgrad launches at the same d.  Bars of
    tests/test_gpu_sparse_zgrad.py (1e-7 while the CPU routes agree to 1e-8) and tests/test_gpu_sparse_predict_grad.py."""
    _, kernel, d = case
    c = dc.sparse_reference(kernel, d)
    h = _lib.SparseHandle(c["X"], c["y"], c["Z"], kernel, c["mean_kind"])
    F, grad, gz, info = h.bound_grad_inducing(c["theta"], c["jitter"])
    F2, _, gz2, _ = h.bound_grad_inducing(c["theta"], c["jitter"])
    assert h.fit(c["theta"], c["jitter"]) == 0
    full = h.predict_grad(c["Xs"])
    mean_only = h.predict_grad(c["Xs"], variance=False)
    h.close()
    bar = zgrad_bar(c["route_difference"])
    em, ev = _err(full[2], c["dmean"]), _err(full[3], c["dvar"])
    print(f"{dc.case_id(case)}: dF/dZ {_err(gz, c['gradZ']):.3e} (bar {bar:.1e}); sparse dmean {em:.3e} dvar {ev:.3e}")
    assert info == 0 and gz.shape == (dc.M_INDUCING, d)
    assert _err(gz, c["gradZ"]) <= bar
    assert F == F2 and np.array_equal(gz, gz2)
    assert em <= SPARSE_XGRAD_BAR and ev <= SPARSE_XGRAD_BAR and mean_only[3] is None
    assert np.array_equal(mean_only[2], full[2])


# ---- pathwise draws ----
PATHS = dc.cases("paths")
assert PATHS == [("paths",) + c[1:] for c in dc.cases("paths_own")]      # one draw set per d serves both


@pytest.mark.parametrize("case", PATHS, ids=[dc.case_id(c).replace("paths-", "paths+paths_own-") for c in PATHS])
def test_paths_eval_and_eval_own(case):
    """paths_contract_kernel / paths_own_kernel<T, GEN, GRAD, DW>, DW = 8, 16, 32, 0, feature and kernel side, value and gradient
    (gradient windows of PC_GW = 4 / PO_GW = 8 coordinates).  Bars of tests/test_gpu_paths.py and tests/test_gpu_paths_own.py."""
    _, kernel, d = case
    c = dc.paths_data(kernel, d)
    S, F = dc.PATHS_SHAPE["S"], dc.PATHS_SHAPE["F"]
    h = _lib.Handle(c["X"], c["y"], kernel, c["mean_kind"])
    assert h.fit(c["theta"]) == 0
    with h.sample_paths(S, F, 2) as p:
        t = p.table()
        out, dout = p.eval(c["Xs"], grad=True)
        oo, od = p.eval_own(c["own"], grad=True)
        assert p.eval(c["Xs"]).tobytes() == out.tobytes() and p.eval_own(c["own"]).tobytes() == oo.tobytes()
    h.close()
    table = {"omega": t["omega"], "phase": t["phase"], "amp": _lib.rff_table(kernel, d, c["theta"], F, 2)[2]}
    a = (kernel, c["theta"], c["X"], c["y"])
    r = pr.paths(*a, c["Xs"], table, t["w"], t["eps"], c["mean_kind"])
    ro = por.paths_own(*a, c["own"], table, t["w"], t["eps"], c["mean_kind"])
    print(f"{dc.case_id(case)}: v {_err(t['v'], r['v']):.3e} out {_err(out, r['out']):.3e} dout {_err(dout, r['dout']):.3e}; "
          f"own out {_err(oo, ro['out']):.3e} dout {_err(od, ro['dout']):.3e}")
    assert dout.shape == (S, len(c["Xs"]), d) and od.shape == (S, 7, d)
    assert _err(t["v"], r["v"]) <= PATHS_BAR and _err(out, r["out"]) <= PATHS_BAR and _err(dout, r["dout"]) <= PATHS_BAR
    assert _err(oo, ro["out"]) <= PATHS_OWN_BAR and _err(od, ro["dout"]) <= PATHS_OWN_BAR


# ---- run-time compiled covariance function ----
RTC = dc.cases("rtc")


@pytest.mark.parametrize("case", RTC, ids=_ids(RTC))
def test_run_time_compiled_se_ard(case):
    """the program specialised for d (<= RTC_SPEC_MAXD = 32) and the generic one: covariance, likelihood and the dual-number
    gradient of the SE-ARD body against the se_ard oracle, at the named kernel's bars."""
    _, kernel, d = case
    c = dc.build_data(kernel, d)
    n, th = dc.N_BUILD, c["theta"]
    Ko, ko, kapo, want = _build_reference("se_ard", d)
    want_grad = orc.log_likelihood_grad("se_ard", th, c["X"], c["y"])
    h = _lib.Handle(c["X"], c["y"], _lib.CustomKernel(SE_ARD_BODY, d + 1, fn=se_ard_fn))
    K = h.covariance(th)
    k, kappa = h.cross_covariance(th, c["Xs"])
    np.testing.assert_allclose(K, Ko, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(k, ko, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(kappa, kapo, rtol=1e-12)
    _check_likelihood(h, c, want, n, 1e-8, dc.case_id(case))
    ll, grad, info = h.loglik_grad(th)
    print(f"{dc.case_id(case)}: K {np.abs(K / Ko - 1).max():.3e}; gradient {_err(grad, want_grad):.3e} of max |gradient|")
    assert info == 0 and h.get_option("grad_analytic") == 1 and close(ll, want[0], n)
    np.testing.assert_allclose(grad, want_grad, rtol=1e-7, atol=1e-7 * np.abs(want_grad).max())
    h.close()


# ---- two live handles ----
def test_two_live_general_form_handles():
    """A general-form handle at d = 32 (the largest dynamic-LDS request: 128 KiB for the build, 4 d + 1 tiles for the gradient), then
    one at d = 2 created while the first lives; covariance, likelihood and theta-gradient on the first, the second and the first
    again.  include/gphip.h promises that handles work side by side."""
    kernel = dc.TWO_TERM
    hs, cs = {}, {}
    for d in (32, 2):                                             # in this order: the later handle is the smaller one
        cs[d] = dc.build_data(kernel, d)
        hs[d] = _lib.Handle(cs[d]["X"], cs[d]["y"], kernel, cs[d]["mean_kind"])
    for d in (32, 2, 32):
        c, h = cs[d], hs[d]
        Ko, _, _, want = _build_reference(kernel, d)
        want_grad = lgr.log_likelihood_grad(kernel, c["theta"], c["X"], c["y"], c["mean_kind"])
        np.testing.assert_allclose(h.covariance(c["theta"]), Ko, rtol=1e-12, atol=1e-14)
        _check_likelihood(h, c, want, dc.N_BUILD, 1e-8, f"two handles, d = {d}")
        ll, grad, info = h.loglik_grad(c["theta"])
        print(f"two handles, d = {d}: gradient {_err(grad, want_grad):.3e}")
        assert info == 0 and close(ll, want[0], dc.N_BUILD)
        np.testing.assert_allclose(grad, want_grad, rtol=1e-7, atol=1e-7 * np.abs(want_grad).max())
    for h in hs.values():
        h.close()
