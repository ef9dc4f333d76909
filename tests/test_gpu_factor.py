"""The resident Cholesky factor held to its componentwise backward-error bound, on every schedule that can produce it.

For every row of tests/factor_cases.py: fit; read K-hat with covariance(theta) on a second handle with the same options (so the
kernel build is outside the verdict); read L-hat, z-hat and the 128-block inverses W-hat with Handle.factor; run the five checks of
tests/factor_reference.py (omega_factor, omega_solve, omega_inverse, the log-det and quadratic-form ties) against their derived
bars.  Which route ran is read off the per-class launch profile and compared with the row's launch counts.

The quadratic form of a fit is not exported by itself: it is read from loglik_parts on the same handle with the single-launch
evaluation ("fused_eval") off, which takes the schedule of the fit; its log det must be the fit's, bit for bit -- the witness that
both calls made the same factor."""
import numpy as np
import pytest

import factor_cases as fc
import factor_reference as fr
from bayesianinference_amd import _lib
from oracle import gp_oracle as orc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not fr.HAVE_LD, reason=fr.SKIP_REASON)]

CLASSES = ("potrf", "trsm", "gemm_panel", "syrk_trailing")
ERR_STATE = 4


def make_handle(case, X, y):
    h = _lib.Handle(X, y, case["kernel"], mean=case["mean"], dtype=case["dtype"])
    for name, value in case["opts"]:
        h.set_option(name, value)
        assert h.get_option(name) == value
    return h


def k_hat(case, X, y, th):
    """K as the device builds it for this row (fp32 handles: the widened fp32 values), from a handle of its own"""
    h2 = make_handle(case, X, y)
    K = h2.covariance(th)
    h2.close()
    return K


def quad_of_fit_route(h, th):
    fused = h.get_option("fused_eval")
    h.set_option("fused_eval", 0)
    _, logdet, quad, info = h.loglik_parts(th)
    h.set_option("fused_eval", fused)
    assert info == 0
    return logdet, quad


def fit_profiled(h, th):
    h.set_option("profile", 2)
    h.reset_profile()
    assert h.fit(th) == 0
    pr = h.profile()
    h.set_option("profile", 0)
    return tuple(int(pr[c]["launches"]) for c in CLASSES)


def fit_and_read(case):
    X, y, th = fc.inputs(case)
    h = make_handle(case, X, y)
    logdet_lik, quad = quad_of_fit_route(h, th)
    launches = fit_profiled(h, th)
    L, z, W = h.factor(winv=True)
    logdet = h.logdet()
    h.close()
    assert logdet == logdet_lik, "the likelihood call and the fit did not make the same factor: the quadratic form is not the fit's"
    return dict(X=X, y=y, th=th, L=L, z=z, W=W, logdet=logdet, quad=quad, launches=launches)


def judge(case, got, K=None, quad=True):
    K = k_hat(case, got["X"], got["y"], got["th"]) if K is None else K
    r = fc.residual(case, got["y"], got["th"])
    checks = fr.run_checks(K, got["L"], got["z"], r, got["W"], got["logdet"], got["quad"] if quad else fr.quad_from(got["z"]), case["dtype"])
    if not quad:
        del checks["quad"]
    print(fr.report(case["id"], checks))
    bad = fr.failed(checks)
    if "factor" in bad:                                           # where: the entries over the bar, by 128-tile and by 16-block
        om = np.asarray(fr.omega_factor_map(K, got["L"]), dtype=np.float64)
        ii, jj = np.nonzero(om > checks["factor"][1])
        print("  over the bar: %d entries, %d on the diagonal; tiles %s; worst (%d, %d) = %.3e" % (
            len(ii), int(np.sum(ii == jj)), sorted({(int(a) // 128, int(b) // 128) for a, b in zip(ii, jj)})[:12],
            *np.unravel_index(np.argmax(om), om.shape), om.max()))
    assert bad == [], checks
    return checks


def upper_is_zero_and_padding_is_identity(got, n):
    assert np.all(np.triu(got["L"], 1) == 0.0)
    for b, Wb in enumerate(got["W"]):
        assert np.all(np.triu(Wb, 1) == 0.0)
        m = min(fr.TB, n - b * fr.TB)
        assert np.array_equal(Wb[m:, m:], np.eye(fr.TB - m)) and np.all(Wb[m:, :m] == 0.0)


@pytest.mark.parametrize("case", fc.SIZE_EDGES, ids=[c["id"] for c in fc.SIZE_EDGES])
def test_size_edges(case):
    got = fit_and_read(case)
    assert got["launches"] == case["launches"], got["launches"]
    upper_is_zero_and_padding_is_identity(got, case["n"])
    judge(case, got)


@pytest.mark.parametrize("case", fc.SCHEDULES, ids=[c["id"] for c in fc.SCHEDULES])
def test_schedule_matrix(case):
    got = fit_and_read(case)
    assert got["launches"] == case["launches"], got["launches"]
    judge(case, got)


@pytest.mark.parametrize("case", fc.KERNELS, ids=[c["id"] for c in fc.KERNELS])
def test_other_covariance_forms(case):
    got = fit_and_read(case)
    assert got["launches"] == case["launches"], got["launches"]
    judge(case, got)


@pytest.mark.parametrize("sid", ["single-64", "mk-lookahead", "tail-64", "panel-df"])
def test_two_fits_give_the_same_bytes(sid):
    case = next(c for c in fc.SCHEDULES if c["id"] == "n641-" + sid)
    a, b = fit_and_read(case), fit_and_read(case)
    assert a["launches"] == b["launches"] == case["launches"]
    for k in ("L", "z", "W"):
        assert np.array_equal(a[k], b[k]), k
    assert a["logdet"] == b["logdet"] and a["quad"] == b["quad"]


def test_routes_the_launch_list_cannot_tell_apart_are_not_the_same_arithmetic():
    """64- and 128-tiles of the single launch show the same launch list; that both ran is seen in the bytes they leave"""
    a = fit_and_read(next(c for c in fc.SCHEDULES if c["id"] == "n641-single-64"))
    b = fit_and_read(next(c for c in fc.SCHEDULES if c["id"] == "n641-single-128"))
    assert not np.array_equal(a["L"], b["L"])
    assert np.max(np.abs(a["L"] - b["L"])) < 1e-10


@pytest.mark.parametrize("potri", [1, 0])
def test_factor_after_loglik_grad(potri):
    """the header says the factor of a gradient call stays resident: the K^-1 route must not have overwritten it"""
    case = fc.SIZE_EDGES[9]                                       # n = 385, fp64, default route
    X, y, th = fc.inputs(case)
    h = make_handle(case, X, y)
    h.set_option("grad_potri", potri)
    logdet_lik, quad = quad_of_fit_route(h, th)
    ll, grad, info = h.loglik_grad(th)
    assert info == 0 and np.all(np.isfinite(grad))
    L, z, W = h.factor(winv=True)
    got = dict(X=X, y=y, th=th, L=L, z=z, W=W, logdet=h.logdet(), quad=quad)
    assert got["logdet"] == logdet_lik
    judge(case, got)
    Xs = np.random.default_rng(5).uniform(-1, 1, size=(33, case["d"]))
    mu, var = h.predict(Xs)
    mo, so = orc.predict_internal(case["kernel"], th, X, y, Xs)
    np.testing.assert_allclose(mu, mo, rtol=1e-7, atol=1e-8)      # (the bars of smoke())
    np.testing.assert_allclose(np.sqrt(var), so, rtol=1e-7)
    L2, z2, W2 = h.factor(winv=True)                              # .. and the prediction left it alone too
    assert np.array_equal(L, L2) and np.array_equal(z, z2) and np.array_equal(W, W2)
    h.close()


@pytest.mark.parametrize("n,m", [(300, 70), (120, 9)])
def test_factor_after_extend(n, m):
    """gphip_extend appends rows to the resident factor: the new handle's factor against K-hat of the union (from a fresh handle on
    the concatenated data), its first n rows the parent's, bit for bit.  (No scalar of the quadratic form is exported there.)"""
    case = dict(fc.SIZE_EDGES[9], id="extend-%d+%d" % (n, m), n=n + m)
    X, y, th = fc.inputs(case)
    parent_case = dict(case, n=n)
    hp = make_handle(parent_case, X[:n], y[:n])
    assert hp.fit(th) == 0
    Lp, zp, Wp = hp.factor(winv=True)
    child, _, info = hp.extend(X[n:], y[n:])
    assert info == 0 and child is not None
    L, z, W = child.factor(winv=True)
    got = dict(X=X, y=y, th=th, L=L, z=z, W=W, logdet=child.logdet(), quad=None)
    assert np.array_equal(L[:n, :n], Lp) and np.array_equal(z[:n], zp)
    for b in range(n // fr.TB):                                   # the parent's whole diagonal blocks keep their inverses
        assert np.array_equal(W[b], Wp[b])
    judge(case, got, quad=False)
    Lp2, zp2, _ = hp.factor(winv=True)                            # the parent is untouched
    assert np.array_equal(Lp, Lp2) and np.array_equal(zp, zp2)
    child.close()
    hp.close()


def test_states_that_have_no_factor():
    case = fc.SIZE_EDGES[4]
    X, y, th = fc.inputs(case)
    h = make_handle(case, X, y)
    with pytest.raises(_lib.GphipError) as e:
        h.factor()
    assert e.value.status == ERR_STATE
    assert h.fit(th) == 0
    L, z = h.factor()
    assert L.shape == (case["n"], case["n"]) and z.shape == (case["n"],)
    h.covariance(th)                                              # overwrites the workspace: the fit is gone
    with pytest.raises(_lib.GphipError) as e:
        h.factor()
    assert e.value.status == ERR_STATE
    assert h.fit(th) == 0 and np.array_equal(h.factor()[0], L)    # .. and a new fit brings the same one back
    h.close()
    hn = _lib.Handle(X, y, "null")
    assert hn.fit(np.array([0.3])) == 0
    with pytest.raises(_lib.GphipError) as e:
        hn.factor()
    assert e.value.status == ERR_STATE
    hn.close()
