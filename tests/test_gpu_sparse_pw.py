"""The sparse inducing-point GP with a noise variance and a mean that depend on the point (gphip_sparse_*_pw) on the device against
the numpy reference of tests/sparse_pw_reference.py (pinned on the CPU by tests/test_sparse_pw.py).  Bars are those of
tests/test_gpu_sparse.py: 1e-8 relative for F and each of its parts, 1e-7 x max |y| for predicted means, 1e-7 x max k(x, x) for
variances, 1e-12 between the routes of one computation.

Measured on MI355X: see the table there; every case prints its errors."""
import ctypes

import numpy as np
import pytest

import sparse_batch_cases as bc
import sparse_pw_reference as pw
import sparse_reference as ref
from bayesianinference_amd import _lib, gaussian_process as gp, nested_sampling as ns, synthetic as syn

pytestmark = pytest.mark.gpu

JIT = pw.JITTER


def _rel(a, b):
    return abs(a - b) / abs(b)


def _case(name, n, d, m, mean):
    X, y = syn.make_dataset(n, d)
    kernel, th = pw.kernel_of(name, d), pw.theta(name, d, mean)
    Z = pw.inducing(X, m, syn.make_test_points(max(m - n, 1), d))
    sn2, _ = ref.noise_and_mean(kernel, th, d, mean)
    return X, y, kernel, th, Z, sn2


def _check_bound(h, want, label, tol=1e-8, **arrays):
    F, parts, info = h.bound_pw(want["th"], JIT, parts=True, **arrays)
    errs = [_rel(a, b) for a, b in zip(parts, want["parts"])]
    print(f"{label}: F {F:.8f} reference {want['F']:.8f} rel {_rel(F, want['F']):.2e} parts {[f'{e:.1e}' for e in errs]}")
    assert info == 0
    assert _rel(F, want["F"]) <= tol and max(errs) <= tol
    return F, parts


@pytest.fixture(scope="module")
def base():
    """(1333, 3, 150), SE-ARD, constant mean in theta: data, arrays and the numpy bound, computed once"""
    X, y, kernel, th, Z, sn2 = _case("se_ard", 1333, 3, 150, "const")
    nu, mv = pw.noise(X, sn2), pw.trend(X)
    want = pw.bound_formulas(kernel, th, X, y, Z, JIT, mv, nu, "const")
    want["th"] = th
    return {"X": X, "y": y, "th": th, "Z": Z, "sn2": sn2, "nu": nu, "mv": mv, "want": want}


# ---- 1. parity against numpy
@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name,n,d,m,mean", pw.CASES)
def test_bound_parts_and_prediction_match_numpy(name, n, d, m, mean, fused):
    X, y, kernel, th, Z, sn2 = _case(name, n, d, m, mean)
    nu, mv = pw.noise(X, sn2), pw.trend(X)
    label = f"{name} N={n} d={d} m={m} {mean} fused={fused}"
    h = _lib.SparseHandle(X, y, Z, kernel, mean)
    h.set_option("sparse_pw_fused", fused)                      # the weight inside the contraction / the scaling pass ahead of it
    want = pw.bound_formulas(kernel, th, X, y, Z, JIT, mv, nu, mean)
    want["th"] = th
    _check_bound(h, want, label, mean_train=mv, nugget_train=nu)
    Xs = syn.make_test_points(77, d)
    mt, nt = pw.trend(Xs), pw.noise(Xs, sn2)
    scale = float(ref.kdiag(kernel, th, X, mean).max())
    for latent in (False, True):
        mu, var = h.predict_pw(Xs, latent, mt, nt)
        wm, wv = pw.predict_formulas(kernel, th, X, y, Z, JIT, Xs, mv, nu, mt, nt, mean, latent)
        em, ev = np.abs(mu - wm).max() / np.abs(y).max(), np.abs(var - wv).max() / scale
        print(f"{label} latent={latent}: mean {em:.2e} var {ev:.2e}")
        assert em <= 1e-7 and ev <= 1e-7
    h.close()


# ---- 2. routes
def test_routes_agree_with_the_default_and_repeat_bit_for_bit():
    X, y, kernel, th, Z, sn2 = _case("se_ard", 1500, 3, 300, "zero")
    nu, mv = pw.noise(X, sn2), pw.trend(X)
    want = pw.bound_formulas(kernel, th, X, y, Z, JIT, mv, nu, "zero")
    h = _lib.SparseHandle(X, y, Z, kernel, "zero")
    defaults = {"sparse_chunk": 0, "sparse_split": 0, "dataflow": h.get_option("dataflow"), "sparse_pw_fused": h.get_option("sparse_pw_fused")}
    assert defaults["sparse_pw_fused"] == 0                      # (the measurement of DESIGN.md section 8i decided it)
    vals = {}
    for key, opts in (("default", {}), ("chunk512", {"sparse_chunk": 512}), ("split3", {"sparse_split": 3}), ("dataflow0", {"dataflow": 0}),
                      ("unfused", {"sparse_pw_fused": 0}), ("fused", {"sparse_pw_fused": 1}), ("fused chunk512", {"sparse_pw_fused": 1, "sparse_chunk": 512}),
                      ("fused split3", {"sparse_pw_fused": 1, "sparse_split": 3})):
        for k, v in {**defaults, **opts}.items():
            h.set_option(k, v)
        F1, p1, i1 = h.bound_pw(th, JIT, mv, nu, parts=True)
        F2, p2, i2 = h.bound_pw(th, JIT, mv, nu, parts=True)
        assert i1 == 0 and i2 == 0 and F1 == F2 and np.array_equal(p1, p2), key           # the same bytes
        vals[key] = F1
        print(key, F1, _rel(F1, want["F"]), h.get_option("last_sparse_chunk"), h.get_option("last_sparse_nsplit"))
        if key.endswith("chunk512"):
            assert h.get_option("last_sparse_chunk") == 512       # three chunks, the last partial (1500 = 512 + 512 + 476)
        if key.endswith("split3"):
            assert h.get_option("last_sparse_nsplit") == 3
    for key, F in vals.items():
        assert _rel(F, vals["default"]) <= 1e-12, key
        assert _rel(F, want["F"]) <= 1e-8, key
    h.close()


# ---- 3. four decades of noise
def test_four_decades_of_noise():
    X, y, kernel, th, Z, sn2 = _case("se_ard", 1333, 3, 150, "zero")
    nu = pw.noise_decades(X, sn2)
    assert nu.max() / nu.min() > 5e3
    want = pw.bound_formulas(kernel, th, X, y, Z, JIT, None, nu, "zero")
    want["th"] = th
    h = _lib.SparseHandle(X, y, Z, kernel, "zero")
    _check_bound(h, want, "four decades", nugget_train=nu)
    h.close()


# ---- 4. consistency with the constant path
def test_consistency_with_the_constant_path(base):
    X, y, th, Z, sn2, nu, mv = (base[k] for k in ("X", "y", "th", "Z", "sn2", "nu", "mv"))
    n, m = len(X), len(Z)
    Xs = syn.make_test_points(77, 3)
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const")
    F0, p0, i0 = h.bound_parts(th, JIT)
    g0 = h.bound_grad(th, JIT)
    pr0 = h.predict(Xs)
    # both arrays NULL: the constant call's bytes, its five parts converted
    F, p6, info = h.bound_pw(th, JIT, parts=True)
    assert info == 0 and F == F0
    conv = np.array([p0[0] - m * np.log(sn2), p0[1] / sn2, p0[2] / sn2, p0[3] / sn2, p0[4] / sn2, n * np.log(sn2)])
    assert np.allclose(p6, conv, rtol=1e-13, atol=0.0)           # (converted on the host: one rounding per part)
    Fb, ib = h.bound_batch_pw(th[None, :], JIT)
    Fc, ic = h.bound_batch(th[None, :], JIT)
    assert ib[0] == 0 and Fb[0] == Fc[0]
    # arrays filled with sn^2 and mu
    Fk, info = h.bound_pw(th, JIT, np.full(n, th[-1]), np.full(n, sn2))
    print(f"constant arrays against the constant call: {_rel(Fk, F0):.2e}")
    assert info == 0 and _rel(Fk, F0) <= 1e-8
    # one array alone
    for label, ma, na in (("mean alone", mv, None), ("nugget alone", None, nu)):
        want = pw.bound_formulas("se_ard", th, X, y, Z, JIT, ma, na, "const")
        want["th"] = th
        _check_bound(h, want, label, mean_train=ma, nugget_train=na)
    # fit_pw, then the plain predict: theta's sn^2 and mu at the test points
    assert h.fit_pw(th, JIT, mv, nu) == 0
    for latent in (False, True):
        mu, var = h.predict(Xs, latent=latent)
        wm, wv = pw.predict_formulas("se_ard", th, X, y, Z, JIT, Xs, mv, nu, None, None, "const", latent)
        em, ev = np.abs(mu - wm).max() / np.abs(y).max(), np.abs(var - wv).max() / pw.SF ** 2
        print(f"predict after fit_pw latent={latent}: mean {em:.2e} var {ev:.2e}")
        assert em <= 1e-7 and ev <= 1e-7
    # predict_pw works after a constant fit as well
    assert h.fit(th, JIT) == 0
    mt, nt = pw.trend(Xs), pw.noise(Xs, sn2)
    mu, var = h.predict_pw(Xs, False, mt, nt)
    wm, wv = ref.predict_formulas("se_ard", th, X, y, Z, JIT, Xs, "const", False)
    assert np.abs(mu - (wm - th[-1] + mt)).max() <= 1e-7 * np.abs(y).max() and np.abs(var - (wv - sn2 + nt)).max() <= 1e-7 * pw.SF ** 2
    # the constant path returns the same bytes after the pw calls
    F1, p1, i1 = h.bound_parts(th, JIT)
    g1 = h.bound_grad(th, JIT)
    pr1 = h.predict(Xs)
    assert (F1, i1) == (F0, i0) and np.array_equal(p1, p0)
    assert g1[0] == g0[0] and np.array_equal(g1[1], g0[1]) and g1[2] == g0[2]
    assert np.array_equal(pr1[0], pr0[0]) and np.array_equal(pr1[1], pr0[1])
    h.close()


# ---- 5. batch
def _row_arrays(X, rows):
    """arrays that depend on the row's theta: nu = sn_s^2 s(x)^2, m = mu_s + 0.3 x_1"""
    nug = np.array([pw.noise(X, r[-2] ** 2) for r in rows])
    mean = np.array([r[-1] + 0.3 * X[:, 0] for r in rows])
    return mean, nug


def test_batch_rows_match_numpy_repeat_and_permute(base):
    X, y, Z = base["X"], base["y"], base["Z"]
    rows = bc.theta_rows("se_ard", 3, "const", 6)
    mean, nug = _row_arrays(X, rows)
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const")
    h.set_option("sparse_batch_slots", 4)                        # two groups: 4 + 2
    F, info, parts = h.bound_batch_pw(rows, JIT, mean, nug, parts=True)
    F2, info2, parts2 = h.bound_batch_pw(rows, JIT, mean, nug, parts=True)
    assert np.array_equal(F, F2) and np.array_equal(info, info2) and np.array_equal(parts, parts2)
    for s, th in enumerate(rows):
        want = pw.bound_formulas("se_ard", th, X, y, Z, JIT, mean[s], nug[s], "const")
        errs = [_rel(a, b) for a, b in zip(parts[s], want["parts"])]
        print(f"row {s}: F rel {_rel(F[s], want['F']):.2e} parts {max(errs):.1e}")
        assert info[s] == 0 and _rel(F[s], want["F"]) <= 1e-8 and max(errs) <= 1e-8
    h.set_option("sparse_batch_slots", 0)                        # one group: a row's bytes do not depend on its place
    Fa, ia, pa = h.bound_batch_pw(rows, JIT, mean, nug, parts=True)
    perm = np.array([3, 0, 5, 1, 4, 2])
    Fp, ip, pp = h.bound_batch_pw(rows[perm], JIT, mean[perm], nug[perm], parts=True)
    assert h.get_option("last_sparse_slots") == 6
    assert np.array_equal(Fp, Fa[perm]) and np.array_equal(pp, pa[perm]) and np.array_equal(ip, ia[perm])
    h.close()


@pytest.mark.parametrize("what", ["nu zero", "nu negative", "nu nan", "nu inf", "mean nan"])
def test_a_row_with_unusable_arrays_fails_alone(base, what):
    X, y, Z = base["X"], base["y"], base["Z"]
    rows = bc.theta_rows("se_ard", 3, "const", 7)
    mean, nug = _row_arrays(X, rows)
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const")
    h.set_option("sparse_batch_slots", 4)
    good = h.bound_batch_pw(rows, JIT, mean, nug, parts=True)
    bad_mean, bad_nug = mean.copy(), nug.copy()
    k = 2                                                        # a row inside the first group, entry 700 of its array
    if what == "mean nan":
        bad_mean[k, 700] = np.nan
    else:
        bad_nug[k, 700] = {"nu zero": 0.0, "nu negative": -1e-3, "nu nan": np.nan, "nu inf": np.inf}[what]
    F, info, parts = h.bound_batch_pw(rows, JIT, bad_mean, bad_nug, parts=True)
    h.close()
    assert info[k] == _lib.INFO_NAN == 2 and np.isnan(F[k]) and np.all(np.isnan(parts[k]))
    others = np.arange(7) != k
    assert np.all(info[others] == 0)
    assert np.array_equal(F[others], good[0][others]) and np.array_equal(parts[others], good[2][others])


# ---- 6. posterior samples
def test_predict_samples_pw_matches_numpy_and_the_batched_bound(base):
    X, y, Z = base["X"], base["y"], base["Z"]
    rows = bc.theta_rows("se_ard", 3, "const", 4)
    mean, nug = _row_arrays(X, rows)
    Xs = syn.make_test_points(77, 3)
    mt, nt = _row_arrays(Xs, rows)
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const")
    for latent in (False, True):
        mu, var, info, F = h.predict_samples_pw(rows, Xs, JIT, latent, mean, nug, mt, nt, bound=True)
        assert np.all(info == 0)
        for s, th in enumerate(rows):
            wm, wv = pw.predict_formulas("se_ard", th, X, y, Z, JIT, Xs, mean[s], nug[s], mt[s], nt[s], "const", latent)
            em, ev = np.abs(mu[s] - wm).max() / np.abs(y).max(), np.abs(var[s] - wv).max() / th[3] ** 2
            print(f"sample {s} latent={latent}: mean {em:.2e} var {ev:.2e}")
            assert em <= 1e-7 and ev <= 1e-7
    Fb, ib = h.bound_batch_pw(rows, JIT, mean, nug)               # the same group size: the same bytes
    assert np.array_equal(F, Fb) and np.all(ib == 0)
    h.close()


# ---- 7. fp32
def test_fp32_pw_errors_stay_within_four_times_the_constant_calls():
    """fp32 objects against the fp64 numpy references at N = 2000, d = 3, m = 300 (the case of the constant fp32 test), default fp32
    jitter.  The pw errors may be at most 4 x the constant call's errors measured in the same test: one more rounding per product
    (the weight) and a different summation.  The errors are those of the constant test -- F, the parts, means, variances -- each
    compared with its own counterpart.  log det B is compared by its ABSOLUTE error: that is the relative error of det B, which the
    factor sn^(2 m) between the two definitions of B (sn^2 I + V V^T there, I + V W V^T here) does not change, while the relative
    error of the logarithm divides the same error by another number (-903.1 there, 242.7 here).  The other parts scale with B.
    Measured on MI355X, constant / pw with the scaling pass / pw with the weight in the kernel: F 1.99e-5 / 3.42e-5 / 2.80e-5,
    |log det B| 4.58e-3 / 6.33e-3 / 6.33e-3 (as relative errors of the two logarithms 5.07e-6 / 2.61e-5 / 2.61e-5, which is 5.1 x:
    that comparison would fail; with arrays filled with sn^2 and mu, the same model through the pw path, 4.70e-3), other parts
    1.17e-6 / 1.2e-6 / 9.6e-7, means 5.49e-5 / 1.15e-4 / 1.16e-4 of max |y|, variances 3.99e-6 / 3.80e-6 / 3.80e-6 of sf^2;
    cond(B) is 5.0e4 for the constant model and 9.8e4 for this one."""
    X, y = syn.make_dataset(2000, 3)
    th, Z = pw.theta("se_ard", 3, "const"), pw.inducing(X, 300, None)
    sn2 = th[-2] ** 2
    nu, mv = pw.noise(X, sn2), pw.trend(X)
    Xs = syn.make_test_points(77, 3)
    mt, nt = pw.trend(Xs), pw.noise(Xs, sn2)
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const", dtype=32)
    F, parts, info = h.bound_parts(th)
    jit = h.get_option("last_jitter")
    assert info == 0 and jit == pytest.approx(1e-4 * pw.SF ** 2, rel=1e-12)
    mu, var = h.predict(Xs)
    want = ref.bound_formulas("se_ard", th, X, y, Z, jit, "const")
    wm, wv = ref.predict_formulas("se_ard", th, X, y, Z, jit, Xs, "const")
    const = {"F": _rel(F, want["F"]), "logdet_abs": abs(parts[0] - want["parts"][0]),
             "parts": max(_rel(a, b) for a, b in zip(parts[1:], want["parts"][1:])),
             "mean": np.abs(mu - wm).max() / np.abs(y).max(), "var": np.abs(var - wv).max() / pw.SF ** 2}
    print("fp32 constant:", {k: f"{v:.2e}" for k, v in const.items()}, f"log det B relative {_rel(parts[0], want['parts'][0]):.2e}")
    wantp = pw.bound_formulas("se_ard", th, X, y, Z, jit, mv, nu, "const")
    wmp, wvp = pw.predict_formulas("se_ard", th, X, y, Z, jit, Xs, mv, nu, mt, nt, "const")
    for fused in (0, 1):
        h.set_option("sparse_pw_fused", fused)
        Fp, pp, info = h.bound_pw(th, -1.0, mv, nu, parts=True)
        assert info == 0 and h.get_option("last_jitter") == jit
        mup, varp = h.predict_pw(Xs, False, mt, nt)
        got = {"F": _rel(Fp, wantp["F"]), "logdet_abs": abs(pp[0] - wantp["parts"][0]),
               "parts": max(_rel(a, b) for a, b in zip(pp[1:], wantp["parts"][1:])),
               "mean": np.abs(mup - wmp).max() / np.abs(y).max(), "var": np.abs(varp - wvp).max() / pw.SF ** 2}
        print(f"fp32 pw fused={fused}:", {k: f"{v:.2e}" for k, v in got.items()}, f"log det B relative {_rel(pp[0], wantp['parts'][0]):.2e}")
        for k in const:
            assert got[k] <= 4.0 * const[k], (k, fused)
    h.close()


# ---- 8. statuses and the host layer
def test_statuses(base):
    X, y, th, Z, nu, mv = (base[k] for k in ("X", "y", "th", "Z", "nu", "mv"))
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const")
    lib, hh = _lib.load(), h._h
    dp = ctypes.POINTER(ctypes.c_double)
    d = lambda a: a.ctypes.data_as(dp)
    p, n = len(th), len(X)
    val, info = ctypes.c_double(0.0), ctypes.c_int(-1)
    out, inf2 = np.zeros(2), np.zeros(2, dtype=np.int32)
    ip = inf2.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    Xs = syn.make_test_points(5, 3)
    m5, v5 = np.zeros(10), np.zeros(10)
    th2 = np.ascontiguousarray(np.vstack([th, th]))
    ARG, DIM, STATE, UNSUPPORTED = 1, 2, 4, 6
    # NULL pointers
    assert lib.gphip_sparse_bound_pw(None, d(th), p, JIT, None, d(nu), ctypes.byref(val), None, ctypes.byref(info)) == ARG
    assert lib.gphip_sparse_bound_pw(hh, None, p, JIT, None, d(nu), ctypes.byref(val), None, ctypes.byref(info)) == ARG
    assert lib.gphip_sparse_bound_pw(hh, d(th), p, JIT, None, d(nu), None, None, ctypes.byref(info)) == ARG
    assert lib.gphip_sparse_bound_pw(hh, d(th), p, JIT, None, d(nu), ctypes.byref(val), None, None) == ARG
    assert lib.gphip_sparse_bound_batch_pw(hh, None, 2, p, JIT, None, None, d(out), None, ip) == ARG
    assert lib.gphip_sparse_bound_batch_pw(hh, d(th2), 2, p, JIT, None, None, None, None, ip) == ARG
    assert lib.gphip_sparse_fit_pw(hh, d(th), p, JIT, None, d(nu), None) == ARG
    assert lib.gphip_sparse_predict_pw(hh, None, 5, 0, None, None, d(m5), d(v5)) == ARG
    assert lib.gphip_sparse_predict_pw(hh, Xs.ctypes.data, 5, 0, None, None, None, d(v5)) == ARG
    assert lib.gphip_sparse_predict_samples_pw(hh, None, 2, p, JIT, None, None, Xs.ctypes.data, 5, 0, None, None, d(m5), d(v5), None, ip) == ARG
    assert lib.gphip_sparse_predict_samples_pw(hh, d(th2), 2, p, JIT, None, None, Xs.ctypes.data, 5, 0, None, None, d(m5), d(v5), None, None) == ARG
    # a non-finite jitter, a wrong p, S or M < 1
    for bad in (float("nan"), float("inf")):
        assert lib.gphip_sparse_bound_pw(hh, d(th), p, bad, None, d(nu), ctypes.byref(val), None, ctypes.byref(info)) == ARG
        assert lib.gphip_sparse_bound_batch_pw(hh, d(th2), 2, p, bad, None, None, d(out), None, ip) == ARG
        assert lib.gphip_sparse_fit_pw(hh, d(th), p, bad, None, d(nu), ctypes.byref(info)) == ARG
        assert lib.gphip_sparse_predict_samples_pw(hh, d(th2), 2, p, bad, None, None, Xs.ctypes.data, 5, 0, None, None, d(m5), d(v5), None, ip) == ARG
    assert lib.gphip_sparse_bound_pw(hh, d(th), p - 1, JIT, None, d(nu), ctypes.byref(val), None, ctypes.byref(info)) == DIM
    assert lib.gphip_sparse_bound_batch_pw(hh, d(th2), 2, p + 1, JIT, None, None, d(out), None, ip) == DIM
    assert lib.gphip_sparse_fit_pw(hh, d(th), p + 1, JIT, None, d(nu), ctypes.byref(info)) == DIM
    assert lib.gphip_sparse_predict_samples_pw(hh, d(th2), 0, p, JIT, None, None, Xs.ctypes.data, 5, 0, None, None, d(m5), d(v5), None, ip) == DIM
    assert lib.gphip_sparse_predict_samples_pw(hh, d(th2), 2, p, JIT, None, None, Xs.ctypes.data, 0, 0, None, None, d(m5), d(v5), None, ip) == DIM
    assert lib.gphip_sparse_predict_samples_pw(hh, d(th2), 2, p - 1, JIT, None, None, Xs.ctypes.data, 5, 0, None, None, d(m5), d(v5), None, ip) == DIM
    # prediction before a fit; M < 1
    assert lib.gphip_sparse_predict_pw(hh, Xs.ctypes.data, 5, 0, None, None, d(m5), d(v5)) == STATE
    assert lib.gphip_sparse_predict_pw(hh, Xs.ctypes.data, 0, 0, None, None, d(m5), d(v5)) == DIM
    # an unusable array on the one-theta calls: info, NaN, no fit
    bad_nu = nu.copy()
    bad_nu[11] = 0.0
    F, parts, inf = h.bound_pw(th, JIT, mv, bad_nu, parts=True)
    assert inf == _lib.INFO_NAN and np.isnan(F) and np.all(np.isnan(parts))
    assert h.fit_pw(th, JIT, mv, bad_nu) == _lib.INFO_NAN
    with pytest.raises(_lib.GphipError) as e:
        h.predict_pw(Xs)
    assert e.value.status == STATE
    # the joint calls after a pw fit
    assert h.fit_pw(th, JIT, mv, nu) == 0
    for call in (lambda: h.predict_cov(Xs), lambda: h.predict_draws(Xs, 2, seed=1), lambda: h.predict_logpdf(Xs, np.zeros(5))):
        with pytest.raises(_lib.GphipError) as e:
            call()
        assert e.value.status == UNSUPPORTED
    assert h.fit(th, JIT) == 0                                    # a constant fit makes them available again
    h.predict_cov(Xs)
    assert h.fit_pw(th, JIT) == 0                                 # ... and so does a pw fit without an array
    h.predict_cov(Xs)
    with pytest.raises(_lib.GphipError) as e:                     # the Python layer checks the arrays' sizes
        h.bound_pw(th, JIT, mv[:-1], nu)
    assert e.value.status == DIM
    h.close()


def test_define_sparse_gaussian_process_with_callable_nugget_and_mean():
    X, y = syn.make_dataset(900, 2)
    variables = [("l1", 0.2, 3.0), ("l2", 0.2, 3.0), ("sf", 0.3, 3.0), ("sn", 0.03, 0.5)]
    nugget = lambda P, th: pw.noise(P, th[3] ** 2)
    trend = lambda P, th: 0.1 * th[2] + 0.3 * np.atleast_2d(P)[:, 0]
    obj = gp.defineSparseGaussianProcess((X, y), "SEARD", 100, nugget=nugget, meanFunction=trend, variables=variables, Jitter=JIT)
    assert not obj.failed and obj["MeanName"] == "zero"
    h, Z = obj["SparseGaussianProcessData"]["HIPHandle"], obj["InducingPoints"]
    th = np.array([0.9, 1.1, 1.0, 0.12])
    F, info = h.bound_pw(th, JIT, trend(X, th), nugget(X, th))
    want = pw.bound_formulas("se_ard", th, X, y, Z, JIT, trend(X, th), nugget(X, th), "zero")["F"]
    assert info == 0 and _rel(F, want) <= 1e-8
    assert obj["LogLikelihoodFunction"](th) == F
    rows = th[None, :] * np.random.default_rng(5).uniform(0.9, 1.1, size=(8, 4))
    vals = obj["LogLikelihoodFunction"](rows)
    Fb, ib = h.bound_batch_pw(rows, JIT, np.array([trend(X, r) for r in rows]), np.array([nugget(X, r) for r in rows]))
    assert vals.shape == (8,) and np.all(ib == 0) and np.array_equal(vals, Fb)
    # the gradient closure is the difference quotient: against the same quotient of the numpy bound
    val, grad = obj["LogLikelihoodGradientFunction"](th)
    assert val == F and np.all(np.isfinite(grad))
    quot = np.zeros(4)
    for k in range(4):
        step = np.finfo(np.float64).eps ** (1.0 / 3.0) * max(abs(th[k]), 1e-2)
        tp, tm = th.copy(), th.copy()
        tp[k] += step
        tm[k] -= step
        fp = pw.bound_formulas("se_ard", tp, X, y, Z, JIT, trend(X, tp), nugget(X, tp), "zero")["F"]
        fm = pw.bound_formulas("se_ard", tm, X, y, Z, JIT, trend(X, tm), nugget(X, tm), "zero")["F"]
        quot[k] = (fp - fm) / (tp[k] - tm[k])
    err = np.abs(grad - quot).max() / np.abs(quot).max()
    print(f"difference quotient against numpy's: {err:.2e}")
    assert err <= 2e-6
    # prediction for one theta and for a taken sample set, against the handle
    P = syn.make_test_points(9, 2)
    one = gp.predictFromSparseGaussianProcess(obj, P, theta=th)
    assert h.fit_pw(th, JIT, trend(X, th), nugget(X, th)) == 0
    mu, var = h.predict_pw(P, False, trend(P, th), nugget(P, th))
    assert np.array_equal(one["Mean"][0], mu) and np.array_equal(one["StandardDeviation"][0], np.sqrt(var))
    wm, wv = pw.predict_formulas("se_ard", th, X, y, Z, JIT, P, trend(X, th), nugget(X, th), trend(P, th), nugget(P, th), "zero")
    assert np.abs(mu - wm).max() <= 1e-7 * np.abs(y).max() and np.abs(var - wv).max() <= 1e-7
    res = ns.nestedSampling(obj, SamplePoolSize=12, MaxIterations=16, MinIterations=6, Seed=3)
    assert not isinstance(res, str) and "Samples" in res
    top = ns.inferenceObject_take(res, 4)
    pred = gp.predictFromSparseGaussianProcess(top, P)
    pts = np.array([s["Point"] for s in top["Samples"]])
    ms, vs, info = h.predict_samples_pw(pts, P, JIT, False, np.array([trend(X, r) for r in pts]), np.array([nugget(X, r) for r in pts]),
                                        np.array([trend(P, r) for r in pts]), np.array([nugget(P, r) for r in pts]))
    assert np.all(info == 0) and np.array_equal(pred["Mean"], ms) and np.array_equal(pred["StandardDeviation"], np.sqrt(vs))
    for call in (lambda: gp.predictJointFromSparseGaussianProcess(obj, P, th), lambda: gp.sparsePredictiveLogDensity(obj, (P, np.zeros(9)), th)):
        with pytest.raises(ValueError, match="point-dependent"):
            call()
    h.close()
