"""gphip_extend on the device: new observations into a resident fit without refactoring it.  The extended handle and a fresh
handle on the concatenated data are held to the same numpy references (tests/extend_reference.py: the reference of
tests/test_gpu_predict_joint.py on the concatenated data; tests/predict_grad_reference.py) at the bars those files' device tests
use; whatever rebuilds K must return the fresh handle's bytes.  The block identity itself is pinned on the CPU by
tests/test_extend.py.  Largest extended-against-fresh differences measured on an MI355X: DESIGN.md section 8k."""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sla

import extend_reference as er
import predict_grad_reference as pg
from bayesianinference_amd import _lib, gaussian_process as gp, synthetic as syn
from oracle import gp_oracle as orc

pytestmark = pytest.mark.gpu

# the bars of tests/test_gpu_predict_joint.py: absolute, for quantities of order sf^2 = 1
BAR = {64: 1e-9, 32: 2e-3}
BAR_LARGE = 1e-8                                   # that file's bar above N = 4096
GRAD_BAR = 1e-8                                    # tests/test_gpu_predict_grad.py, of max |reference|
_refs = {}


def _case(kname, d, mean, n, m):
    """data and CPU references of one case on the concatenated data, computed once and left unchanged"""
    key = (kname, d, mean, n, m)
    if key not in _refs:
        kernel, th = er.kernel_of(kname, d), er.theta_of(kname, d, mean)
        X, y, Xn, yn, Xs = er.case_data(n, m, d)
        Xc, yc = np.vstack([X, Xn]), np.concatenate([y, yn])
        mu, S, _ = er.reference(kernel, th, Xc, yc, Xs, mean)
        K = orc.covariance_matrix(kernel, th, Xc, mean)
        x0 = syn.normal(syn.STREAM_THETA, 0, n + m)             # a solve whose answer is of order 1, as the bar assumes
        b = K @ x0
        cf = sla.cho_factor(K, lower=True)
        c = {"kernel": kernel, "theta": th, "X": X, "y": y, "Xn": Xn, "yn": yn, "Xs": Xs, "Xc": Xc, "yc": yc, "mu": mu, "S": S,
             "b": b, "x": sla.cho_solve(cf, b), "logdet": 2.0 * np.log(np.diag(cf[0])).sum(),
             "z": np.random.default_rng(3).standard_normal((5, len(Xs)))}
        c["draws"] = mu + c["z"] @ np.linalg.cholesky(S + 1e-8 * np.eye(len(Xs))).T
        if kname != "custom":                                   # (gphip_predict_grad does not take run-time compiled kernels)
            c["grad"] = pg.exact(kernel, th, Xc, yc, Xs, mean)
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[key] = c
    return _refs[key]


def _rel(g, want):
    return float(np.abs(g - want).max() / np.abs(want).max())


def _meets_the_bars(h, c, dtype, label):
    """bar 1 (values against numpy) and bar 4 (gradients, draws) on a handle with the fit of c's theta on the concatenated data"""
    bar = BAR[dtype]
    pm, pv = h.predict(c["Xs"])
    mean, cov = h.predict_cov(c["Xs"])
    x = h.solve(c["b"])
    ld = h.logdet()
    draws, info = h.predict_draws(c["Xs"], len(c["z"]), z=c["z"], latent=False, jitter=1e-8)
    errs = {"mean": np.abs(pm - c["mu"]).max(), "var": np.abs(pv - np.diag(c["S"])).max(), "cov": np.abs(cov - c["S"]).max(),
            "cov mean": np.abs(mean - c["mu"]).max(), "solve": np.abs(x - c["x"]).max(),
            "logdet": abs(ld - c["logdet"]), "draws": np.abs(draws - c["draws"]).max()}
    print(f"{label}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bar {bar:.0e})")
    assert info == 0
    for k, v in errs.items():
        assert v <= bar, (label, k, v)
    out = {"predict": (pm, pv), "cov": cov, "solve": x, "logdet": ld}
    if "grad" in c:
        g = h.predict_grad(c["Xs"])
        em, ev = _rel(g[2], c["grad"]["dmean"]), _rel(g[3], c["grad"]["dvar"])
        # fp32: 10 x the relative error of the handle's own predictive mean, as tests/test_gpu_predict_grad.py
        gbar = GRAD_BAR if dtype == 64 else 10 * _rel(pm, c["grad"]["mean"])
        print(f"{label}: dmean {em:.2e} dvar {ev:.2e} (bar {gbar:.1e})")
        assert em <= gbar and ev <= gbar, label
        out["grad"] = g
    return out


def _fitted(c, mean, dtype, opts=None, data=("X", "y")):
    h = _lib.Handle(c[data[0]], c[data[1]], c["kernel"], mean, dtype=dtype)
    for k, v in (opts or {}).items():
        h.set_option(k, v)
    return h


PARAMS = [(k, d, mean, 64, 300, 130, {}) for (k, d, mean) in er.KERNELS] + \
         [("se_ard", 3, "zero", 32, 300, 130, {}), ("se_ard", 3, "zero", 64, 300, 130, {"dataflow": 0})] + \
         [("se_ard", 3, "zero", 64, n, m, {}) for (n, m) in er.SHAPES[1:]]
IDS = [f"{k}-d{d}-{mean}-fp{dt}-{n}+{m}" + ("-lookahead" if o else "") for (k, d, mean, dt, n, m, o) in PARAMS]


@pytest.mark.parametrize("kname,d,mean,dtype,n,m,opts", PARAMS, ids=IDS)
def test_extended_handle_is_a_fitted_handle_on_the_concatenated_data(kname, d, mean, dtype, n, m, opts):
    c = _case(kname, d, mean, n, m)
    th, Xs = c["theta"], c["Xs"]
    h = _fitted(c, mean, dtype, opts)
    ll_parent = h.loglik(th)[0]
    assert h.fit(th) == 0
    before = h.predict(Xs)
    want_logp, linfo = h.predict_logpdf(c["Xn"], c["yn"])
    ext, logp, info = h.extend(c["Xn"], c["yn"])
    assert info == 0 and linfo == 0 and ext is not None
    assert (ext.N, ext.d, ext.p, ext.dtype, ext.mean) == (n + m, d, h.p, dtype, mean) and ext.kernel is h.kernel
    # 2. the log density of the new points: the bytes of predict_logpdf, and the difference of the two log likelihoods
    assert logp == want_logp
    fresh = _fitted(c, mean, dtype, data=("Xc", "yc"))
    ll_fresh = fresh.loglik(th)[0]
    ll_bar = 1e-8 * abs(ll_fresh) if dtype == 64 else 1e-3 * max(abs(ll_fresh), n + m)     # (fp32: the bar of tests/test_gpu_parity.py)
    print(f"logp {logp:.12g}, loglik(fresh) - loglik(parent) {ll_fresh - ll_parent:.12g}: {abs(ll_fresh - ll_parent - logp):.2e} (bar {ll_bar:.1e})")
    assert abs(ll_fresh - ll_parent - logp) <= ll_bar
    # 5. the parent is untouched; a second call gives the same bytes
    after = h.predict(Xs)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    ext2, logp2, info2 = h.extend(c["Xn"], c["yn"])
    assert info2 == 0 and logp2 == logp
    # 1. + 4. both handles against numpy at the same bars
    assert fresh.fit(th) == 0
    got = _meets_the_bars(ext, c, dtype, "extended")
    ref = _meets_the_bars(fresh, c, dtype, "fresh   ")
    diffs = {"mean": np.abs(got["predict"][0] - ref["predict"][0]).max(), "var": np.abs(got["predict"][1] - ref["predict"][1]).max(),
             "cov": np.abs(got["cov"] - ref["cov"]).max(), "solve": np.abs(got["solve"] - ref["solve"]).max(),
             "logdet": abs(got["logdet"] - ref["logdet"])}
    print("extended - fresh: " + " ".join(f"{k} {v:.2e}" for k, v in diffs.items()))
    assert np.array_equal(ext2.predict(Xs)[0], got["predict"][0]) and np.array_equal(ext2.predict(Xs)[1], got["predict"][1])
    assert np.array_equal(ext2.solve(c["b"]), got["solve"]) and ext2.logdet() == got["logdet"]
    ext2.close()
    # closing the parent first leaves the extended handle working
    h.close()
    again = ext.predict(Xs)
    assert np.array_equal(again[0], got["predict"][0]) and np.array_equal(again[1], got["predict"][1])
    # 3. whatever rebuilds K returns the fresh handle's bytes
    th2 = th * 1.1
    assert ext.loglik(th2) == fresh.loglik(th2)
    ge, gf = ext.loglik_grad(th2), fresh.loglik_grad(th2)
    assert ge[0] == gf[0] and ge[2] == gf[2] == 0 and np.array_equal(ge[1], gf[1])
    assert np.array_equal(ext.covariance(th2), fresh.covariance(th2))
    assert ext.fit(th) == 0 and fresh.fit(th) == 0
    pe, pf = ext.predict(Xs), fresh.predict(Xs)
    assert np.array_equal(pe[0], pf[0]) and np.array_equal(pe[1], pf[1])
    ext.close()
    fresh.close()


def test_chain_of_single_point_extensions():
    n, m = er.CHAIN
    c = _case("se_ard", 3, "zero", n, m)
    th, Xs = c["theta"], c["Xs"]
    h = _fitted(c, "zero", 64)
    assert h.fit(th) == 0
    once, logp_once, info = h.extend(c["Xn"], c["yn"])
    assert info == 0
    cur, logp, made = h, 0.0, []
    for i in range(m):
        cur, lp, info = cur.extend(c["Xn"][i:i + 1], c["yn"][i:i + 1])
        assert info == 0 and cur.N == n + i + 1
        made.append(cur)
        logp += lp
    a = _meets_the_bars(cur, c, 64, "chain   ")
    b = _meets_the_bars(once, c, 64, "M = 3   ")
    fresh = _fitted(c, "zero", 64, data=("Xc", "yc"))
    assert fresh.fit(th) == 0
    f = _meets_the_bars(fresh, c, 64, "fresh   ")
    for other in (b, f):
        for k in ("cov", "solve"):
            assert np.abs(a[k] - other[k]).max() <= BAR[64]
        assert np.abs(a["predict"][0] - other["predict"][0]).max() <= BAR[64] and np.abs(a["predict"][1] - other["predict"][1]).max() <= BAR[64]
        assert abs(a["logdet"] - other["logdet"]) <= BAR[64]
    assert abs(logp - logp_once) <= 1e-8 * abs(logp_once)
    th2 = th * 1.1
    assert cur.loglik(th2) == fresh.loglik(th2)
    for x in made + [once, fresh, h]:
        x.close()


def test_extension_past_the_single_launch_range():
    """(12200, 200): the parent's factor comes from the single dataflow launch (96 tile columns), the extended size (97) is past
    dataflow_max_nt.  Against a fresh device handle only, at the bar tests/test_gpu_predict_joint.py uses above N = 4096; the
    solve and log det relative to their size (the bar is stated for quantities of order 1)."""
    n, m, d = 12200, 200, 3
    X, y, Xn, yn, Xs = er.case_data(n, m, d, m_test=130)
    th = er.theta_of("se_ard", d)
    h = _lib.Handle(X, y, "se_ard", "zero")
    assert h.fit(th) == 0 and h.get_option("dataflow_max_nt") == 96
    ext, logp, info = h.extend(Xn, yn)
    assert info == 0 and logp == h.predict_logpdf(Xn, yn)[0]
    h.close()
    fresh = _lib.Handle(np.vstack([X, Xn]), np.concatenate([y, yn]), "se_ard", "zero")
    assert fresh.fit(th) == 0
    b = syn.make_outputs(np.vstack([X, Xn]), row0=5)
    res = []
    for g in (ext, fresh):
        res.append((g.predict(Xs), g.predict_cov(Xs)[1], g.solve(b), g.logdet(), g.predict_grad(Xs)))
    (pe, ce, xe, le, ge), (pf, cf, xf, lf, gf) = res
    errs = {"mean": np.abs(pe[0] - pf[0]).max(), "var": np.abs(pe[1] - pf[1]).max(), "cov": np.abs(ce - cf).max(),
            "solve": _rel(xe, xf), "logdet": abs(le - lf) / abs(lf), "dmean": _rel(ge[2], gf[2]), "dvar": _rel(ge[3], gf[3])}
    print("extended - fresh at (12200, 200): " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= BAR_LARGE, (k, v)
    th2 = th * 1.1
    assert ext.loglik(th2) == fresh.loglik(th2)
    ext.close()
    fresh.close()


def test_refusals():
    c = _case("se_ard", 3, "zero", 300, 1)
    th = c["theta"]
    h = _fitted(c, "zero", 64)
    with pytest.raises(_lib.GphipError) as e:
        h.extend(c["Xn"], c["yn"])
    assert e.value.status == 4                                    # no fit
    assert h.fit(th) == 0
    before = h.predict(c["Xs"])
    ext, logp, info = h.extend(c["Xn"], np.array([np.inf]))
    assert ext is None and info == _lib.INFO_NAN and np.isnan(logp)
    with pytest.raises(_lib.GphipError) as e:
        h.extend(np.zeros((0, 3)), np.zeros(0))
    assert e.value.status == 2
    out, lp, inf = ctypes.c_void_p(), ctypes.c_double(0.0), ctypes.c_int(0)         # M = 0 and M above the limit at the C ABI
    dp = ctypes.POINTER(ctypes.c_double)
    for M in (0, 16385):
        assert h._lib.gphip_extend(h._h, c["Xn"].ctypes.data, c["yn"].ctypes.data_as(dp), M, ctypes.byref(out), ctypes.byref(lp), ctypes.byref(inf)) == 2
        assert not out.value
    assert gp.extendGaussianProcess(h, (c["Xn"], np.array([np.nan]))) is None
    good = gp.extendGaussianProcess(h, (c["Xn"], c["yn"]))
    assert good is not None and good.N == 301
    good.close()
    after = h.predict(c["Xs"])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert h.fit_pw(th, nugget_train=np.full(300, 0.02)) == 0
    with pytest.raises(_lib.GphipError) as e:
        h.extend(c["Xn"], c["yn"])
    assert e.value.status == 6                                    # a fit with a point-dependent array
    h.close()
    # Sigma under the pivot rule: the same far-away point twice at sn = 1e-9 (tests/test_extend.py: second pivot 0 <= 1.4e-14)
    kernel, mean, th, X, y, Xn, yn = er.refusal_case()
    h = _lib.Handle(X, y, kernel, mean)
    assert h.fit(th) == 0
    ext, logp, info = h.extend(Xn, yn)
    assert ext is None and info == _lib.INFO_NOT_SPD and np.isnan(logp)
    one, _, info = h.extend(Xn[:1], yn[:1])
    assert info == 0 and one is not None
    one.close()
    assert h.predict(Xn[:1])[1][0] > 0.5                          # the parent keeps its fit
    h.close()
    fresh = _lib.Handle(np.vstack([X, Xn]), np.concatenate([y, yn]), kernel, mean)
    assert fresh.fit(th) == _lib.INFO_NOT_SPD
    fresh.close()


def test_null_kernel_on_the_host():
    X, y, Xn, yn, Xs = er.case_data(50, 3, 2)
    th = np.array([0.3, 0.2])
    h = _lib.Handle(X, y, "null", "const")
    assert h.fit(th) == 0
    ext, logp, info = h.extend(Xn, yn)
    assert info == 0 and logp == h.predict_logpdf(Xn, yn)[0] and ext.N == 53
    fresh = _lib.Handle(np.vstack([X, Xn]), np.concatenate([y, yn]), "null", "const")
    assert fresh.fit(th) == 0
    assert ext.logdet() == fresh.logdet()
    for a, b in zip(ext.predict(Xs), fresh.predict(Xs)):
        assert np.array_equal(a, b)
    assert ext.loglik(th) == fresh.loglik(th)
    for g in (h, ext, fresh):
        g.close()


def test_no_leaks():
    import torch
    c = _case("se_ard", 3, "zero", 300, 1)
    h = _fitted(c, "zero", 64)
    assert h.fit(c["theta"]) == 0
    h.extend(c["Xn"], c["yn"])[0].close()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(20):
        ext, _, info = h.extend(c["Xn"], c["yn"])
        assert info == 0
        ext.predict(c["Xs"])
        ext.close()
    free1, _ = torch.cuda.mem_get_info()
    assert abs(free1 - free0) <= 8 << 20, (free0, free1)
    h.close()
