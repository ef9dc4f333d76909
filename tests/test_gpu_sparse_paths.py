"""gphip_sparse_paths_create on the device -- pathwise draws of the latent posterior function of the sparse object -- against the
numpy reference of tests/sparse_paths_reference.py evaluated on the table and the draw read back from the object
(gphip_paths_get, gphip_sparse_paths_get), so that the comparison is deterministic.  fp64 bar: the project's parity bar, 1e-8
of max |reference|, on the function values and gradients.  v itself is printed, not held to the bar: it is determined up to
cond(K_uu) x 1e-16 only, and k(x, Z) damps exactly those directions.

Shapes (sparse_paths_reference.CASES): N = 300, F = 64 (the sum's Ftot = 129 is ragged against a slab of 32 features), M = 77
test points (two 64-point tiles, the second ragged); m = 70 (m_pad = 128, ragged) with S = 5, m = 130 with S = 130 (two 128-tiles
on both indices), d = 9 (the DW = 16 register form).  Measured errors: DESIGN.md section 8o."""
import ctypes as C

import numpy as np
import pytest

import paths_reference as pr
import sparse_paths_reference as spr
from bayesianinference_amd import _lib, gaussian_process as gp, synthetic as syn

pytestmark = pytest.mark.gpu

BAR = 1e-8
PHILOX_BAR = 1e-13                    # tests/test_gpu_paths.py: a unit normal of the library against numpy's
SEED = 5
IDS = [c[0] for c in spr.CASES]
SE_ARD_BODY = "T s = 0; for (int k = 0; k < D; ++k) { const T u = (X(k) - Y(k)) / P(k); s += u * u; } return P(D) * P(D) * exp((T)-0.5 * s);"
_made = {}


def _err(g, want):
    return float(np.abs(g - want).max() / np.abs(want).max())


def _fitted(case, dtype=64, opts=None):
    """(handle fitted at the case's theta with the default jitter, theta, jitter)"""
    _, m, _, d, kernel, mean, ell = case
    X, y, Z, _ = spr.case_data(m, d)
    h = _lib.SparseHandle(X, y, Z, kernel, mean, dtype=dtype)
    for k, v in (opts or {}).items():
        h.set_option(k, v)
    th = spr.theta_of(kernel, d, mean, ell)
    assert h.fit(th) == 0
    return h, th, h.get_option("last_jitter")


def _own_points(Xs, S, M=3):
    """[S, M, d]: draw s at the test points (3 s + t) mod len(Xs), and those indices"""
    idx = (M * np.arange(S)[:, None] + np.arange(M)[None, :]) % len(Xs)
    return Xs[idx], idx


def _device(case):
    """the object's table, draw, v, out, dout and the values at every draw's own points; computed once and left unchanged"""
    if case[0] not in _made:
        _, m, S, d, kernel, mean, _ = case
        Xs = spr.case_data(m, d)[3]
        h, th, jit = _fitted(case)
        with h.sample_paths(S, spr.F, SEED) as p:
            t = p.table()
            out, dout = p.eval(Xs, grad=True)
            own, down = p.eval_own(_own_points(Xs, S)[0], grad=True)
            shape = (p.S, p.Ftot, p.N, p.d)
        h.close()
        t.update({"out": out, "dout": dout, "own": own, "down": down, "shape": shape, "theta": th, "jitter": jit})
        for v in t.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _made[case[0]] = t
    return _made[case[0]]


def _reference(case, t, Xs=None):
    _, m, _, d, kernel, mean, _ = case
    X, y, Z, P = spr.case_data(m, d)
    table = {"omega": t["omega"], "phase": t["phase"], "amp": _lib.rff_table(kernel, d, t["theta"], spr.F, SEED)[2]}
    return spr.paths(kernel, t["theta"], X, y, Z, t["jitter"], P if Xs is None else Xs, table, t["w"], t["xi"], t["zeta"], mean)


def _ftot(kernel):
    return (2 * spr.F if "+rq" in kernel else spr.F) + (1 if kernel.endswith("+const") else 0)


@pytest.mark.parametrize("case", spr.CASES, ids=IDS)
def test_draws_match_the_reference(case):
    _, m, S, d, kernel, mean, _ = case
    Xs = spr.case_data(m, d)[3]
    t = _device(case)
    assert t["shape"] == (S, _ftot(kernel), m, d)                 # N reads m
    om, ph, _ = _lib.rff_table(kernel, d, t["theta"], spr.F, SEED)
    assert t["omega"].tobytes() == om.tobytes() and t["phase"].tobytes() == ph.tobytes()      # the table of the fitted theta, byte for byte
    # the documented streams against numpy's own Philox4x32-10: w under the seed, xi and zeta under the keys of tags 10 and 11
    ws = pr.philox_normal(SEED, np.arange(S)[:, None], np.arange(_ftot(kernel))[None, :])
    xs, zs = spr.philox_streams(SEED, S, m)
    assert np.abs(t["w"] - ws).max() <= PHILOX_BAR
    assert np.abs(t["xi"] - xs).max() <= PHILOX_BAR and np.abs(t["zeta"] - zs).max() <= PHILOX_BAR
    assert np.abs(t["eps"] - np.sqrt(t["jitter"]) * t["zeta"]).max() <= 4e-16 * np.sqrt(t["jitter"]) * np.abs(t["zeta"]).max()
    r = _reference(case, t)
    ev, eo, ed = _err(t["v"], r["v"]), _err(t["out"], r["out"]), _err(t["dout"], r["dout"])
    idx = _own_points(Xs, S)[1]
    rows = np.arange(S)[:, None]
    eow, edw = _err(t["own"], r["out"][rows, idx]), _err(t["down"], r["dout"][rows, idx])
    print(f"{case[0]}: out {eo:.3e} dout {ed:.3e} own {eow:.3e} own dout {edw:.3e} of max |reference|; v {ev:.3e} (not held)")
    assert eo <= BAR and ed <= BAR and eow <= BAR and edw <= BAR


def test_ill_conditioned_inducing_matrix():
    """l = (3, 4, 5) on data in [-1, 1]^3: cond(K_uu) = 6.5e11 at m = 70 with the default jitter, where the float64 reference
    itself is off by 5e-9 of max |f| against its evaluation in 40-digit arithmetic (sparse_paths_reference.paths_mp).  The bar is
    10 x that error, computed here; the device's error is measured against the extended-precision values."""
    case = ("ill", 70, 3, 3, "se_ard", "const", spr.ELL_ILL)
    _, m, S, d, kernel, mean, _ = case
    X, y, Z, Xs = spr.case_data(m, d)
    Xs = Xs[:10]
    h, th, jit = _fitted(case)
    with h.sample_paths(S, spr.F, SEED) as p:
        t = p.table()
        out = p.eval(Xs)
        own = p.eval_own(_own_points(Xs, S)[0])
    h.close()
    t.update({"theta": th, "jitter": jit})
    table = {"omega": t["omega"], "phase": t["phase"], "amp": _lib.rff_table(kernel, d, th, spr.F, SEED)[2]}
    r = _reference(case, t, Xs)
    e = spr.paths_mp(kernel, th, X, y, Z, jit, Xs, table, t["w"], t["xi"], t["zeta"], mean)
    own_err = _err(r["out"], e["out"])
    idx = _own_points(Xs, S)[1]
    dev, dev_own = _err(out, e["out"]), _err(own, e["out"][np.arange(S)[:, None], idx])
    print(f"ill-conditioned: float64 reference {own_err:.3e}, device eval {dev:.3e}, eval_own {dev_own:.3e}, bar {10 * own_err:.3e}; "
          f"v: reference {_err(r['v'], e['v']):.3e}, device {_err(t['v'], e['v']):.3e}, max |v| {np.abs(e['v']).max():.2e}")
    assert dev <= 10 * own_err and dev_own <= 10 * own_err


def test_prefix_property_determinism_and_independence_of_the_fit():
    case = spr.CASES[1]                                           # se_ard, constant mean
    _, m, S, d, kernel, mean, _ = case
    X, y, Z, Xs = spr.case_data(m, d)
    t = _device(case)
    h, th, jit = _fitted(case)
    pm, pv = h.predict(Xs)
    F0, _ = h.bound(th)                                           # (the fit stays resident)
    p3 = h.sample_paths(3, spr.F, SEED)
    p3b = h.sample_paths(3, spr.F, SEED)
    pm2, pv2 = h.predict(Xs)
    assert pm.tobytes() == pm2.tobytes() and pv.tobytes() == pv2.tobytes()        # the fit is untouched
    t3, t3b = p3.table(), p3b.table()
    for k in t3:                                                  # two creations: the same bytes
        assert t3[k].tobytes() == t3b[k].tobytes(), k
    p3b.close()
    for k in ("w", "xi", "zeta", "eps"):                          # the prefix property in S
        assert t3[k].tobytes() == t[k][:3].tobytes(), k
    assert t3["omega"].tobytes() == t["omega"].tobytes() and t3["phase"].tobytes() == t["phase"].tobytes()
    o3, d3 = p3.eval(Xs, grad=True)
    assert _err(o3, t["out"][:3]) <= 1e-10
    assert p3.eval(Xs).tobytes() == o3.tobytes()                  # out does not depend on dout being asked for
    o3b, d3b = p3.eval(Xs, grad=True)
    assert o3.tobytes() == o3b.tobytes() and d3.tobytes() == d3b.tobytes()        # two evaluations: the same bytes
    P = _own_points(Xs, 3)[0]
    w1, g1 = p3.eval_own(P, grad=True)
    w2, g2 = p3.eval_own(P, grad=True)
    assert w1.tobytes() == w2.tobytes() and g1.tobytes() == g2.tobytes() and p3.eval_own(P).tobytes() == w1.tobytes()
    # forced strips and chunks, through the sparse object's options
    h.set_option("paths_split", 3)
    h.set_option("paths_chunk", 64)
    os_, ds_ = p3.eval(Xs, grad=True)
    assert h.get_option("last_paths_nsplit") == 3
    ws_, gs_ = p3.eval_own(P, grad=True)
    with h.sample_paths(3, spr.F, SEED) as ps:                    # strips of the create call's feature pass
        assert _err(ps.eval(Xs), o3) <= 1e-10
    h.set_option("paths_split", 0)
    h.set_option("paths_chunk", 0)
    assert _err(os_, o3) <= 1e-10 and _err(ds_, d3) <= 1e-10 and _err(ws_, w1) <= 1e-10 and _err(gs_, g1) <= 1e-10
    assert h.get_option("last_paths_create_us") > 0 and h.get_option("last_paths_eval_us") > 0
    assert h.get_option("last_paths_feature_us") > 0 and h.get_option("last_paths_subst_us") > 0
    pm3, pv3 = h.predict(Xs)
    F1, _ = h.bound(th)
    assert pm.tobytes() == pm3.tobytes() and pv.tobytes() == pv3.tobytes() and F0 == F1
    # a refit at another theta and new inducing points of the same number: the object still evaluates the same bytes
    other = th.copy()
    other[:3] *= 1.7
    assert h.fit(other) == 0
    assert p3.eval(Xs).tobytes() == o3.tobytes()
    h.set_inducing(Z[::-1] * 0.9)
    assert p3.eval(Xs).tobytes() == o3.tobytes() and p3.eval_own(P).tobytes() == w1.tobytes()
    assert p3.table()["v"].tobytes() == t3["v"].tobytes()
    # the parent cannot be destroyed, or given another number of inducing points, under a live object
    lib = _lib.load()
    with pytest.raises(_lib.GphipError) as e:
        h.close()
    assert e.value.status == 4 and "paths" in str(e.value)
    with pytest.raises(_lib.GphipError) as e:
        h.set_inducing(Z[:50])
    assert e.value.status == 4 and h.m == m
    assert h.fit(th) == 0 and np.all(np.isfinite(h.predict(Xs)[0]))               # .. and is still alive
    assert lib.gphip_sparse_paths_get(p3._q, None, None) == 0
    p3.close()
    h.set_inducing(Z[:50])
    assert h.m == 50 and h.fit(th) == 0
    h.close()
    assert h._h is None


def test_statuses():
    case = spr.CASES[0]
    _, m, S, d, kernel, mean, _ = case
    X, y, Z, Xs = spr.case_data(m, d)
    th = spr.theta_of(kernel, d, mean)
    lib = _lib.load()
    h = _lib.SparseHandle(X, y, Z, kernel, mean)
    q, info = C.c_void_p(), C.c_int(0)
    create = lambda hh, s, f: lib.gphip_sparse_paths_create(hh, s, f, 0, C.byref(q), C.byref(info))      # noqa: E731
    assert create(h._h, S, spr.F) == 4 and not q.value            # no fit
    assert "before a successful" in (lib.gphip_sparse_last_error(h._h) or b"").decode()
    assert h.fit(th) == 0
    assert create(None, S, spr.F) == 1
    assert lib.gphip_sparse_paths_create(h._h, S, spr.F, 0, None, C.byref(info)) == 1
    assert lib.gphip_sparse_paths_create(h._h, S, spr.F, 0, C.byref(q), None) == 1
    for s, f in ((0, spr.F), (S, 0), (2049, spr.F), (2048, 40000)):
        assert create(h._h, s, f) == 2 and not q.value, (s, f)
    # no resident fit after a batch, a prediction over samples and new inducing points
    for drop in (lambda: h.bound_batch(np.vstack([th, th])), lambda: h.predict_samples(np.vstack([th, th]), Xs[:3]),
                 lambda: h.set_inducing(Z)):
        assert h.fit(th) == 0
        assert create(h._h, S, spr.F) == 0 and q.value
        assert lib.gphip_paths_destroy(q) == 0
        drop()
        assert create(h._h, S, spr.F) == 4 and not q.value
    # calls on the object: their statuses, and the error text through the sparse object
    assert h.fit(th) == 0
    with h.sample_paths(2, 8, 0) as p:
        out = np.zeros((2, 1))
        assert lib.gphip_paths_eval(p._q, None, 1, _lib._d(out), None) == 1
        assert "null argument" in (lib.gphip_sparse_last_error(h._h) or b"").decode()
        assert lib.gphip_paths_eval(p._q, Xs.ctypes.data, 0, _lib._d(out), None) == 2
        assert "M < 1" in (lib.gphip_sparse_last_error(h._h) or b"").decode()
        assert lib.gphip_paths_eval_own(p._q, Xs.ctypes.data, 0, _lib._d(out), None) == 2
        with pytest.raises(_lib.GphipError) as e:
            p.eval(np.zeros((0, d)))
        assert e.value.status == 2 and "M < 1" in str(e.value)
    # a fit made with a point-dependent array; without one the _pw call is the constant call
    assert h.fit_pw(th, nugget_train=np.full(len(X), spr.SN ** 2)) == 0
    assert create(h._h, S, spr.F) == 6 and not q.value
    assert h.fit_pw(th) == 0
    assert create(h._h, S, spr.F) == 0 and q.value
    assert lib.gphip_paths_destroy(q) == 0
    h.close()
    custom = _lib.SparseHandle(X, y, Z, _lib.CustomKernel(SE_ARD_BODY, d + 1), mean)
    assert custom.fit(th) == 0
    assert create(custom._h, S, spr.F) == 6 and not q.value
    custom.close()
    # gphip_sparse_paths_get on an exact object's handle
    e = _lib.Handle(X, y, kernel, mean)
    assert e.fit(th) == 0
    with e.sample_paths(2, 8, 0) as p:
        assert lib.gphip_sparse_paths_get(p._q, None, None) == 1
        assert set(p.table()) == {"omega", "phase", "w", "eps", "v"}
    e.close()


def test_sample_moments_follow_the_linear_gaussian_law():
    """S = 2048 draws at 6 points against the closed-form law over (w, xi, zeta) for the read-back table.  Monte-Carlo error only:
    5 sigma of a mean of S draws, 5 sqrt(2 / S) max C_ii for a covariance entry (the thresholds of tests/test_gpu_paths.py)."""
    n, m, s, f, d = 300, 40, 2048, 64, 2
    X, y, Z, Xs = spr.case_data(m, d, n=n, m_test=6)
    th = np.array([0.5, 0.7, 1.1, 0.15, 0.2])
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const")
    assert h.fit(th, 1e-6) == 0                                  # (a jitter large enough for its term to count)
    jit = h.get_option("last_jitter")
    with h.sample_paths(s, f, 123) as p:
        t = p.table()
        out = p.eval(Xs)
    h.close()
    table = {"omega": t["omega"], "phase": t["phase"], "amp": _lib.rff_table("se_ard", d, th, f, 123)[2]}
    mo = spr.moments("se_ard", th, X, y, Z, jit, Xs, table, "const")
    cmax = np.max(np.diag(mo["cov"]))
    em = np.abs(out.mean(axis=0) - mo["mean"]).max()
    ec = np.abs(np.cov(out.T) - mo["cov"]).max()
    print(f"sample mean off by {em:.3e} (bar {5 * np.sqrt(cmax / s):.3e}), covariance by {ec:.3e} (bar {5 * np.sqrt(2.0 / s) * cmax:.3e})")
    assert em <= 5.0 * np.sqrt(cmax / s) and ec <= 5.0 * np.sqrt(2.0 / s) * cmax


# fp32 object against the fp64 reference at N = 2000, d = 3, m = 300, default fp32 jitter (1e-4 k(x, x)), 77 test points: the case
# of the other sparse fp32 tests, 20 draws.  Measured on an MI355X, of max |reference|: eval 3.28e-3, its
# gradient 5.62e-3, eval_own (fp64 accumulation of the same fp32 v) 1.59e-3; the bars are 4 x those, the convention of section 8c.
# cond(K_uu) is bounded by m sf^2 / jitter = 3e6 here, times the fp32 unit roundoff 6e-8 on v; k(x, Z) damps what reaches f.
FP32_OUT, FP32_DOUT, FP32_OWN = 3.28e-3, 5.62e-3, 1.59e-3


def test_fp32_object_against_the_fp64_reference():
    X, y = syn.make_dataset(2000, 3)
    Z = gp.selectInducingPoints(X, 300, seed=1)
    Xs = syn.make_test_points(77, 3)
    th = np.array([0.8, 1.05, 1.3, spr.SF, spr.SN, spr.MU])
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const", dtype=32)
    assert h.fit(th) == 0
    jit = h.get_option("last_jitter")
    assert jit == pytest.approx(1e-4 * spr.SF ** 2, rel=1e-12)
    with h.sample_paths(20, spr.F, SEED) as p:
        t = p.table()
        out, dout = p.eval(Xs, grad=True)
        own = p.eval_own(_own_points(Xs, 20)[0])
    h.close()
    table = {"omega": t["omega"], "phase": t["phase"], "amp": _lib.rff_table("se_ard", 3, th, spr.F, SEED)[2]}
    r = spr.paths("se_ard", th, X, y, Z, jit, Xs, table, t["w"], t["xi"], t["zeta"], "const")
    idx = _own_points(Xs, 20)[1]
    eo, ed, ew = _err(out, r["out"]), _err(dout, r["dout"]), _err(own, r["out"][np.arange(20)[:, None], idx])
    print(f"fp32 (jitter {jit:.3e}): out {eo:.3e} dout {ed:.3e} own {ew:.3e} of max |reference|")
    assert eo <= 4 * FP32_OUT and ew <= 4 * FP32_OWN and ed <= 4 * FP32_DOUT


def test_python_layer():
    n, d, m = 300, 1, 30
    X, y = syn.make_dataset(n, d)
    th = np.array([0.3, 1.1, 0.15])
    obj = gp.defineSparseGaussianProcess((X, y[:, None]), "se", m, variables=[("l", 0.05, 2.0), ("sf", 0.1, 5.0), ("sn", 0.01, 1.0)], Jitter=1e-8)
    assert not obj.failed
    handle = obj["SparseGaussianProcessData"]["HIPHandle"]
    pts = np.linspace(-0.9, 0.9, 25)
    assert gp.samplePathsFromSparseGaussianProcess(obj, 5) is None                # unsampled and no theta
    assert gp.samplePathsFromSparseGaussianProcess(obj, 0, th) is None
    assert gp.samplePathsFromGaussianProcess(obj, 5) is None and gp.samplePathsFromSparseGaussianProcess({"a": 1}, 5, th) is None
    # one theta: one fit, one paths object; gradients against central differences
    with gp.samplePathsFromSparseGaussianProcess(obj, 6, th, Features=64, seed=3) as f:
        vals, grads = f(pts), f.gradient(pts)
        assert vals.shape == (6, 25) and grads.shape == (6, 25, 1) and len(f._parts) == 1 and np.all(f.sample == 0)
        assert f(pts).tobytes() == vals.tobytes()                 # coherent across calls
        fd = (f(pts + 1e-5) - f(pts - 1e-5)) / 2e-5
        assert np.abs(fd - grads[:, :, 0]).max() <= 1e-6 * np.abs(grads).max()
        own = f.own(np.broadcast_to(pts[None, :3, None], (6, 3, 1)).copy())
        assert np.abs(own - vals[:, :3]).max() <= 1e-10 * np.abs(vals).max()
        # the draws scatter around the sparse predictive mean
        mean = gp.predictFromSparseGaussianProcess(obj, pts, th)["Mean"][0]
        assert np.abs(vals - mean).max() <= 1.0
    # a posterior of two samples: the draws are split over the samples by weight, one paths object per theta used
    sampled = obj.append({"Samples": [{"Point": th, "CrudePosteriorWeight": 0.6},
                                      {"Point": np.array([0.5, 0.9, 0.2]), "CrudePosteriorWeight": 0.4}]})
    with gp.samplePathsFromSparseGaussianProcess(sampled, 40, Features=64, seed=1) as f:
        vals, grads = f(pts), f.gradient(pts)
        assert vals.shape == (40, 25) and grads.shape == (40, 25, 1) and np.all(np.isfinite(vals))
        assert set(np.unique(f.sample)) == {0, 1} and len(f._parts) == 2
        which = np.random.default_rng(1).choice(2, size=40, p=np.array([0.6, 0.4]))
        assert np.array_equal(f.sample, which)                    # the assignment of samplePathsFromGaussianProcess
        fd = (f(pts + 1e-5) - f(pts - 1e-5)) / 2e-5
        assert np.abs(fd - grads[:, :, 0]).max() <= 1e-6 * np.abs(grads).max()
        # the per-theta keys of samplePathsFromGaussianProcess: the rows of sample 0 are the draws of one object under its key
        rows = np.flatnonzero(which == 0)
        assert handle.fit(th, obj["Jitter"]) == 0
        key = int(np.random.SeedSequence([1, 0]).generate_state(1, np.uint64)[0])
        with handle.sample_paths(len(rows), 64, key) as p:
            assert _err(p.eval(pts[:, None]), vals[rows]) <= 1e-10
    # Thompson sampling in d = 1: per draw a value at least the draw's best candidate, and the value `own` returns at the reported x
    box = np.array([[-0.95, 0.95]])
    res = gp.thompsonSampleFromSparseGaussianProcess(obj, 8, box, th, Features=64, seed=2, candidates=64, starts=3, iterations=25)
    assert res["x"].shape == (8, 1) and res["f"].shape == (8,) and np.all(res["sample"] == 0)
    assert np.all(res["x"] >= box[0, 0]) and np.all(res["x"] <= box[0, 1])
    cand = box[0, 0] + (box[0, 1] - box[0, 0]) * np.random.default_rng(2).random((64, 1))
    with gp.samplePathsFromSparseGaussianProcess(obj, 8, th, Features=64, seed=2) as f:
        best = f(cand).max(axis=1)
        at_x = f.own(res["x"][:, None, :])[:, 0]
    print("thompson:", np.c_[res["x"][:, 0], res["f"], best])
    assert np.all(res["f"] >= best)
    assert np.abs(at_x - res["f"]).max() <= 1e-12 * np.abs(res["f"]).max()
    res2 = gp.thompsonSampleFromSparseGaussianProcess(sampled, 8, box, Features=64, seed=2, candidates=64, starts=2, iterations=10)
    assert res2["x"].shape == (8, 1) and np.all(np.isfinite(res2["f"])) and set(np.unique(res2["sample"])) <= {0, 1}
    assert gp.thompsonSampleFromSparseGaussianProcess(obj, 8, box) is None
    handle.close()
