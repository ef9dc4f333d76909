"""gphip_paths_create / gphip_paths_eval on the device -- pathwise draws of the latent posterior function -- against the numpy
reference of tests/paths_reference.py evaluated on the table and the draw read back from the object (gphip_paths_get), so that
the comparison is deterministic: the fp64 bar is the project's parity bar, 1e-8 of max |reference|.

Shapes: the cases of predict_grad_reference.CASES (N = 300: Npad = 384 with a ragged tile; M = 130: three 64-point tiles, the last
ragged), S = 20 (ragged against the 16 draws of an MFMA block), F = 100 (ragged against a slab of 32 features; the two-term
cases give Ftot = 200 / 100 / 101).  d = 20 keeps its coordinates in registers and LDS; d = 40 (> KB_LDS_MAXD) takes the
global-memory form.  Errors measured on an MI355X are in DESIGN.md section 8m."""
import ctypes as C

import numpy as np
import pytest

import paths_reference as pr
from bayesianinference_amd import _lib, gaussian_process as gp, synthetic as syn

pytestmark = pytest.mark.gpu

BAR = 1e-8
# a unit normal of the library against numpy's: the same 53-bit uniforms, then log, sqrt, the product 2 pi u and cos, each within a
# few ulp in both: ~10 x 2^-53 of a value of at most sqrt(2 x 53 log 2) = 8.6, plus the rounding of the angle (2 pi x 2^-53) times
# that radius -- below 2e-14.  1e-13 absolute; two different streams differ by O(1).
PHILOX_BAR = 1e-13
S, F = 20, 100
IDS = [pr.case_id(c) for c in pr.CASES]
SE_ARD_BODY = "T s = 0; for (int k = 0; k < D; ++k) { const T u = (X(k) - Y(k)) / P(k); s += u * u; } return P(D) * P(D) * exp((T)-0.5 * s);"
_made = {}


def _err(g, want):
    return float(np.abs(g - want).max() / np.abs(want).max())


def _fitted(c, dtype=64, opts=None):
    h = _lib.Handle(c["X"], c["y"], c["kernel"], c["mean_kind"], dtype=dtype)
    for k, v in (opts or {}).items():
        h.set_option(k, v)
    assert h.fit(c["theta"]) == 0
    return h


def _ftot(name):
    return (2 * F if "+rq" in name else F) + (1 if name.endswith("+const") else 0)


def _device(case, dtype=64, s=S, f=F, seed=5):
    """the object's table, draw, v, out and dout of one case, computed once per process and left unchanged"""
    key = (case, dtype, s, f, seed)
    if key not in _made:
        c = pr.case_reference(*case)
        h = _fitted(c, dtype)
        with h.sample_paths(s, f, seed) as p:
            t = p.table()
            out, dout = p.eval(c["Xs"], grad=True)
            shape = (p.S, p.Ftot, p.N, p.d)
        h.close()
        t.update({"out": out, "dout": dout, "shape": shape})
        for v in t.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _made[key] = t
    return _made[key]


def _reference(case, t, dtype=np.float64):
    c = pr.case_reference(*case)
    name, d, mean = case
    table = {"omega": t["omega"], "phase": t["phase"], "amp": _lib.rff_table(name, d, c["theta"], F, 5)[2]}
    return pr.paths(name, c["theta"], c["X"], c["y"], c["Xs"], table, t["w"], t["eps"], mean, dtype=dtype)


@pytest.mark.parametrize("case", pr.CASES, ids=IDS)
def test_draws_match_the_reference(case):
    name, d, mean = case
    c = pr.case_reference(*case)
    t = _device(case)
    assert t["shape"] == (S, _ftot(name), len(c["X"]), d)
    om, ph, _ = _lib.rff_table(name, d, c["theta"], F, 5)
    assert t["omega"].tobytes() == om.tobytes() and t["phase"].tobytes() == ph.tobytes()      # the table of the fitted theta, byte for byte
    sn = abs(c["theta"][-2 if mean == "const" else -1])
    assert abs(t["eps"].std() / sn - 1.0) <= 0.05 and abs(t["w"].std() - 1.0) <= 0.1
    # the documented streams, against numpy's own Philox4x32-10: w under the seed, eps under the seed's key of tag 9
    n = len(c["X"])
    ws = pr.philox_normal(5, np.arange(S)[:, None], np.arange(_ftot(name))[None, :])
    es = pr.philox_normal(pr.rff_key(5, pr.TAG_EPS), np.arange(S)[:, None], np.arange(n)[None, :])
    assert np.abs(t["w"] - ws).max() <= PHILOX_BAR and np.abs(t["eps"] / sn - es).max() <= PHILOX_BAR
    # .. which is no stream of the table: the noise on the first d points of draw s is not direction s of the table's first term
    z = pr.philox_normal(pr.rff_key(5, pr.TAG_DIRECTION), np.arange(S)[:, None], np.arange(d)[None, :])
    assert np.abs(t["eps"][:, :d] / sn - z).min() > 1e-6
    if name in ("se", "se_ard"):                                  # SE: omega l is that direction itself
        ell = np.abs(c["theta"][:d]) if name == "se_ard" else abs(c["theta"][0])
        assert np.abs(t["omega"][:S] * ell - z).max() <= PHILOX_BAR
        assert np.abs(t["eps"][:, :d] / sn - t["omega"][:S] * ell).min() > 1e-6
    r = _reference(case, t)
    ev, eo, ed = _err(t["v"], r["v"]), _err(t["out"], r["out"]), _err(t["dout"], r["dout"])
    print(f"{name} d={d} {mean}: v {ev:.3e} out {eo:.3e} dout {ed:.3e} of max |reference|")
    assert ev <= BAR and eo <= BAR and ed <= BAR


@pytest.mark.parametrize("case", [pr.CASES[1], pr.CASES[5]], ids=[IDS[1], IDS[5]])
def test_fp32_handle(case):
    """The bar is 10 x the error of the numpy reference evaluated in float32 arithmetic against its float64 evaluation, on the
    same table and draw -- never measured against the device.  Measured on an MI355X: DESIGN.md section 8m."""
    name, d, mean = case
    t = _device(case, dtype=32)
    r64, r32 = _reference(case, t), _reference(case, t, np.float32)
    for k in ("v", "out", "dout"):
        base, dev = _err(r32[k].astype(np.float64), r64[k]), _err(t[k], r64[k])
        print(f"fp32 {name} d={d} {k}: device {dev:.3e}, numpy float32 {base:.3e}, bar {10 * base:.3e}")
        assert dev <= 10 * base, k


def test_one_draw_one_point_one_feature():
    case = pr.CASES[1]
    c = pr.case_reference(*case)
    name, d, mean = case
    h = _fitted(c)
    for s, f, m in ((1, F, len(c["Xs"])), (S, F, 1), (S, 1, len(c["Xs"])), (1, 1, 1)):
        with h.sample_paths(s, f, 9) as p:
            t = p.table()
            out, dout = p.eval(c["Xs"][:m], grad=True)
        assert out.shape == (s, m) and dout.shape == (s, m, d)
        table = {"omega": t["omega"], "phase": t["phase"], "amp": _lib.rff_table(name, d, c["theta"], f, 9)[2]}
        r = pr.paths(name, c["theta"], c["X"], c["y"], c["Xs"][:m], table, t["w"], t["eps"], mean)
        assert _err(t["v"], r["v"]) <= BAR and _err(out, r["out"]) <= BAR and _err(dout, r["dout"]) <= BAR, (s, f, m)
    h.close()


def test_more_dimensions_than_the_lds_window():
    d, n, m = 40, 100, 70
    X, y = syn.make_dataset(n, d)
    Xs = syn.make_test_points(m, d)
    th = np.array(list(np.linspace(5.0, 8.0, d)) + [1.1, 0.15, 0.2])
    h = _lib.Handle(X, y, "matern52_ard", "const")
    assert h.fit(th) == 0
    with h.sample_paths(5, 40, 2) as p:
        t = p.table()
        out, dout = p.eval(Xs, grad=True)
    h.close()
    table = {"omega": t["omega"], "phase": t["phase"], "amp": _lib.rff_table("matern52_ard", d, th, 40, 2)[2]}
    r = pr.paths("matern52_ard", th, X, y, Xs, table, t["w"], t["eps"], "const")
    print(f"d = 40: v {_err(t['v'], r['v']):.3e} out {_err(out, r['out']):.3e} dout {_err(dout, r['dout']):.3e}")
    assert _err(t["v"], r["v"]) <= BAR and _err(out, r["out"]) <= BAR and _err(dout, r["dout"]) <= BAR


def test_strips_chunks_and_the_gradient_flag():
    case = pr.CASES[5]                                            # product of two terms + constant
    c = pr.case_reference(*case)
    t = _device(case)
    r = _reference(case, t)
    h = _fitted(c)
    with h.sample_paths(S, F, 5) as p:
        base = p.eval(c["Xs"])
        assert base.tobytes() == p.eval(c["Xs"], grad=True)[0].tobytes()      # out does not depend on dout being asked for
        assert _err(base, t["out"]) <= 1e-10                      # (another handle's object of the same seed: v to rounding)
        for split in (1, 3):
            h.set_option("paths_split", split)
            o1, d1 = p.eval(c["Xs"], grad=True)
            o2, d2 = p.eval(c["Xs"], grad=True)
            assert h.get_option("last_paths_nsplit") == split
            assert o1.tobytes() == o2.tobytes() and d1.tobytes() == d2.tobytes()
            assert _err(o1, r["out"]) <= BAR and _err(d1, r["dout"]) <= BAR
            assert p.eval(c["Xs"]).tobytes() == o1.tobytes()
        h.set_option("paths_split", 0)
        h.set_option("paths_chunk", 128)                          # 130 points: a seam after 128
        oc, dc = p.eval(c["Xs"], grad=True)
        h.set_option("paths_chunk", 0)
        assert _err(oc, t["out"]) <= 1e-10 and _err(dc, t["dout"]) <= 1e-10
        assert h.get_option("last_paths_create_us") > 0 and h.get_option("last_paths_eval_us") > 0
    # strips of the create call's feature pass: the same v to rounding
    h.set_option("paths_split", 3)
    with h.sample_paths(S, F, 5) as p3:
        assert _err(p3.table()["v"], r["v"]) <= BAR
    h.close()


def test_prefix_property_and_independence_of_the_parent():
    case = pr.CASES[4]                                            # rq_ard
    c = pr.case_reference(*case)
    t = _device(case)
    h = _fitted(c)
    pm, pv = h.predict(c["Xs"])
    p8 = h.sample_paths(8, F, 5)
    pm2, pv2 = h.predict(c["Xs"])
    assert pm.tobytes() == pm2.tobytes() and pv.tobytes() == pv2.tobytes()        # the parent's fit is untouched
    t8 = p8.table()
    assert t8["w"].tobytes() == t["w"][:8].tobytes() and t8["eps"].tobytes() == t["eps"][:8].tobytes()
    assert t8["omega"].tobytes() == t["omega"].tobytes() and t8["phase"].tobytes() == t["phase"].tobytes()
    o8 = p8.eval(c["Xs"])
    assert _err(o8, t["out"][:8]) <= 1e-10
    # the parent fitted again at another theta: the object still evaluates the same bytes
    other = c["theta"].copy()
    other[:3] *= 1.7
    assert h.fit(other) == 0
    assert p8.eval(c["Xs"]).tobytes() == o8.tobytes()
    # the parent cannot be destroyed under a live object
    with pytest.raises(_lib.GphipError) as e:
        h.close()
    assert e.value.status == 4
    pm3, _ = h.predict(c["Xs"])                                   # .. and is still alive
    assert np.all(np.isfinite(pm3))
    p8.close()
    h.close()
    assert h._h is None


def test_statuses_and_the_null_kernel():
    case = pr.CASES[1]
    name, d, mean = case
    c = pr.case_reference(*case)
    lib = _lib.load()
    h = _lib.Handle(c["X"], c["y"], name, mean)
    q, info = C.c_void_p(), C.c_int(0)
    assert lib.gphip_paths_create(h._h, S, F, 0, C.byref(q), C.byref(info)) == 4 and not q.value        # no fit
    assert h.fit(c["theta"]) == 0
    assert lib.gphip_paths_create(None, S, F, 0, C.byref(q), C.byref(info)) == 1
    assert lib.gphip_paths_create(h._h, S, F, 0, None, C.byref(info)) == 1
    assert lib.gphip_paths_create(h._h, S, F, 0, C.byref(q), None) == 1
    for s, f in ((0, F), (S, 0), (2049, F), (2048, 40000)):
        assert lib.gphip_paths_create(h._h, s, f, 0, C.byref(q), C.byref(info)) == 2 and not q.value, (s, f)
    with h.sample_paths(2, 8, 0) as p:
        out = np.zeros((2, 1))
        assert lib.gphip_paths_eval(p._q, None, 1, _lib._d(out), None) == 1
        assert lib.gphip_paths_eval(p._q, c["Xs"].ctypes.data, 1, None, None) == 1
        assert lib.gphip_paths_eval(p._q, c["Xs"].ctypes.data, 0, _lib._d(out), None) == 2
        assert lib.gphip_paths_eval(None, c["Xs"].ctypes.data, 1, _lib._d(out), None) == 1
    assert h.fit_pw(c["theta"], nugget_train=np.full(len(c["X"]), 0.15 ** 2)) == 0
    assert lib.gphip_paths_create(h._h, S, F, 0, C.byref(q), C.byref(info)) == 6 and not q.value
    h.close()
    custom = _lib.Handle(c["X"], c["y"], _lib.CustomKernel(SE_ARD_BODY, d + 1), mean)
    assert custom.fit(c["theta"]) == 0
    assert lib.gphip_paths_create(custom._h, S, F, 0, C.byref(q), C.byref(info)) == 6 and not q.value
    custom.close()
    null = _lib.Handle(c["X"], c["y"], "null", "const")
    assert null.fit(np.array([0.3, 0.2])) == 0
    with null.sample_paths(3, 10, 0) as p:
        out, dout = p.eval(c["Xs"], grad=True)
        assert p.Ftot == 0
    null.close()
    assert np.all(out == 0.2) and np.all(dout == 0.0) and out.shape == (3, len(c["Xs"])) and dout.shape == (3, len(c["Xs"]), d)


def test_sharded_fit_is_refused_and_a_replicated_one_computes_on_the_first_device():
    Xg, yg = syn.make_dataset(1100, 2)
    Xs = syn.make_test_points(40, 2)
    th = np.array([0.9, 1.2, 1.1, 0.15, 0.2])
    one = _lib.Handle(Xg, yg, "se_ard", "const")
    assert one.fit(th) == 0
    with one.sample_paths(4, 32, 1) as p:
        want = p.eval(Xs)
    one.close()
    lib = _lib.load()
    for rep in (0, 1):
        g = _lib.Handle(Xg, yg, "se_ard", "const", device=[0, 0])
        g.set_option("shard_min_n", 0)
        g.set_option("panel", 2)
        g.set_option("replicate_factor", rep)
        assert g.fit(th) == 0
        if rep == 0:
            q, info = C.c_void_p(), C.c_int(0)
            assert lib.gphip_paths_create(g._h, 4, 32, 1, C.byref(q), C.byref(info)) == 6 and not q.value
        else:
            with g.sample_paths(4, 32, 1) as p:
                assert _err(p.eval(Xs), want) <= 1e-9
        g.close()


def test_sample_moments_follow_the_linear_gaussian_law():
    """N = 64, M = 8, S = 2048, F = 64: over s, the outputs are draws of N(m + G (y - m), A A^T + sn^2 B B^T) for the read-back
    table.  Monte-Carlo error only: 5 sigma of a mean of S draws, 5 sqrt(2 / S) max C_ii for a covariance entry; fixed seed."""
    n, m, s, f, d = 64, 8, 2048, 64, 2
    X, y = syn.make_dataset(n, d)
    Xs = syn.make_test_points(m, d)
    th = np.array([0.9, 1.2, 1.1, 0.15, 0.2])
    h = _lib.Handle(X, y, "se_ard", "const")
    assert h.fit(th) == 0
    with h.sample_paths(s, f, 123) as p:
        t = p.table()
        out = p.eval(Xs)
    h.close()
    table = {"omega": t["omega"], "phase": t["phase"], "amp": _lib.rff_table("se_ard", d, th, f, 123)[2]}
    mo = pr.moments("se_ard", th, X, y, Xs, table, "const")
    cmax = np.max(np.diag(mo["cov"]))
    em = np.abs(out.mean(axis=0) - mo["mean"]).max()
    ec = np.abs(np.cov(out.T) - mo["cov"]).max()
    print(f"sample mean off by {em:.3e} (bar {5 * np.sqrt(cmax / s):.3e}), covariance by {ec:.3e} (bar {5 * np.sqrt(2.0 / s) * cmax:.3e})")
    assert em <= 5.0 * np.sqrt(cmax / s) and ec <= 5.0 * np.sqrt(2.0 / s) * cmax


def test_python_layer():
    name, d, mean = pr.CASES[3]                                   # matern32, d = 2, constant mean
    c = pr.case_reference(name, d, mean)
    pts = c["Xs"][:30]
    with gp.samplePathsFromGaussianProcess((c["X"], c["y"][:, None]), 6, name, c["theta"], meanFunction="const", Features=64, seed=3) as f:
        vals, grads = f(pts), f.gradient(pts)
        assert vals.shape == (6, 30) and grads.shape == (6, 30, d)
        assert f(pts).tobytes() == vals.tobytes()                 # coherent across calls
        step = 1e-5
        for k in range(d):
            e = np.zeros(d)
            e[k] = step
            fd = (f(pts + e) - f(pts - e)) / (2.0 * step)
            assert np.abs(fd - grads[:, :, k]).max() <= 1e-6 * np.abs(grads).max(), k
    assert gp.samplePathsFromGaussianProcess((c["X"], c["y"][:, None]), 0, name, c["theta"]) is None
    # a posterior of two samples: the draws are split over the samples by weight, one paths object per theta used
    c1 = pr.case_reference(*pr.CASES[0])                          # se, d = 1
    obj = gp.defineGaussianProcess((c1["X"], c1["y"][:, None]), "se", variables=[("l", 0.05, 2.0), ("sf", 0.1, 5.0), ("sn", 0.01, 1.0)])
    assert gp.samplePathsFromGaussianProcess(obj, 5) is None      # unsampled
    obj = obj.append({"Samples": [{"Point": c1["theta"], "CrudePosteriorWeight": 0.6},
                                  {"Point": np.array([0.6, 0.7, 0.2]), "CrudePosteriorWeight": 0.4}]})
    x = c1["Xs"][:25]
    with gp.samplePathsFromGaussianProcess(obj, 40, Features=64, seed=1) as f:
        vals, grads = f(x[:, 0]), f.gradient(x[:, 0])
        assert vals.shape == (40, 25) and grads.shape == (40, 25, 1) and np.all(np.isfinite(vals))
        assert set(np.unique(f.sample)) == {0, 1} and len(f._parts) == 2
        fs = gp.gaussianProcessFunctionSamples(obj, x[:, 0], 40, seed=1)
        assert np.array_equal(f.sample, fs["Sample"])             # the assignment of gaussianProcessFunctionSamples
        fd = (f(x[:, 0] + 1e-5) - f(x[:, 0] - 1e-5)) / 2e-5
        assert np.abs(fd - grads[:, :, 0]).max() <= 1e-6 * np.abs(grads).max()
