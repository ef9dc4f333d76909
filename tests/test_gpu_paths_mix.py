"""gphip_paths_create_samples on the device -- pathwise draws over several hyper-parameter rows in one object -- against the numpy
reference of tests/paths_mix_reference.py (per row tests/paths_reference.py and tests/paths_own_reference.py, stacked in draw order)
evaluated on the tables, w and eps read back from the object, so that the comparisons are deterministic.  fp64 bar: the project's
parity bar, 1e-8 of max |reference|; fp32 bar: that of tests/test_gpu_paths.py, 10 x the float32 numpy evaluation's own error
against float64, never the device's.

Shapes: those of the existing paths tests -- N = 300 (ten slabs of 32 training points, the last ragged), F = 100 (a ragged feature
slab), M = 7.  Rows: the case's theta and copies with the length scales multiplied by 0.8 and 1.25; the noise is kept, so every
row factors, and every test asserts that all info are 0.  R = 3 with counts (7, 0, 13): 140 pairs = a workgroup seam inside a row
(draw 18), a seam across rows inside the first workgroup and a ragged last workgroup; a row without draws in between.
Errors measured on an MI355X are in DESIGN.md section 8q."""
import ctypes as C

import numpy as np
import pytest

import paths_mix_reference as pmr
import paths_reference as pr
from bayesianinference_amd import _lib, gaussian_process as gp, synthetic as syn

pytestmark = pytest.mark.gpu

BAR = 1e-8
F, M = 100, 7
COUNTS, SEEDS = (7, 0, 13), (5, 6, 7)
IDS = [pr.case_id(c) for c in pr.CASES]
SE_ARD_BODY = "T s = 0; for (int k = 0; k < D; ++k) { const T u = (X(k) - Y(k)) / P(k); s += u * u; } return P(D) * P(D) * exp((T)-0.5 * s);"


def _err(g, want):
    assert np.all(np.isfinite(want)) and g.shape == want.shape      # no comparison skips a row silently
    return float(np.abs(g - want).max() / np.abs(want).max())


def _handle(c, dtype=64, opts=None):
    h = _lib.Handle(c["X"], c["y"], c["kernel"], c["mean_kind"], dtype=dtype)
    for k, v in (opts or {}).items():
        h.set_option(k, v)
    return h


def _own_points(c, s, m):
    d = c["X"].shape[1]
    P = syn.make_test_points(s * m, d).reshape(s, m, d).copy()
    if s > 5 and m > 3:
        P[5, 3] = c["X"][11]                                      # a pair on a training point
    return P


def _read(p):
    """(tables per row, w, eps, v) of a mixture object, and the checks every test makes: all info 0, rows in draw order"""
    R, row_of = p.rows()
    assert np.all(p.info == 0) and len(p.info) == R
    t = p.table()
    assert set(t) == {"w", "eps", "v"}
    return [p.table(r) for r in range(R)], t["w"], t["eps"], t["v"], row_of


def _check(case, c, th, counts, p, P, pts, bar=BAR, label=""):
    """v, eval_own and eval of the mixture object p against the reference on what is read back from it"""
    name, d, mean = case
    tables, w, eps, v, row_of = _read(p)
    assert np.array_equal(row_of, pmr.row_of_draw(counts))
    oo, od = p.eval_own(P, grad=True)
    so, sd = p.eval(pts, grad=True)
    ro = pmr.mix(name, th, c["X"], c["y"], P, tables, w, eps, counts, mean, own=True)
    rs = pmr.mix(name, th, c["X"], c["y"], pts, tables, w, eps, counts, mean)
    errs = {"v": _err(v, rs["v"]), "own out": _err(oo, ro["out"]), "own dout": _err(od, ro["dout"]), "eval out": _err(so, rs["out"]),
            "eval dout": _err(sd, rs["dout"])}
    print(f"{label}{name} d={d} {mean}: " + " ".join(f"{k} {e:.3e}" for k, e in errs.items()) + " of max |reference|")
    for k, e in errs.items():
        assert e <= bar, (k, e)
    return errs


@pytest.mark.parametrize("case", pr.CASES, ids=IDS)
def test_parity_per_draw(case):
    name, d, mean = case
    c = pr.case_reference(*case)
    th = pmr.rows_of(name, d, c["theta"])
    S = sum(COUNTS)
    h = _handle(c)
    with h.sample_paths_samples(th, COUNTS, SEEDS, F) as p:
        assert (p.S, p.N, p.d) == (S, len(c["X"]), d) and S * M == 140
        _check(case, c, th, COUNTS, p, _own_points(c, S, M), c["Xs"][:M])
    h.close()


@pytest.mark.parametrize("case", [pr.CASES[1], pr.CASES[5], pr.CASES[6]], ids=[IDS[1], IDS[5], IDS[6]])
def test_against_the_loop_route(case):
    """per row fit(theta_r) + sample_paths(counts[r], F, seeds[r]): table, w and eps the same bytes; values and gradients within
    twice the bar (each route is within the bar of the same reference).  One-term ARD, product + constant, and the sum at d = 20."""
    name, d, mean = case
    c = pr.case_reference(*case)
    th = pmr.rows_of(name, d, c["theta"])
    S, start = sum(COUNTS), np.concatenate([[0], np.cumsum(COUNTS)])
    P, pts = _own_points(c, S, M), c["Xs"][:M]
    h = _handle(c)
    with h.sample_paths_samples(th, COUNTS, SEEDS, F) as p:
        tables, w, eps, v, _ = _read(p)
        oo, od = p.eval_own(P, grad=True)
        so, sd = p.eval(pts, grad=True)
    for r in range(len(COUNTS)):
        om, ph, amp = _lib.rff_table(name, d, th[r], F, SEEDS[r])
        assert tables[r]["omega"].tobytes() == om.tobytes() and tables[r]["phase"].tobytes() == ph.tobytes() and tables[r]["amp"].tobytes() == amp.tobytes()
        if COUNTS[r] == 0:
            continue
        sl = slice(start[r], start[r + 1])
        assert h.fit(th[r]) == 0
        with h.sample_paths(COUNTS[r], F, SEEDS[r]) as one:
            t = one.table()
            lo, ld = one.eval_own(P[sl], grad=True)
            ls, lsd = one.eval(pts, grad=True)
        assert t["omega"].tobytes() == om.tobytes() and t["w"].tobytes() == w[sl].tobytes() and t["eps"].tobytes() == eps[sl].tobytes()
        errs = (_err(v[sl], t["v"]), _err(oo[sl], lo), _err(od[sl], ld), _err(so[sl], ls), _err(sd[sl], lsd))
        print(f"{name} row {r} against the loop route: v {errs[0]:.3e} own {errs[1]:.3e} {errs[2]:.3e} eval {errs[3]:.3e} {errs[4]:.3e}")
        assert max(errs) <= 2 * BAR
    h.close()


@pytest.mark.parametrize("m", [1, 7])
def test_many_rows_in_one_workgroup(m):
    """R = 40 rows of one draw each: at M = 1 one workgroup holds all 40 rows, at M = 7 a workgroup of 128 pairs spans 19 or 20.
    d = 3 stages 7 rows of features and 64 rows of kernel data: by the rule the feature contraction reads global memory, the
    kernel contraction LDS; "paths_mix_stage" 0 sends both to global memory, and R = 3 of the same case (7 draws and 13 in a
    workgroup) runs both from LDS."""
    case = pr.CASES[1]
    name, d, mean = case
    c = pr.case_reference(*case)
    R = 40
    th = pmr.rows_of(name, d, c["theta"], np.linspace(0.8, 1.25, R))
    counts, seeds = [1] * R, list(range(100, 100 + R))
    P, pts = _own_points(c, R, m), c["Xs"][:m]
    got = {}
    for stage in (-1, 0):
        h = _handle(c, opts={"paths_mix_stage": stage})
        with h.sample_paths_samples(th, counts, seeds, F) as p:
            assert h.get_option("last_paths_mix_groups") == 1
            _check(case, c, th, counts, p, P, pts, label=f"R=40 M={m} stage={stage}: ")
            got[stage] = p.eval_own(P, grad=True)
        h.close()
    assert _err(got[0][0], got[-1][0]) <= 2 * BAR and _err(got[0][1], got[-1][1]) <= 2 * BAR
    th3 = pmr.rows_of(name, d, c["theta"])
    h = _handle(c)
    with h.sample_paths_samples(th3, COUNTS, SEEDS, F) as p:
        _check(case, c, th3, COUNTS, p, _own_points(c, sum(COUNTS), m), pts, label=f"R=3 M={m} staged: ")
    h.close()


@pytest.mark.parametrize("d", [8, 9, 16, 17, 32, 33, 40])
def test_dimensions(d):
    """every instantiation (DW = 8, 16, 32 at their upper edges and one above) and the global-memory form with its gradient
    windows of 8 (d = 33: five windows, the last of one coordinate; d = 40: five full ones)"""
    n, f, counts, seeds = 100, 40, (4, 0, 5), (2, 3, 4)
    X, y = syn.make_dataset(n, d)
    base = np.array(list(np.linspace(5.0, 8.0, d)) + [1.1, 0.15, 0.2])
    case = ("matern52_ard", d, "const")
    c = {"X": X, "y": y, "kernel": "matern52_ard", "mean_kind": "const"}
    th = pmr.rows_of("matern52_ard", d, base)
    S = sum(counts)
    P = syn.make_test_points(S * M, d).reshape(S, M, d).copy()
    P[2, 3] = X[11]
    h = _handle(c)
    with h.sample_paths_samples(th, counts, seeds, f) as p:
        _check(case, c, th, counts, p, P, syn.make_test_points(M, d))
    h.close()


def test_groups():
    case = pr.CASES[2]                                            # matern52_ard, d = 8
    name, d, mean = case
    c = pr.case_reference(*case)
    th = pmr.rows_of(name, d, c["theta"], (1.0, 0.8, 1.25, 0.9, 1.1))
    counts, seeds = (3, 2, 4, 1, 5), (1, 2, 3, 4, 5)
    h = _handle(c, opts={"paths_mix_slots": 2})
    with h.sample_paths_samples(th, counts, seeds, F) as p:
        assert h.get_option("last_paths_mix_groups") == 3 and h.get_option("last_paths_mix_slots") == 2
        assert h.get_option("last_paths_mix_create_us") > 0
        _check(case, c, th, counts, p, _own_points(c, sum(counts), M), c["Xs"][:M], label="three groups: ")
    h.close()


def test_bytes():
    case = pr.CASES[5]                                            # product of two terms + constant
    name, d, mean = case
    c = pr.case_reference(*case)
    th = pmr.rows_of(name, d, c["theta"])
    S = sum(COUNTS)
    P, pts = _own_points(c, S, M), c["Xs"][:M]
    h = _handle(c)
    with h.sample_paths_samples(th, COUNTS, SEEDS, F) as p:
        o1, d1 = p.eval_own(P, grad=True)
        assert p.eval_own(P).tobytes() == o1.tobytes()            # out does not depend on dout being asked for
        o2, d2 = p.eval_own(P, grad=True)
        assert o1.tobytes() == o2.tobytes() and d1.tobytes() == d2.tobytes()
        s1, sd1 = p.eval(pts, grad=True)
        assert p.eval(pts).tobytes() == s1.tobytes()
        b1, bd1 = p.eval_own(np.broadcast_to(pts, (S,) + pts.shape), grad=True)
        assert s1.tobytes() == b1.tobytes() and sd1.tobytes() == bd1.tobytes()      # eval is eval_own on the broadcast points
        with h.sample_paths_samples(th, COUNTS, SEEDS, F) as p2:   # the same call again: the same object
            t1, t2 = p.table(), p2.table()
            assert all(t1[k].tobytes() == t2[k].tobytes() for k in ("w", "eps", "v"))
            assert p2.eval_own(P).tobytes() == o1.tobytes()
        h.set_option("paths_split", 3)
        _check(case, c, th, COUNTS, p, P, pts, label="three strips: ")
        assert h.get_option("last_paths_own_nsplit") == 3 and h.get_option("last_paths_nsplit") == 3
        h.set_option("paths_split", 0)
        h.set_option("paths_chunk", 4)                            # 7 points per draw: a seam after 4
        oc, dc = p.eval_own(P, grad=True)
        h.set_option("paths_chunk", 0)
        assert _err(oc, o1) <= 2 * BAR and _err(dc, d1) <= 2 * BAR
    h.close()


def test_a_failing_row():
    case = pr.CASES[1]
    name, d, mean = case
    c = pr.case_reference(*case)
    good = pmr.rows_of(name, d, c["theta"])
    counts, seeds = (7, 5, 8), (5, 6, 7)
    S, P, pts = sum(counts), _own_points(c, sum(counts), M), c["Xs"][:M]
    bad = good.copy()
    bad[1, 1] = np.nan
    h = _handle(c)
    with h.sample_paths_samples(good, counts, seeds, F) as p:
        assert np.all(p.info == 0)
        vg, (og, dg), (sg, sdg) = p.table()["v"], p.eval_own(P, grad=True), p.eval(pts, grad=True)
    with h.sample_paths_samples(bad, counts, seeds, F) as p:
        assert list(p.info) == [0, _lib.INFO_NAN, 0]
        vb, (ob, db), (sb, sdb) = p.table()["v"], p.eval_own(P, grad=True), p.eval(pts, grad=True)
    dead, live = slice(7, 12), np.r_[0:7, 12:20]
    for g, b in ((vg, vb), (og, ob), (dg, db), (sg, sb), (sdg, sdb)):
        assert np.all(np.isnan(b[dead])) and np.all(np.isfinite(g))
        assert b[live].tobytes() == g[live].tobytes()             # the other rows: the bytes of the call with a valid theta there
    # every row with draws fails: no object, status OK; the row without draws is not looked at
    allbad = good.copy()
    allbad[0, 0] = np.inf
    allbad[2, 2] = np.nan
    assert h.sample_paths_samples(allbad, (3, 0, 2), seeds, F) is None
    assert list(h.last_paths_info) == [_lib.INFO_NAN, 0, _lib.INFO_NAN]
    h.close()
    assert h._h is None


def test_statuses_and_lifetime():
    case = pr.CASES[1]
    name, d, mean = case
    c = pr.case_reference(*case)
    th = pmr.rows_of(name, d, c["theta"])
    lib = _lib.load()
    h = _handle(c)
    R, p = th.shape
    cnt, sd, info, q = (C.c_int * R)(*COUNTS), (C.c_uint64 * R)(*SEEDS), (C.c_int * R)(), C.c_void_p()
    tp = _lib._d(th)

    def call(hh=None, T=tp, r=R, pp=p, cn=cnt, s=sd, f=F, out=C.byref(q), inf=info):
        rc = lib.gphip_paths_create_samples(h._h if hh is None else hh, T, r, pp, cn, s, f, out, inf)
        assert not q.value or rc == 0
        return rc
    assert lib.gphip_paths_create_samples(None, tp, R, p, cnt, sd, F, C.byref(q), info) == 1
    assert call(T=None) == 1 and call(cn=None) == 1 and call(s=None) == 1 and call(out=None) == 1 and call(inf=None) == 1
    assert call(pp=p + 1) == 2 and call(r=0) == 2 and call(f=0) == 2
    assert call(cn=(C.c_int * R)(7, -1, 13)) == 2                 # a negative count
    assert call(cn=(C.c_int * R)(0, 0, 0)) == 2                   # S < 1
    assert call(cn=(C.c_int * R)(1000, 1000, 49)) == 2            # S = 2049
    assert call(cn=(C.c_int * R)(1000, 1000, 48), f=40000) == 2   # Ftot S > 2^26
    big = np.tile(th[0], (2000, 1))                               # R Ftot d = 2000 x 30000 x 3 > 2^27 with Ftot S = 30000
    one = (C.c_int * 2000)(1)
    assert lib.gphip_paths_create_samples(h._h, _lib._d(big), 2000, p, one, (C.c_uint64 * 2000)(), 30000, C.byref(q), (C.c_int * 2000)()) == 2
    assert not q.value
    # a resident fit is dropped by the call, and the object blocks the parent's destruction
    assert h.fit(th[0]) == 0
    pm, _ = h.predict(c["Xs"][:M])
    with h.sample_paths_samples(th, COUNTS, SEEDS, F) as pth:
        with pytest.raises(_lib.GphipError) as e:
            h.predict(c["Xs"][:M])
        assert e.value.status == 4
        before = pth.eval(c["Xs"][:M])
        assert h.fit(th[1]) == 0                                  # a later fit does not touch the object
        assert pth.eval(c["Xs"][:M]).tobytes() == before.tobytes()
        with pytest.raises(_lib.GphipError) as e:
            h.close()
        assert e.value.status == 4
        # the ordinary object's calls on a mixture object and the new ones on an ordinary object
        S, ftot, n, dd = C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        assert lib.gphip_paths_shape(pth._q, C.byref(S), C.byref(ftot), C.byref(n), C.byref(dd)) == 0
        assert (S.value, ftot.value, n.value, dd.value) == (sum(COUNTS), F, len(c["X"]), d)
        om = np.zeros((F, d))
        assert lib.gphip_paths_get(pth._q, _lib._d(om), None, None, None, None) == 1
        assert lib.gphip_paths_get(pth._q, None, _lib._d(np.zeros(F)), None, None, None) == 1
        assert lib.gphip_paths_get_table(pth._q, 3, _lib._d(om), None, None) == 2 and lib.gphip_paths_get_table(pth._q, -1, None, None, None) == 2
        with h.sample_paths(4, F, 9) as plain:
            assert plain.rows()[0] == 1 and np.array_equal(plain.rows()[1], np.zeros(4))
            t = plain.table()
            assert plain.table(0)["omega"].tobytes() == t["omega"].tobytes() and plain.table(0)["phase"].tobytes() == t["phase"].tobytes()
            assert plain.table(0)["amp"].tobytes() == _lib.rff_table(name, d, th[1], F, 9)[2].tobytes()
    assert np.all(np.isfinite(pm))
    h.close()
    assert h._h is None
    custom = _lib.Handle(c["X"], c["y"], _lib.CustomKernel(SE_ARD_BODY, d + 1), mean)
    assert lib.gphip_paths_create_samples(custom._h, tp, R, p, cnt, sd, F, C.byref(q), info) == 6 and not q.value
    custom.close()


def test_fp32_handle():
    """The bar is 10 x the error of the numpy reference evaluated in float32 arithmetic against its float64 evaluation, on the
    same tables and draws -- never measured against the device."""
    case = pr.CASES[1]
    name, d, mean = case
    c = pr.case_reference(*case)
    th = pmr.rows_of(name, d, c["theta"])
    S = sum(COUNTS)
    P, pts = _own_points(c, S, M), c["Xs"][:M]
    h = _handle(c, dtype=32)
    with h.sample_paths_samples(th, COUNTS, SEEDS, F) as p:
        tables, w, eps, v, _ = _read(p)
        oo, od = p.eval_own(P, grad=True)
        so, sd = p.eval(pts, grad=True)
    h.close()
    r64 = {"own": pmr.mix(name, th, c["X"], c["y"], P, tables, w, eps, COUNTS, mean, own=True),
           "eval": pmr.mix(name, th, c["X"], c["y"], pts, tables, w, eps, COUNTS, mean)}
    r32 = {"own": pmr.mix(name, th, c["X"], c["y"], P, tables, w, eps, COUNTS, mean, own=True, dtype=np.float32),
           "eval": pmr.mix(name, th, c["X"], c["y"], pts, tables, w, eps, COUNTS, mean, dtype=np.float32)}
    for which, k, dev in (("eval", "v", v), ("own", "out", oo), ("own", "dout", od), ("eval", "out", so), ("eval", "dout", sd)):
        base, got = _err(r32[which][k].astype(np.float64), r64[which][k]), _err(dev, r64[which][k])
        print(f"fp32 {which} {k}: device {got:.3e}, numpy float32 {base:.3e}, bar {10 * base:.3e}")
        assert got <= 10 * base, (which, k)


def test_null_kernel():
    case = pr.CASES[1]
    c = pr.case_reference(*case)
    d = case[1]
    null = _lib.Handle(c["X"], c["y"], "null", "const")
    th = np.array([[0.3, 0.2], [0.4, -1.5], [0.5, 0.7]])
    with null.sample_paths_samples(th, (2, 0, 3), (1, 2, 3), 10) as p:
        assert np.all(p.info == 0) and p.Ftot == 0 and p.rows()[0] == 3
        out, dout = p.eval(c["Xs"][:M], grad=True)
        oo = p.eval_own(np.zeros((5, 2, d)))
    null.close()
    assert np.all(out[:2] == 0.2) and np.all(out[2:] == 0.7) and np.all(dout == 0.0) and out.shape == (5, M) and dout.shape == (5, M, d)
    assert np.all(oo[:2] == 0.2) and np.all(oo[2:] == 0.7)


def test_python_end_to_end():
    c1 = pr.case_reference(*pr.CASES[0])                          # se, d = 1: the object of test_gpu_paths.py::test_python_layer
    obj = gp.defineGaussianProcess((c1["X"], c1["y"][:, None]), "se", variables=[("l", 0.05, 2.0), ("sf", 0.1, 5.0), ("sn", 0.01, 1.0)])
    obj = obj.append({"Samples": [{"Point": c1["theta"], "CrudePosteriorWeight": 0.6},
                                  {"Point": np.array([0.6, 0.7, 0.2]), "CrudePosteriorWeight": 0.4}]})
    x = c1["Xs"][:25]
    own = np.stack([np.roll(x, k, axis=0)[:5] for k in range(40)])               # [40, 5, 1]: every draw at its own points
    with gp.samplePathsFromGaussianProcess(obj, 40, Features=64, seed=1) as f:
        assert len(f._parts) == 2
        loop = (f(x[:, 0]), f.gradient(x[:, 0]), f.own(own), f.own_gradient(own), np.array(f.sample))
    with gp.samplePathsFromGaussianProcess(obj, 40, Features=64, seed=1, Batched=True) as f:
        assert len(f._parts) == 1 and np.array_equal(f.sample, loop[4]) and set(np.unique(f.sample)) == {0, 1}
        vals, grads = f(x[:, 0]), f.gradient(x[:, 0])
        got = (vals, grads, f.own(own), f.own_gradient(own))
        for k, (g, want) in enumerate(zip(got, loop[:4])):
            e = _err(g, want)
            print(f"Batched against the loop route, quantity {k}: {e:.3e}")
            assert e <= 2 * BAR, k                                # draw by draw: both routes are within the bar of one reference
        fd = (f(x[:, 0] + 1e-5) - f(x[:, 0] - 1e-5)) / 2e-5
        assert np.abs(fd - grads[:, :, 0]).max() <= 1e-6 * np.abs(grads).max()
    box = np.array([[c1["X"].min(), c1["X"].max()]])
    res = gp.thompsonSampleFromGaussianProcess(obj, 12, box, Features=64, seed=2, Batched=True, candidates=64, iterations=10)
    assert res["x"].shape == (12, 1) and np.all(np.isfinite(res["f"])) and np.all(res["x"] >= box[0, 0]) and np.all(res["x"] <= box[0, 1])
    cand = box[0, 0] + (box[0, 1] - box[0, 0]) * np.random.default_rng(2).random((64, 1))
    with gp.samplePathsFromGaussianProcess(obj, 12, Features=64, seed=2, Batched=True) as f:
        best = f(cand[:, 0]).max(axis=1)
        assert np.array_equal(f.sample, res["sample"])
    assert np.all(res["f"] >= best)                               # the maximisers are at least the best candidate
