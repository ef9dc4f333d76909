"""gphip_paths_eval_own on the device -- every pathwise draw at its own points -- against the numpy reference of
tests/paths_own_reference.py evaluated on the table and the draw read back from the object (gphip_paths_get), so that the
comparisons are deterministic: the fp64 bar is the project's parity bar, 1e-8 of max |reference| (BAR of tests/test_gpu_paths.py).

Shapes: the cases of paths_reference.CASES (N = 300: ten slabs of 32 training points, the last ragged; S = 20, F = 100: a ragged
feature slab; d = 20 keeps its coordinates in registers and LDS) and d = 40 (> KB_LDS_MAXD: the global-memory form, five
gradient windows of 8), M = 7 points per draw: 140 pairs = one full workgroup of 128 and a ragged one, the seam inside draw 18.
Errors measured on an MI355X are in DESIGN.md section 8n."""

import numpy as np
import pytest

import paths_own_reference as por
import paths_reference as pr
from bayesianinference_amd import _lib, gaussian_process as gp, synthetic as syn

pytestmark = pytest.mark.gpu

BAR = 1e-8
S, F, M, SEED = 20, 100, 7, 5
IDS = [pr.case_id(c) for c in pr.CASES]


def _err(g, want):
    return float(np.abs(g - want).max() / np.abs(want).max())


def _fitted(c, dtype=64):
    h = _lib.Handle(c["X"], c["y"], c["kernel"], c["mean_kind"], dtype=dtype)
    assert h.fit(c["theta"]) == 0
    return h


def _own_points(c, s, m):
    """m points per draw, drawn separately per draw (one seeded stream cut into the draws' blocks)"""
    d = c["X"].shape[1]
    P = syn.make_test_points(s * m, d).reshape(s, m, d).copy()
    if s > 5 and m > 3:
        P[5, 3] = c["X"][11]                                      # a pair on a training point
    return P


def _reference(case, c, t, P, f=F, seed=SEED, dtype=np.float64):
    name, d, mean = case
    table = {"omega": t["omega"], "phase": t["phase"], "amp": _lib.rff_table(name, d, c["theta"], f, seed)[2]}
    return por.paths_own(name, c["theta"], c["X"], c["y"], P, table, t["w"], t["eps"], mean, dtype=dtype)


@pytest.mark.parametrize("case", pr.CASES, ids=IDS)
def test_own_points_match_the_reference(case):
    c = pr.case_reference(*case)
    P = _own_points(c, S, M)
    h = _fitted(c)
    with h.sample_paths(S, F, SEED) as p:
        t = p.table()
        out, dout = p.eval_own(P, grad=True)
    h.close()
    r = _reference(case, c, t, P)
    eo, ed = _err(out, r["out"]), _err(dout, r["dout"])
    print(f"{case[0]} d={case[1]} {case[2]}: out {eo:.3e} dout {ed:.3e} of max |reference|")
    assert out.shape == (S, M) and dout.shape == (S, M, case[1])
    assert eo <= BAR and ed <= BAR


def test_more_dimensions_than_the_lds_window():
    d, n, s, f = 40, 100, 5, 40
    X, y = syn.make_dataset(n, d)
    th = np.array(list(np.linspace(5.0, 8.0, d)) + [1.1, 0.15, 0.2])
    P = syn.make_test_points(s * M, d).reshape(s, M, d).copy()
    P[2, 3] = X[11]
    h = _lib.Handle(X, y, "matern52_ard", "const")
    assert h.fit(th) == 0
    with h.sample_paths(s, f, 2) as p:
        t = p.table()
        out, dout = p.eval_own(P, grad=True)
        assert p.eval_own(P).tobytes() == out.tobytes()
    h.close()
    table = {"omega": t["omega"], "phase": t["phase"], "amp": _lib.rff_table("matern52_ard", d, th, f, 2)[2]}
    r = por.paths_own("matern52_ard", th, X, y, P, table, t["w"], t["eps"], "const")
    print(f"d = 40: out {_err(out, r['out']):.3e} dout {_err(dout, r['dout']):.3e}")
    assert _err(out, r["out"]) <= BAR and _err(dout, r["dout"]) <= BAR


def test_against_the_shared_call():
    """all draws at the same 130 points: each call is within the bar of the same reference, so they agree to twice the bar"""
    case = pr.CASES[5]
    c = pr.case_reference(*case)
    h = _fitted(c)
    with h.sample_paths(S, F, SEED) as p:
        so, sd = p.eval(c["Xs"], grad=True)
        oo, od = p.eval_own(np.broadcast_to(c["Xs"], (S,) + c["Xs"].shape), grad=True)
    h.close()
    eo, ed = float(np.abs(oo - so).max() / np.abs(so).max()), float(np.abs(od - sd).max() / np.abs(sd).max())
    print(f"eval_own against eval at 130 shared points: out {eo:.3e} dout {ed:.3e}")
    assert len(c["Xs"]) == 130 and eo <= 2 * BAR and ed <= 2 * BAR


@pytest.mark.parametrize("s,m", [(1, 1), (20, 1), (20, 7), (3, 300)])
def test_lane_mapping_and_seams(s, m):
    """a single pair; a workgroup that spans many draws; 140 pairs (a workgroup boundary inside a draw, a ragged last workgroup);
    900 pairs (workgroups inside one draw and workgroups that cross a draw boundary)"""
    case = pr.CASES[1]
    c = pr.case_reference(*case)
    P = _own_points(c, s, m)
    h = _fitted(c)
    with h.sample_paths(s, F, SEED) as p:
        t = p.table()
        out, dout = p.eval_own(P, grad=True)
        only = p.eval_own(P)
    h.close()
    r = _reference(case, c, t, P)
    print(f"S = {s}, M = {m}: out {_err(out, r['out']):.3e} dout {_err(dout, r['dout']):.3e}")
    assert _err(out, r["out"]) <= BAR and _err(dout, r["dout"]) <= BAR
    assert only.tobytes() == out.tobytes()


def test_strips_chunks_and_bytes():
    case = pr.CASES[5]                                            # product of two terms + constant
    c = pr.case_reference(*case)
    s, m = 3, 300
    P = _own_points(c, s, m)
    h = _fitted(c)
    with h.sample_paths(s, F, SEED) as p:
        t = p.table()
        r = _reference(case, c, t, P)
        shared = p.eval(c["Xs"], grad=True)
        base, dbase = p.eval_own(P, grad=True)
        assert p.eval_own(P).tobytes() == base.tobytes()          # out does not depend on dout being asked for
        again = p.eval_own(P, grad=True)
        assert again[0].tobytes() == base.tobytes() and again[1].tobytes() == dbase.tobytes()      # two calls: the same bytes
        assert _err(base, r["out"]) <= BAR and _err(dbase, r["dout"]) <= BAR
        assert h.get_option("last_paths_own_us") > 0 and h.get_option("last_paths_own_nsplit") >= 1
        for split in (1, 2, 5):
            h.set_option("paths_split", split)
            o1, d1 = p.eval_own(P, grad=True)
            assert h.get_option("last_paths_own_nsplit") == split
            o2, d2 = p.eval_own(P, grad=True)
            assert o1.tobytes() == o2.tobytes() and d1.tobytes() == d2.tobytes()
            assert p.eval_own(P).tobytes() == o1.tobytes()
            print(f"paths_split {split}: out {_err(o1, r['out']):.3e} dout {_err(d1, r['dout']):.3e}")
            assert _err(o1, r["out"]) <= BAR and _err(d1, r["dout"]) <= BAR
        h.set_option("paths_split", 0)
        h.set_option("paths_chunk", 64)                           # 300 points per draw: seams after 64, 128, 192 and 256
        oc, dc = p.eval_own(P, grad=True)
        h.set_option("paths_chunk", 0)
        print(f"paths_chunk 64 against the default: out {_err(oc, base):.3e} dout {_err(dc, dbase):.3e}")
        assert _err(oc, base) <= BAR and _err(dc, dbase) <= BAR
        assert _err(oc, r["out"]) <= BAR and _err(dc, r["dout"]) <= BAR
        after = p.eval(c["Xs"], grad=True)                        # the shared call returns what it returned before
        assert after[0].tobytes() == shared[0].tobytes() and after[1].tobytes() == shared[1].tobytes()
    h.close()


@pytest.mark.parametrize("case", [pr.CASES[1], pr.CASES[5]], ids=[IDS[1], IDS[5]])
def test_fp32_handle(case):
    """The bar is 10 x the error of the numpy reference evaluated in float32 arithmetic against its float64 evaluation, on the
    same table and draw -- never measured against the device (the rule of tests/test_gpu_paths.py::test_fp32_handle)."""
    c = pr.case_reference(*case)
    P = _own_points(c, S, M)
    h = _fitted(c, dtype=32)
    with h.sample_paths(S, F, SEED) as p:
        t = p.table()
        out, dout = p.eval_own(P, grad=True)
        assert p.eval_own(P).tobytes() == out.tobytes()
    h.close()
    r64, r32 = _reference(case, c, t, P), _reference(case, c, t, P, dtype=np.float32)
    for k, dev in (("out", out), ("dout", dout)):
        base, e = _err(r32[k].astype(np.float64), r64[k]), _err(dev, r64[k])
        print(f"fp32 {case[0]} d={case[1]} {k}: device {e:.3e}, numpy float32 {base:.3e}, bar {10 * base:.3e}")
        assert e <= 10 * base, k


def test_statuses_and_the_null_kernel():
    case = pr.CASES[1]
    name, d, mean = case
    c = pr.case_reference(*case)
    lib = _lib.load()
    h = _fitted(c)
    P = _own_points(c, 2, 1)
    with h.sample_paths(2, 8, 0) as p:
        out = np.zeros((2, 1))
        assert lib.gphip_paths_eval_own(p._q, None, 1, _lib._d(out), None) == 1
        assert lib.gphip_paths_eval_own(p._q, P.ctypes.data, 1, None, None) == 1
        assert lib.gphip_paths_eval_own(p._q, P.ctypes.data, 0, _lib._d(out), None) == 2
        assert lib.gphip_paths_eval_own(None, P.ctypes.data, 1, _lib._d(out), None) == 1
        assert np.all(out == 0.0)                                  # nothing was written
    h.close()
    null = _lib.Handle(c["X"], c["y"], "null", "const")
    assert null.fit(np.array([0.3, 0.2])) == 0
    with null.sample_paths(3, 10, 0) as p:
        out, dout = p.eval_own(_own_points(c, 3, 4), grad=True)
    null.close()
    assert np.all(out == 0.2) and np.all(dout == 0.0) and out.shape == (3, 4) and dout.shape == (3, 4, d)


def test_maximize_and_thompson_sampling():
    """the d = 1 configuration of tests/test_paths_own.py on the device: every draw's maximiser is (a) no worse than its best
    candidate and (b) within the grid's own slack of the maximum over a 4001-point grid, both evaluated by the device's eval"""
    case = pr.CASES[0]
    name, d, mean = case
    c = pr.case_reference(*case)
    box = np.array([[c["X"].min(), c["X"].max()]])
    grid = np.linspace(box[0, 0], box[0, 1], 4001)
    with gp.samplePathsFromGaussianProcess((c["X"], c["y"][:, None]), S, name, c["theta"], Features=F, seed=SEED) as f:
        res = f.maximize(box, candidates=64, starts=4, seed=0)
        fgrid = f(grid[:, None])
        cand = box[0, 0] + (box[0, 1] - box[0, 0]) * np.random.default_rng(0).random((64, 1))
        best_cand = f(cand).max(axis=1)
        at = f.own(res["x"][:, None, :])[:, 0]
        g = f.own_gradient(res["x"][:, None, :])
    delta = por.grid_slack(fgrid, grid[1] - grid[0])
    worst_a, worst_b = float((res["f"] - best_cand).min()), float((res["f"] - fgrid.max(axis=1) + delta).min())
    print(f"maximize on the device: min (f(x^) - best candidate) {worst_a:.3e}, min (f(x^) - grid max + slack) {worst_b:.3e}")
    assert res["x"].shape == (S, 1) and res["f"].shape == (S,) and g.shape == (S, 1, 1)
    assert np.abs(at - res["f"]).max() <= 1e-12 * np.abs(at).max()      # the value returned is the draw at the point returned
    assert np.all(res["x"] >= box[0, 0]) and np.all(res["x"] <= box[0, 1])
    assert np.all(res["f"] >= best_cand)                          # (a)
    assert np.all(res["f"] >= fgrid.max(axis=1) - delta)          # (b)
    ts = gp.thompsonSampleFromGaussianProcess((c["X"], c["y"][:, None]), 6, box, name, c["theta"], Features=F, seed=SEED, candidates=64, iterations=20)
    assert ts["x"].shape == (6, d) and ts["f"].shape == (6,) and ts["sample"].shape == (6,)
    assert np.all(ts["x"] >= box[0, 0]) and np.all(ts["x"] <= box[0, 1]) and np.all(np.isfinite(ts["f"]))
    assert gp.thompsonSampleFromGaussianProcess((c["X"], c["y"][:, None]), 0, box, name, c["theta"]) is None
