"""Prediction from a sparse object over all posterior samples in one call (gphip_sparse_predict_samples) on the device, against
the numpy reference of tests/sparse_reference.py.  The numpy side of every case (conditioning, agreement of the reference's two
routes) is checked on the CPU by tests/test_sparse_samples.py.  Bars are those of tests/test_gpu_sparse.py: 1e-7 x max |y| for
means, 1e-7 x max k(x, x) for variances, 1e-8 relative for the bound against the reference; 1e-12 relative between the bound of
this call and gphip_sparse_bound_batch of the same rows (the bar DESIGN.md section 8f used for batched against one-theta)."""

import numpy as np
import pytest

import sparse_batch_cases as cases
import sparse_reference as ref
import sparse_samples_cases as sc
from bayesianinference_amd import _lib, gaussian_process as gp, synthetic as syn

pytestmark = pytest.mark.gpu

TOL, TOL_F, TOL_BATCH = 1e-7, 1e-8, 1e-12


def _errors(mean, var, F, want, rows):
    """largest scaled differences over the given rows: (means / max |y|, variances / max k(x, x), F relative)"""
    em = max(np.abs(mean[s] - want["mean"][s]).max() / want["ymax"] for s in rows)
    ev = max(np.abs(var[s] - want["var"][s]).max() / want["kmax"][s] for s in rows)
    eF = max(abs(F[s] - want["F"][s]) / abs(want["F"][s]) for s in rows) if F is not None else 0.0
    return em, ev, eF


def _within_bars(mean, var, F, want, rows, label):
    em, ev, eF = _errors(mean, var, F, want, rows)
    print(f"{label}: mean {em:.2e} var {ev:.2e} bound {eF:.2e}")
    assert em <= TOL and ev <= TOL and eF <= TOL_F, label


@pytest.mark.parametrize("label", [k for k in sc.LABELS if k != "failure"])
def test_parity_with_the_reference(label):
    kernel, X, y, Z, mean, rows, jit, good = sc.case(label)
    Xs = sc.test_points(X.shape[1])
    h = _lib.SparseHandle(X, y, Z, kernel, mean)
    for latent in (False, True):
        want = sc.reference(label, latent)
        mu, var, info, F = h.predict_samples(rows, Xs, jit, latent=latent, bound=True)
        assert mu.shape == (len(rows), sc.M) and var.shape == mu.shape and F.shape == (len(rows),)
        assert np.all(info == 0)
        _within_bars(mu, var, F, want, good, f"{label} latent={latent}")
        Fb, ib = h.bound_batch(rows, jit)
        eb = np.abs(F - Fb).max() / np.abs(Fb).min()
        d1m = d1v = 0.0
        for s, th in enumerate(rows):                               # (no bar of its own: both routes hold the reference's)
            assert h.fit(th, jit) == 0
            m1, v1 = h.predict(Xs, latent=latent)
            d1m = max(d1m, np.abs(mu[s] - m1).max() / want["ymax"])
            d1v = max(d1v, np.abs(var[s] - v1).max() / want["kmax"][s])
        print(f"{label} latent={latent}: against bound_batch {eb:.2e}; against fit + predict mean {d1m:.2e} var {d1v:.2e}")
        assert np.all(ib == 0) and np.all(np.abs(F - Fb) <= TOL_BATCH * np.abs(Fb))
    h.close()


def test_seams_of_chunks_and_groups_and_bit_identity():
    X, y, Z, mean, rows, Xs, want = sc.seams_case()
    S = len(rows)
    h = _lib.SparseHandle(X, y, Z, "se_ard", mean)
    jit = cases.JITTER
    names = ("sparse_samples_chunk", "sparse_batch_slots", "sparse_chunk")
    for key, val in ((None, 0), ("sparse_samples_chunk", 128), ("sparse_batch_slots", 2), ("sparse_chunk", 512)):
        for k in names:
            h.set_option(k, 0)
        if key:
            h.set_option(key, val)
        a = h.predict_samples(rows, Xs, jit, bound=True)
        b = h.predict_samples(rows, Xs, jit, bound=True)
        assert np.all(a[2] == 0)
        assert all(np.array_equal(p, q) for p, q in zip(a, b)), key            # the same bytes
        _within_bars(a[0], a[1], a[3], want, range(S), f"{key}={val}")
        print(key, "slots", h.get_option("last_sparse_slots"), "test chunk", h.get_option("last_sparse_samples_chunk"), "data chunk",
              h.get_option("last_sparse_chunk"))
        if key is None:
            assert h.get_option("last_sparse_samples_chunk") == 384 and h.get_option("last_sparse_slots") == S
            r = h.predict_samples(rows[::-1], Xs, jit, bound=True)
            assert all(np.array_equal(p[::-1], q) for p, q in zip(r, a))       # reversed rows, reversed outputs, bit for bit
        if key == "sparse_samples_chunk":
            assert h.get_option("last_sparse_samples_chunk") == 128             # chunks of 128, 128 and 44 points
        if key == "sparse_batch_slots":
            assert h.get_option("last_sparse_slots") == 1                       # groups of 2, 2 and 1 row
        if key == "sparse_chunk":
            assert h.get_option("last_sparse_chunk") == 512
    h.close()


def test_failures_stay_in_their_row():
    kernel, X, y, Z, mean, rows, jit, good = sc.case("failure")
    Xs = sc.test_points(2)
    want = sc.reference("failure", False)
    h = _lib.SparseHandle(X, y, Z, kernel, mean)
    mu, var, info, F = h.predict_samples(rows, Xs, jit, bound=True)
    print("info", info, "F", F)
    assert list(info) == [0, _lib.INFO_NAN, 0, _lib.INFO_NOT_SPD, 0]
    for s in (1, 3):
        assert np.all(np.isnan(mu[s])) and np.all(np.isnan(var[s])) and np.isnan(F[s])
    _within_bars(mu, var, F, want, good, "the good rows next to the failing ones")
    # 128 test points per pass against m_pad = 128: the shape at which a complete group would take the dataflow substitution
    h.set_option("sparse_samples_chunk", 128)
    mu3, var3, info3, F3 = h.predict_samples(rows, Xs, jit, bound=True)
    h.set_option("sparse_samples_chunk", 0)
    assert list(info3) == list(info) and np.all(np.isnan(mu3[[1, 3]])) and np.all(np.isnan(var3[[1, 3]]))
    _within_bars(mu3, var3, F3, want, good, "the same in chunks of 128 test points")
    sub = list(good)
    mu2, var2, info2, F2 = h.predict_samples(rows[sub], Xs, jit, bound=True)
    assert np.all(info2 == 0)
    pick = {k: (v[sub] if isinstance(v, np.ndarray) else v) for k, v in want.items()}
    _within_bars(mu2, var2, F2, pick, range(len(sub)), "the good rows alone")
    assert h.fit(rows[2], jit) == 0
    m1, v1 = h.predict(Xs)
    _within_bars(m1[None], v1[None], None, {k: (v[2:3] if isinstance(v, np.ndarray) else v) for k, v in want.items()}, [0],
                 "fit + predict afterwards")
    h.close()


def test_one_test_point_and_one_sample():
    kernel, X, y, Z, mean, rows, jit, _ = sc.case("parity0")
    h = _lib.SparseHandle(X, y, Z, kernel, mean)
    want = sc.reference("parity0", False)
    Xs = sc.test_points(X.shape[1])
    mu, var, info, F = h.predict_samples(rows, Xs[:1], jit, bound=True)                # M = 1
    assert mu.shape == (len(rows), 1) and np.all(info == 0)
    first = {k: (v[:, :1] if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in want.items()}
    _within_bars(mu, var, F, first, range(len(rows)), "M = 1")
    mu, var, info, F = h.predict_samples(rows[1], Xs, jit, bound=True)                 # S = 1
    assert mu.shape == (1, sc.M) and np.all(info == 0)
    one = {k: (v[1:2] if isinstance(v, np.ndarray) else v) for k, v in want.items()}
    _within_bars(mu, var, F, one, [0], "S = 1")
    h.close()


# fp32 objects against the fp64 reference at N = 2000, d = 3, m = 300, default fp32 jitter (1e-4 k(x, x) of the row), 77 test
# points: the case of tests/test_gpu_sparse.py, whose bars (4 x the values measured in DESIGN.md section 8c) hold for its theta,
# row 0 here.  Every other row holds 4 x the error the one-theta fp32 call shows on that same row (the 4 x rule of sections 8b / 8c).
FP32_BARS = {"mean": 4 * 5.49e-5, "var": 4 * 3.99e-6}


def test_fp32_objects_against_the_fp64_reference():
    X, y = syn.make_dataset(2000, 3)
    Z = cases.inducing(X, 300)
    rows = np.vstack([cases.base_theta("se_ard", 3, "const"), cases.theta_rows("se_ard", 3, "const", 3)])
    Xs = syn.make_test_points(77, 3)
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const", dtype=32)
    mu, var, info = h.predict_samples(rows, Xs)
    assert np.all(info == 0)
    ymax = np.abs(y).max()
    for s, th in enumerate(rows):
        sf2 = th[3] ** 2
        assert h.fit(th) == 0
        jit = h.get_option("last_jitter")
        assert jit == pytest.approx(1e-4 * sf2, rel=1e-12)
        m1, v1 = h.predict(Xs)
        wm, wv = ref.predict_formulas("se_ard", th, X, y, Z, jit, Xs, "const")
        em, ev = np.abs(mu[s] - wm).max() / ymax, np.abs(var[s] - wv).max() / sf2
        em1, ev1 = np.abs(m1 - wm).max() / ymax, np.abs(v1 - wv).max() / sf2
        bar_m, bar_v = (FP32_BARS["mean"], FP32_BARS["var"]) if s == 0 else (4 * em1, 4 * ev1)
        print(f"fp32 row {s}: mean {em:.2e} var {ev:.2e}; one-theta mean {em1:.2e} var {ev1:.2e}")
        assert em <= bar_m and ev <= bar_v, s
    h.close()


def test_status_contract():
    kernel, X, y, Z, mean, rows, jit, _ = sc.case("parity0")
    h = _lib.SparseHandle(X, y, Z, kernel, mean)
    lib = h._lib
    Xs = np.ascontiguousarray(sc.test_points(X.shape[1])[:5])
    Th = np.ascontiguousarray(rows[:2])
    S, p, M = 2, Th.shape[1], 5
    mu, var, F, info = np.zeros((S, M)), np.zeros((S, M)), np.zeros(S), np.zeros(S, dtype=np.int32)
    d, ip = _lib._d, info.ctypes.data_as(_lib._ip)

    def call(hh=h._h, th=d(Th), s=S, pp=p, j=jit, xs=Xs.ctypes.data, m=M, a=d(mu), b=d(var), f=d(F), i=ip):
        return lib.gphip_sparse_predict_samples(hh, th, s, pp, j, xs, m, 0, a, b, f, i)

    assert call(hh=None) == 1 and call(th=None) == 1 and call(xs=None) == 1 and call(a=None) == 1 and call(b=None) == 1
    assert call(i=None) == 1
    assert call(j=float("nan")) == 1 and call(j=float("inf")) == 1
    assert call(pp=p - 1) == 2 and call(s=0) == 2 and call(m=0) == 2
    assert h.fit(rows[0], jit) == 0
    h.predict(Xs)
    assert call(f=None) == 0 and np.all(info == 0)                  # the bound is optional
    with pytest.raises(_lib.GphipError) as e:                       # the call dropped the fit
        h.predict(Xs)
    assert e.value.status == 4
    h.close()


def test_python_mixture_prediction_is_one_call():
    X, y = syn.make_dataset(1000, 2)
    variables = [("l1", 0.2, 3.0), ("l2", 0.2, 3.0), ("sf", 0.3, 3.0), ("sn", 0.03, 0.5)]
    obj = gp.defineSparseGaussianProcess((X, y), "SEARD", 50, variables=variables, Jitter=1e-6)
    assert not obj.failed
    pts = np.array([[0.9, 1.1, 1.0, 0.12], [0.7, 1.3, 1.2, 0.2], [1.0, np.nan, 1.0, 0.1], [1.2, 0.8, 0.9, 0.15],
                    [0.8, 0.9, 1.4, 0.1], [1.1, 1.0, 1.1, 0.25]])
    w = np.array([0.3, 0.2, 0.1, 0.2, 0.1, 0.1])
    sampled = obj.append({"Samples": [{"Point": list(q), "CrudePosteriorWeight": float(v)} for q, v in zip(pts, w)]})
    handle = obj["SparseGaussianProcessData"]["HIPHandle"]
    calls = {"predict_samples": 0, "fit": 0}

    def counting(name):
        inner = getattr(handle, name)

        def wrapper(*a, **k):
            calls[name] += 1
            return inner(*a, **k)
        return wrapper

    handle.predict_samples, handle.fit = counting("predict_samples"), counting("fit")
    Xs = syn.make_test_points(40, 2)
    pred = gp.predictFromSparseGaussianProcess(sampled, Xs)
    assert calls == {"predict_samples": 1, "fit": 0}
    assert pred["Mean"].shape == (6, 40) and pred["StandardDeviation"].shape == (6, 40) and np.array_equal(pred["Weights"], w)
    assert np.all(np.isnan(pred["Mean"][2])) and np.all(np.isnan(pred["StandardDeviation"][2]))
    Xd, yd, Z = obj["Data"][0], np.asarray(obj["Data"][1]).ravel(), obj["InducingPoints"]
    for s in (0, 1, 3, 4, 5):
        wm, wv = ref.predict_formulas("se_ard", pts[s], Xd, yd, Z, 1e-6, Xs, "zero")
        em = np.abs(pred["Mean"][s] - wm).max() / np.abs(yd).max()
        ev = np.abs(pred["StandardDeviation"][s] ** 2 - wv).max() / pts[s][2] ** 2
        print(f"sample {s}: mean {em:.2e} var {ev:.2e}")
        assert em <= TOL and ev <= TOL
    one = gp.predictFromSparseGaussianProcess(obj, Xs, theta=pts[0])
    assert calls == {"predict_samples": 1, "fit": 1} and one["Mean"].shape == (1, 40)
    m1, _ = handle.predict(Xs)                                      # the theta= form left its fit resident
    assert np.array_equal(m1, one["Mean"][0])
    handle.close()
