"""Pathwise posterior function draws of the sparse object (gphip_sparse_paths_create and gphip_paths_eval / _eval_own on its
result) timed on the device.  fp64, SE-ARD, d = 8, F = 1024, warm, median of REPS calls with their min and max (host clock around
calls that end in a device synchronise).  One part per run:
  create [k ..]   sizes k of SIZES = (N, m, S): (32768, 1024, 64), (262144, 2048, 512), (1000000, 4096, 512): gphip_sparse_fit, then
                  the create call -- whole, its feature pass (weights, GenFeature at Z, the prior kernel) and its substitutions, from
                  the read-only options; the rest is the table on the host, uploads and allocation.
  eval            at (32768, 1024): eval of 64 draws at 16384 points against gphip_sparse_predict_draws at M = 16384, S = 64;
                  eval_own at S = 512, M = 32 with gradients; 64 draws at 10^6 points.
  law             CPU only: the closed-form covariance of the draws given the table (sparse_paths_reference.moments) against the
                  latent Sigma of the sparse object, F = 256, 1024, 16384, on the 70-point example of tests/test_sparse_paths.py, at
                  test points inside the data (the data pin the function) and outside (the posterior is wide).  The error is the
                  prior's: absolute, O(sf^2 / sqrt(F)), not relative to Sigma.
  baseline        calls this feature does not change -- exact paths.eval / eval_own (N = 8192), gphip_sparse_predict
                  (N = 32768, m = 1024, M = 16384) -- for a comparison of two builds: run it with GPHIP_LIB set to a library of
                  the parent commit and without, alternately, in fresh processes.
One JSON line per record; --out FILE also appends the lines to that file."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())

import numpy as np

REPS = int(os.environ.get("PATHS_REPS", "5"))
D, F = 8, 1024
SIZES = [(32768, 1024, 64), (262144, 2048, 512), (1000000, 4096, 512)]
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def timed(fn, reps=REPS):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return stats(ts)


def sparse_object(n, m):
    from bayesianinference_amd import _lib, gaussian_process as gp, synthetic as syn
    X, y = syn.make_dataset(n, D)
    h = _lib.SparseHandle(X, y, gp.selectInducingPoints(X, m, seed=1), "se_ard")
    return h, syn.default_theta("se_ard", D)


def create(which):
    for k in which:
        n, m, S = SIZES[k]
        h, th = sparse_object(n, m)
        emit({"what": "sparse_fit", "N": n, "m": m, **timed(lambda: h.fit(th))})
        cr, feat, sub = [], [], []
        for rep in range(REPS + 1):
            t0 = time.perf_counter()
            p = h.sample_paths(S, F, seed=rep)
            cr.append((time.perf_counter() - t0) * 1e3)
            feat.append(h.get_option("last_paths_feature_us") / 1e3)
            sub.append(h.get_option("last_paths_subst_us") / 1e3)
            p.close()
        emit({"what": "create", "N": n, "m": m, "S": S, "F": F, **stats(cr[1:]), "feature_ms": round(statistics.median(feat[1:]), 3),
              "subst_ms": round(statistics.median(sub[1:]), 3)})
        h.close()


def evaluate():
    from bayesianinference_amd import synthetic as syn
    n, m, _ = SIZES[0]
    h, th = sparse_object(n, m)
    assert h.fit(th) == 0
    Xs = syn.make_test_points(16384, D)
    with h.sample_paths(64, F, seed=1) as p:
        emit({"what": "eval", "N": n, "m": m, "S": 64, "M": 16384, "grad": False, **timed(lambda: p.eval(Xs)),
              "nsplit_kernel": h.get_option("last_paths_nsplit")})
        emit({"what": "eval", "N": n, "m": m, "S": 64, "M": 16384, "grad": True, **timed(lambda: p.eval(Xs, grad=True))})
        big = syn.make_test_points(1000000, D)
        emit({"what": "eval", "N": n, "m": m, "S": 64, "M": 1000000, "grad": False, **timed(lambda: p.eval(big), reps=2)})
    emit({"what": "sparse_predict_draws", "N": n, "m": m, "S": 64, "M": 16384,
          **timed(lambda: h.predict_draws(Xs, 64, seed=1, latent=True), reps=3)})
    own = np.ascontiguousarray(syn.make_test_points(512 * 32, D).reshape(512, 32, D))
    with h.sample_paths(512, F, seed=1) as p:
        emit({"what": "eval_own", "N": n, "m": m, "S": 512, "M": 32, "grad": True, **timed(lambda: p.eval_own(own, grad=True)),
              "nsplit_kernel": h.get_option("last_paths_own_nsplit")})
    h.close()


def law():
    sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
    import sparse_joint_reference as sj
    import sparse_paths_reference as spr
    from bayesianinference_amd import _lib
    m, d = 70, 3
    X, y, Z, Xs = spr.case_data(m, d)
    th = spr.theta_of("se_ard", d, "const", spr.ELL_NARROW)
    jit = spr.JREL * spr.SF ** 2
    for where, P in (("inside the data", Xs[:40]), ("outside the data", 2.5 * Xs[:40])):
        S = sj.joint_formulas("se_ard", th, X, y, Z, jit, P, "const", latent=True)[1]
        smax = float(np.max(np.diag(S)))
        for f in (256, 1024, 16384):
            om, ph, amp = _lib.rff_table("se_ard", d, th, f, 1)
            cov = spr.moments("se_ard", th, X, y, Z, jit, P, {"omega": om, "phase": ph, "amp": amp}, "const")["cov"]
            err = float(np.abs(cov - S).max())
            emit({"what": "law", "where": where, "F": f, "max_abs_error": float("%.3e" % err), "max_Sigma_ii": float("%.3e" % smax),
                  "of_max_Sigma_ii": round(err / smax, 4), "of_sf2": round(err / spr.SF ** 2, 5)})


def baseline():
    from bayesianinference_amd import _lib, synthetic as syn
    lib = os.environ.get("GPHIP_LIB", "this")
    X, y = syn.make_dataset(8192, D)
    e = _lib.Handle(X, y, "se_ard")
    assert e.fit(syn.default_theta("se_ard", D)) == 0
    Xs = syn.make_test_points(16384, D)
    own = np.ascontiguousarray(syn.make_test_points(512 * 32, D).reshape(512, 32, D))
    with e.sample_paths(512, F, seed=1) as p:
        emit({"what": "exact eval", "N": 8192, "S": 512, "M": 16384, "lib": lib, **timed(lambda: p.eval(Xs))})
        emit({"what": "exact eval_own", "N": 8192, "S": 512, "M": 32, "grad": True, "lib": lib, **timed(lambda: p.eval_own(own, grad=True))})
    e.close()
    n, m, _ = SIZES[0]
    h, th = sparse_object(n, m)
    assert h.fit(th) == 0
    emit({"what": "sparse_predict", "N": n, "m": m, "M": 16384, "lib": lib, **timed(lambda: h.predict(Xs))})
    h.close()


if __name__ == "__main__":
    part = sys.argv[1] if len(sys.argv) > 1 else "create"
    if part == "create":
        picks = [int(v) for v in sys.argv[2:] if v.isdigit()]
        create(picks or range(len(SIZES)))
    else:
        {"eval": evaluate, "law": law, "baseline": baseline}[part]()
