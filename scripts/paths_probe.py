"""Pathwise posterior function draws (gphip_paths_create / gphip_paths_eval) timed on the device.  fp64, SE-ARD, d = 8, F = 1024,
warm, median of REPS calls with their min and max (host clock around calls that end in a device synchronise).
  * create, N in PATHS_N (default 8192, 32768) x S in (64, 512): the whole call, its feature pass (weights + GenFeature on the
    training points + the residual kernel) and its substitutions, from the parent's read-only options; the rest is the table on
    the host, uploads and allocation.
  * eval, M = 1000 and 16384, with and without gradients, and the kernel-level view from profile class 6 (event-timed
    paths_contract_kernel launches: GenFeature and GenKernel separately, as a fraction of the fp64 MFMA figure -- 2 S M j flops
    per generator pass over the 78.6 TFLOP/s matrix peak -- and the pairs generated per second).
  * gphip_predict_draws at the same N, M, S (M <= GPHIP_JOINT_MAX_M): the only other way to S coherent draws; it has no gradient
    and draws again on every call.
  * one eval at M = 10^6 (S = 64), which gphip_predict_draws cannot do.
  * --baseline: gphip_predict (1000 points), gphip_predict_draws (M = 1000, S = 64) and gphip_solve (8 vectors) only, for a
    comparison of two builds: run it with GPHIP_LIB set to a library of the parent commit and without, alternately.
  * --one N S M: one create and two evaluations with gradients, nothing timed: the call pattern to run under
    `rocprofv3 --kernel-trace --stats` (the four paths_contract_kernel instantiations' own times) and, in a run of its own, under
    `rocprofv3 --pmc` (SQ_VALU_MFMA_BUSY_CYCLES against SQ_BUSY_CYCLES and SQ_ACTIVE_INST_VALU: matrix pipe or generator).
One JSON line per record; --out FILE also appends the lines to that file."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())

import numpy as np

REPS = int(os.environ.get("PATHS_REPS", "5"))
NS = [int(v) for v in os.environ.get("PATHS_N", "8192,32768").split(",")]
D, F = 8, 1024
MFMA_F64_FLOPS = 78.6e12
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


def fitted(n):
    from bayesianinference_amd import _lib, synthetic as syn
    X, y = syn.make_dataset(n, D)
    h = _lib.Handle(X, y, "se_ard")
    assert h.fit(syn.default_theta("se_ard", D)) == 0
    return h, y


def baseline():
    from bayesianinference_amd import synthetic as syn
    for n in NS:
        h, y = fitted(n)
        Xs = syn.make_test_points(1000, D)
        rhs = np.tile(y, (8, 1)) * np.arange(1, 9)[:, None]
        emit({"what": "predict", "N": n, "M": 1000, "lib": os.environ.get("GPHIP_LIB", "this"), **timed(lambda: h.predict(Xs))})
        emit({"what": "predict_draws", "N": n, "M": 1000, "S": 64, "lib": os.environ.get("GPHIP_LIB", "this"),
              **timed(lambda: h.predict_draws(Xs, 64, seed=1, latent=True, jitter=1e-8))})
        emit({"what": "solve", "N": n, "nrhs": 8, "lib": os.environ.get("GPHIP_LIB", "this"), **timed(lambda: h.solve(rhs))})
        h.close()


def kernel_view(h, p, Xs, grad):
    """event times of the contraction launches of one evaluation (profile class 6), split by the flops each pass declares"""
    h.set_option("profile", 2)
    h._lib.gphip_reset_profile(h._h)
    p.eval(Xs, grad=grad)
    import ctypes as C
    ms, launches, flops, nbytes = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    h._lib.gphip_get_profile(h._h, 6, C.byref(ms), C.byref(launches), C.byref(flops), C.byref(nbytes))
    h.set_option("profile", 0)
    return ms.value, launches.value, flops.value


def main():
    from bayesianinference_amd import synthetic as syn
    if "--baseline" in sys.argv:
        return baseline()
    if "--one" in sys.argv:                        # one create and two evaluations with gradients: the pattern to run under a profiler
        n, S, M = (int(v) for v in sys.argv[sys.argv.index("--one") + 1:sys.argv.index("--one") + 4])
        h, _ = fitted(n)
        Xs = syn.make_test_points(M, D)
        with h.sample_paths(S, F, seed=1) as p:
            p.eval(Xs, grad=True)
            p.eval(Xs, grad=True)
        h.close()
        return None
    for n in NS:
        h, _ = fitted(n)
        for S in (64, 512):
            cr, parts = [], {"feature": [], "subst": []}
            for rep in range(REPS + 1):
                t0 = time.perf_counter()
                p = h.sample_paths(S, F, seed=rep)
                cr.append((time.perf_counter() - t0) * 1e3)
                parts["feature"].append(h.get_option("last_paths_feature_us") / 1e3)
                parts["subst"].append(h.get_option("last_paths_subst_us") / 1e3)
                if rep < REPS:
                    p.close()
            emit({"what": "create", "N": n, "S": S, "F": F, **stats(cr[1:]), "feature_ms": round(statistics.median(parts["feature"][1:]), 3),
                  "subst_ms": round(statistics.median(parts["subst"][1:]), 3)})
            for M in (1000, 16384):
                Xs = syn.make_test_points(M, D)
                for grad in (False, True):
                    emit({"what": "eval", "N": n, "S": S, "M": M, "grad": grad, **timed(lambda: p.eval(Xs, grad=grad)),
                          "nsplit_kernel": h.get_option("last_paths_nsplit")})
                    ms, launches, flops = kernel_view(h, p, Xs, grad)
                    emit({"what": "eval kernels (class 6)", "N": n, "S": S, "M": M, "grad": grad, "launches": launches, "ms": round(ms, 3),
                          "declared_gflop": round(flops / 1e9, 2), "of_fp64_mfma_peak": round(flops / (ms * 1e-3) / MFMA_F64_FLOPS, 4) if ms > 0 else None})
                emit({"what": "predict_draws", "N": n, "S": S, "M": M, **timed(lambda: h.predict_draws(Xs, S, seed=1, latent=True, jitter=1e-8), reps=3)})
            if S == 64:
                big = syn.make_test_points(1000000, D)
                emit({"what": "eval", "N": n, "S": S, "M": 1000000, "grad": False, **timed(lambda: p.eval(big), reps=2)})
            p.close()
        h.close()


if __name__ == "__main__":
    main()
