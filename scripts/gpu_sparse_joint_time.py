"""Timings of the sparse object's joint predictive distribution (gphip_sparse_predict_cov / _logpdf / _draws), fp64, SE-ARD d = 8,
warm, median of REPS calls; the per-phase times are the library's HIP-event readouts (option profile = 1: "ms_joint_v" V1 and V2,
"ms_joint_build" K(X*, X*), "ms_joint_downdate" the two-segment downdate, "ms_joint_factor" the factorisation of Sigma) of one
further gphip_sparse_predict_logpdf call.
  * (N, m, M) = (32768, 1024, 1000), (262144, 2048, 8192), (1 000 000, 4096, 8192): the three calls, next to gphip_sparse_predict
    of the same M points; at N = 32768 also gphip_predict_cov of an ordinary handle with the same M in the same process;
  * the two-segment downdate_kernel alone (M = 8192: 2144 output tiles, one strip, so the event pair times one launch) as a
    fraction of the fp64 MFMA figure on M (M + 1) 2 m flops at m = 2048 and at m = 128, where the contraction is four stages long.
One JSON line per case; with an argument the lines also go to that file.  SPARSE_JOINT_TIME_CASES=small keeps to N <= 32768."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
from bayesianinference_amd import _lib, synthetic as syn  # noqa: E402

REPS = 10
MFMA_F64_TFLOPS = 78.6                      # the fp64 matrix-pipe figure README.md uses
JITTER = 1e-8


def timed(f, reps=REPS):
    f()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ms), 3), round(min(ms), 3)


def phases(h, f):
    h.set_option("profile", 1)
    f()
    out = {k: round(h.get_option(k), 3) for k in _lib.SPARSE_JOINT_PHASES}
    h.set_option("profile", 0)
    return out


def downdate_fraction(h, Xs, ys, m, M):
    """the downdate phase of five profiled calls: median ms and its share of the fp64 MFMA figure on M (M + 1) 2 m flops"""
    ms = statistics.median(phases(h, lambda: h.predict_logpdf(Xs, ys))["ms_joint_downdate"] for _ in range(5))
    gflop = M * (M + 1.0) * 2.0 * m / 1e9
    return {"downdate_ms": round(ms, 3), "gflop": round(gflop, 1), "tflops": round(gflop / ms, 2),
            "fraction_of_mfma_f64": round(gflop / ms / MFMA_F64_TFLOPS, 3), "strips": int(h.get_option("last_sparse_joint_nsplit"))}


def main():
    small = os.environ.get("SPARSE_JOINT_TIME_CASES", "") == "small"
    cases = [(32768, 1024, 1000)] + ([] if small else [(262144, 2048, 8192), (1000000, 4096, 8192)])
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    th = syn.default_theta("se_ard", 8)
    for n, m, M in cases:
        X, y = syn.make_dataset(n, 8)
        Xs = syn.make_test_points(M, 8)
        ys = syn.make_outputs(Xs)
        h = _lib.SparseHandle(X, y, X[::n // m][:m], "se_ard")
        assert h.fit(th, JITTER) == 0
        rec = {"call": "sparse_joint", "N": n, "m": m, "M": M, "reps": REPS}
        rec["predict_cov_ms"], _ = timed(lambda: h.predict_cov(Xs))
        rec["predict_logpdf_ms"], _ = timed(lambda: h.predict_logpdf(Xs, ys))
        rec["predict_draws16_ms"], _ = timed(lambda: h.predict_draws(Xs, 16, seed=1))
        rec["sparse_predict_ms"], _ = timed(lambda: h.predict(Xs))
        rec["phase_ms"] = phases(h, lambda: h.predict_logpdf(Xs, ys))
        rec["strips"] = int(h.get_option("last_sparse_joint_nsplit"))
        if (m, M) == (2048, 8192):
            rec["downdate"] = downdate_fraction(h, Xs, ys, m, M)
        h.close()
        if n == 32768:
            e = _lib.Handle(X, y, "se_ard")
            assert e.fit(th) == 0
            rec["exact_predict_cov_ms"], _ = timed(lambda: e.predict_cov(Xs))
            e.close()
        emit(rec)
    # the short contraction: m = 128, four stages of the pipeline per segment
    n, m, M = 32768, 128, 8192
    X, y = syn.make_dataset(n, 8)
    Xs = syn.make_test_points(M, 8)
    ys = syn.make_outputs(Xs)
    h = _lib.SparseHandle(X, y, X[::n // m][:m], "se_ard")
    assert h.fit(th, JITTER) == 0
    h.predict_logpdf(Xs, ys)
    rec = {"call": "sparse_joint_downdate", "N": n, "m": m, "M": M}
    rec.update(downdate_fraction(h, Xs, ys, m, M))
    if small:                                   # (the long contraction is otherwise taken from the (262144, 2048, 8192) case)
        h.close()
        m = 2048
        h = _lib.SparseHandle(X, y, X[::n // m][:m], "se_ard")
        assert h.fit(th, JITTER) == 0
        h.predict_logpdf(Xs, ys)
        emit({"call": "sparse_joint_downdate", "N": n, "m": m, "M": M, **downdate_fraction(h, Xs, ys, m, M)})
    h.close()
    emit(rec)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
