"""Sparse-GP timings (gphip_sparse_bound / gphip_sparse_predict), fp64, SE-ARD d = 8, warm, median of REPS calls; the per-phase
times are the library's HIP-event readouts (option profile = 1: K_uu factor, cross build, forward substitution, accumulation,
B factor) of one further call.
  * whole gphip_sparse_bound at (N, m) = (32768, 1024), (32768, 2048), (262144, 2048), (1 000 000, 4096); at N = 32768 also
    gphip_loglik of an ordinary handle in the same process and the ratio;
  * sparse_accumulate_kernel alone: m = 8192, N = 16384 in one chunk, as a fraction of the fp64 MFMA figure on N m (m + 1) flops;
    next to it the whole gphip_predict_cov at N = M = 8192, whose downdate_kernel has the same tile shape (its own time: the
    downdate_kernel row of a `rocprofv3 --kernel-trace --stats` run of this script);
  * gphip_sparse_predict of 10 000 points at m = 4096.
One JSON line per case; with an argument the lines also go to that file.  SPARSE_TIME_CASES=small keeps to N <= 32768."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
from bayesianinference_amd import _lib, synthetic as syn  # noqa: E402

REPS = 10
MFMA_F64_TFLOPS = 78.6                      # the fp64 matrix-pipe figure README.md uses


def timed(f, reps=REPS):
    f()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms), min(ms)


def phases(h, f):
    h.set_option("profile", 1)
    f()
    out = {k: round(h.get_option(k), 3) for k in _lib.SPARSE_PHASES}
    h.set_option("profile", 0)
    return out


def main():
    small = os.environ.get("SPARSE_TIME_CASES", "") == "small"
    cases = [(32768, 1024), (32768, 2048)] + ([] if small else [(262144, 2048), (1000000, 4096)])
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for n, m in cases:
        X, y = syn.make_dataset(n, 8)
        th = syn.default_theta("se_ard", 8)
        h = _lib.SparseHandle(X, y, X[::n // m][:m], "se_ard")
        reps = REPS if n <= 262144 else 5
        med, best = timed(lambda: h.bound(th, 1e-8), reps)
        rec = {"call": "sparse_bound", "N": n, "m": m, "ms": round(med, 3), "min_ms": round(best, 3), "reps": reps,
               "phase_ms": phases(h, lambda: h.bound(th, 1e-8)), "chunk": int(h.get_option("last_sparse_chunk")),
               "strips": int(h.get_option("last_sparse_nsplit")), "gflop": round(2.0 * n * m * m / 1e9, 1)}
        rec["tflops"] = round(rec["gflop"] / med, 2)
        if n == 1000000:
            Xs = syn.make_test_points(10000, 8)
            pm, pb = timed(lambda: h.predict(Xs), 5)
            rec["predict_10000_ms"] = round(pm, 3)
        h.close()
        if n == 32768:
            e = _lib.Handle(X, y, "se_ard")
            em, eb = timed(lambda: e.loglik(th))
            e.close()
            rec["exact_loglik_ms"] = round(em, 3)
            rec["exact_over_sparse"] = round(em / med, 2)
        emit(rec)
    # the accumulation kernel alone
    n, m = 16384, 8192
    X, y = syn.make_dataset(n, 8)
    th = syn.default_theta("se_ard", 8)
    h = _lib.SparseHandle(X, y, X[::n // m][:m], "se_ard")
    h.bound(th, 1e-6)
    acc = [phases(h, lambda: h.bound(th, 1e-6)) for _ in range(5)]
    ms_acc = statistics.median(a["ms_accumulate"] for a in acc)
    flop = float(n) * m * (m + 1)
    emit({"call": "sparse_accumulate_kernel", "N": n, "m": m, "chunk": int(h.get_option("last_sparse_chunk")),
          "strips": int(h.get_option("last_sparse_nsplit")), "ms": round(ms_acc, 3), "tflops": round(flop / ms_acc / 1e9, 2),
          "of_mfma": round(flop / ms_acc / 1e9 / MFMA_F64_TFLOPS, 3), "phase_ms": acc[-1]})
    h.close()
    X, y = syn.make_dataset(8192, 8)
    e = _lib.Handle(X, y, "se_ard")
    assert e.fit(th) == 0
    Xs = syn.make_test_points(8192, 8)
    jm, jb = timed(lambda: e.predict_cov(Xs), 3)
    emit({"call": "predict_cov", "N": 8192, "M": 8192, "ms": round(jm, 3), "downdate_gflop": round(8192.0 * 8193 * 8192 / 1e9, 1),
          "downdate_strips": int(e.get_option("last_joint_nsplit"))})
    e.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
