"""Timings of the sparse bound's analytic gradient (gphip_sparse_bound_grad), fp64, SE-ARD d = 8 (p = 10), warm, median of REPS
calls; the per-phase times are the library's HIP-event readouts (option profile = 1) of one further call.
  * (N, m) = (32768, 1024), (32768, 2048), (262144, 2048), (1 000 000, 4096): gphip_sparse_bound_grad against gphip_sparse_bound
    in the same process and against the difference quotient it replaces, 2 p + 1 = 21 calls of gphip_sparse_bound, timed as such
    (median of QREPS rounds of 21 calls);
  * sparse_weight_kernel alone ("ms_grad_weights" times nothing else): m = 8192, one chunk of 16384 points, as a fraction of
    the fp64 MFMA figure on 2 N m^2 flops.
One JSON line per case; with an argument the lines also go to that file.  SPARSE_TIME_CASES=small keeps to N <= 32768."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
from bayesianinference_amd import _lib, synthetic as syn  # noqa: E402

REPS = 10
QREPS = 3
MFMA_F64_TFLOPS = 78.6                      # the fp64 matrix-pipe figure README.md uses
PHASES = _lib.SPARSE_PHASES + _lib.SPARSE_GRAD_PHASES


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
    out = {k: round(h.get_option(k), 3) for k in PHASES}
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
        reps = REPS if n <= 262144 else 3
        bm, _ = timed(lambda: h.bound(th, 1e-8), reps)
        gm, gb = timed(lambda: h.bound_grad(th, 1e-8), reps)
        nq = 2 * len(th) + 1
        qm, _ = timed(lambda: [h.bound(th, 1e-8) for _ in range(nq)], QREPS if n <= 262144 else 1)
        F, g, info = h.bound_grad(th, 1e-8)
        rec = {"call": "sparse_bound_grad", "N": n, "m": m, "p": len(th), "ms": round(gm, 3), "min_ms": round(gb, 3), "reps": reps,
               "bound_ms": round(bm, 3), "grad_over_bound": round(gm / bm, 2), "quotient_ms": round(qm, 1),
               "quotient_over_grad": round(qm / gm, 1), "info": info, "analytic": int(h.get_option("grad_analytic")),
               "phase_ms": phases(h, lambda: h.bound_grad(th, 1e-8)), "chunk": int(h.get_option("last_sparse_chunk"))}
        h.close()
        emit(rec)
    # the weight kernel alone
    n, m = 16384, 8192
    X, y = syn.make_dataset(n, 8)
    th = syn.default_theta("se_ard", 8)
    h = _lib.SparseHandle(X, y, X[::n // m][:m], "se_ard")
    h.bound_grad(th, 1e-6)
    runs = [phases(h, lambda: h.bound_grad(th, 1e-6)) for _ in range(3)]
    ms_w = statistics.median(a["ms_grad_weights"] for a in runs)
    flop = 2.0 * n * m * m
    emit({"call": "sparse_weight_kernel", "N": n, "m": m, "chunk": int(h.get_option("last_sparse_chunk")), "ms": round(ms_w, 3),
          "tflops": round(flop / ms_w / 1e9, 2), "of_mfma": round(flop / ms_w / 1e9 / MFMA_F64_TFLOPS, 3), "phase_ms": runs[-1]})
    h.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
