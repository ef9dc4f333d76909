"""Timings of the sparse bound's gradient in the inducing locations (gphip_sparse_bound_grad_inducing), fp64, SE-ARD d = 8, warm,
median of REPS calls (3 at N = 10^6), at (N, m) = (32768, 1024), (32768, 2048), (262144, 2048), (1 000 000, 4096):
gphip_sparse_bound_grad against gphip_sparse_bound_grad_inducing in the same process, the two calls INTERLEAVED (one of each per
repetition), and the library's HIP-event phase "ms_grad_inducing" (the column-wise reductions for dF/dZ) next to "ms_grad_reduce"
(the reductions for dF/dtheta) from one further profiled call.
One JSON line per case; with an argument the lines also go to that file.  SPARSE_TIME_CASES=small keeps to N <= 32768."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
from bayesianinference_amd import _lib, synthetic as syn  # noqa: E402

REPS = 10
PHASES = _lib.SPARSE_PHASES + _lib.SPARSE_GRAD_PHASES + _lib.SPARSE_ZGRAD_PHASES


def interleaved(fa, fb, reps):
    fa()
    fb()
    ta, tb = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fa()
        t1 = time.perf_counter()
        fb()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        tb.append((t2 - t1) * 1e3)
    return statistics.median(ta), statistics.median(tb)


def main():
    small = os.environ.get("SPARSE_TIME_CASES", "") == "small"
    cases = [(32768, 1024), (32768, 2048)] + ([] if small else [(262144, 2048), (1000000, 4096)])
    lines = []
    for n, m in cases:
        X, y = syn.make_dataset(n, 8)
        th = syn.default_theta("se_ard", 8)
        h = _lib.SparseHandle(X, y, X[::n // m][:m], "se_ard")
        reps = REPS if n <= 262144 else 3
        gm, zm = interleaved(lambda: h.bound_grad(th, 1e-8), lambda: h.bound_grad_inducing(th, 1e-8), reps)
        h.set_option("profile", 1)
        F, g, gz, info = h.bound_grad_inducing(th, 1e-8)
        ph = {k: round(h.get_option(k), 3) for k in PHASES}
        h.set_option("profile", 0)
        rec = {"call": "sparse_bound_grad_inducing", "N": n, "m": m, "d": 8, "reps": reps, "bound_grad_ms": round(gm, 3),
               "bound_grad_inducing_ms": round(zm, 3), "inducing_over_grad": round(zm / gm, 3), "info": info,
               "ms_grad_inducing": ph["ms_grad_inducing"], "ms_grad_reduce": ph["ms_grad_reduce"],
               "inducing_over_reduce": round(ph["ms_grad_inducing"] / max(ph["ms_grad_reduce"], 1e-9), 2),
               "inducing_share_of_call": round(ph["ms_grad_inducing"] / zm, 4), "phase_ms": ph,
               "chunk": int(h.get_option("last_sparse_chunk"))}
        h.close()
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
