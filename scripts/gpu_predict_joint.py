"""Joint prediction timings (gphip_predict_cov / gphip_predict_draws), fp64, SE-ARD d = 8: wall time per call after a warm-up
call (every call returns host data, so it ends device-synchronised), the downdate's strip count, and -- with the library's
profile option -- the time the child context's downdate launch took.  One JSON line per case; with an argument, the lines
also go to that file.  The downdate kernel's own time is best read from a `rocprofv3 --kernel-trace --stats` run of this
script (downdate_kernel / strip_reduce_kernel rows)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from bayesianinference_amd import _lib, synthetic as syn  # noqa: E402

REPS = 3
CASES = [("cov", 32768, 1000, 0), ("cov", 8192, 8192, 0), ("draws", 8192, 4096, 1000)]


def main():
    lines = []
    for kind, n, m, s in CASES:
        X, y = syn.make_dataset(n, 8)
        th = syn.default_theta("se_ard", 8)
        h = _lib.Handle(X, y, "se_ard")
        assert h.fit(th) == 0
        Xs = syn.make_test_points(m, 8)
        call = (lambda: h.predict_cov(Xs)) if kind == "cov" else (lambda: h.predict_draws(Xs, s, seed=1))
        call()
        t0 = time.perf_counter()
        for _ in range(REPS):
            call()
        ms = (time.perf_counter() - t0) / REPS * 1e3
        t0 = time.perf_counter()
        for _ in range(REPS):
            h.predict(Xs)
        ms_marg = (time.perf_counter() - t0) / REPS * 1e3
        rec = {"call": f"predict_{kind}", "N": n, "M": m, "S": s, "ms_per_call": round(ms, 3),
               "predict_marginals_ms": round(ms_marg, 3), "downdate_strips": int(h.get_option("last_joint_nsplit")),
               "downdate_gflop": round(m * (m + 1) * n / 1e9, 2)}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        h.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
