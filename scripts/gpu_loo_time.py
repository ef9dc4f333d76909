"""Leave-one-out timings next to the calls they share their device work with: gphip_loglik, gphip_loglik_grad, gphip_loo,
gphip_loo_grad at N = 2048, 8192, 32768 (fp64, SE-ARD, d = 8), one handle per size, same process.  Every call returns host
data, so it ends device-synchronised: the whole-call figure is the host clock around it, warm, median of REPS calls, the four
calls interleaved.  A second pass with option profile = 2 reads the library's HIP-event time per kernel class; "trsm" holds
the panel solves, the inverse launch (U = L^-T) and the U U^T / B B^T products, so
    M product = trsm(loo_grad) - trsm(loglik_grad)          U U^T = trsm(loglik_grad) - trsm(loo)
each next to the flops its tiles execute (M: the full contraction length; U U^T: k >= 128 ti for tile row ti).  One JSON line per size; with an argument the lines also go to that file."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from bayesianinference_amd import _lib, synthetic as syn  # noqa: E402

REPS = 10
MFMA_F64_TFLOPS = 78.6                      # the fp64 matrix-pipe figure README.md uses


def main():
    sizes = [int(v) for v in os.environ.get("LOO_TIME_SIZES", "2048,8192,32768").split(",")]
    lines = []
    for n in sizes:
        X, y = syn.make_dataset(n, 8)
        th = syn.default_theta("se_ard", 8)
        h = _lib.Handle(X, y, "se_ard")
        calls = {"loglik": lambda: h.loglik(th), "loglik_grad": lambda: h.loglik_grad(th),
                 "loo": lambda: h.loo(th, mean=False, var=False, logp=False), "loo_grad": lambda: h.loo_grad(th)}
        for f in calls.values():
            f()
        ms = {k: [] for k in calls}
        for _ in range(REPS):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                ms[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: statistics.median(v) for k, v in ms.items()}
        h.set_option("profile", 2)
        prof = {}
        for k, f in calls.items():
            h.reset_profile()
            f()
            prof[k] = h.profile()
        h.set_option("profile", 0)
        trsm = {k: prof[k]["trsm"]["ms"] for k in calls}
        npad = -(-n // 128) * 128
        tiles = (npad // 128) * (npad // 128 + 1) // 2
        m_flop = 2.0 * 128 * 128 * npad * tiles                     # full contraction length
        m_ms, uut_ms = trsm["loo_grad"] - trsm["loglik_grad"], trsm["loglik_grad"] - trsm["loo"]
        nt = npad // 128                                              # tile (ti, tj <= ti) of U U^T contracts k >= 128 ti only
        uut_flop = 2.0 * 128 ** 3 * nt * (nt + 1) * (nt + 2) / 6
        rec = {"N": n, "ms": {k: round(v, 3) for k, v in med.items()},
               "min_ms": {k: round(min(v), 3) for k, v in ms.items()},
               "loo_over_loglik_grad": round(med["loo"] / med["loglik_grad"], 3),
               "loo_grad_over_loglik_grad": round(med["loo_grad"] / med["loglik_grad"], 3),
               "class_ms": {k: {c: round(v["ms"], 3) for c, v in prof[k].items() if v["ms"] > 0} for k in calls},
               "m_product_ms": round(m_ms, 3), "m_product_tflops": round(m_flop / m_ms / 1e9, 1) if m_ms > 0 else None,
               "m_product_of_mfma": round(m_flop / m_ms / 1e9 / MFMA_F64_TFLOPS, 3) if m_ms > 0 else None,
               "uut_ms": round(uut_ms, 3), "uut_tflops": round(uut_flop / uut_ms / 1e9, 1) if uut_ms > 0 else None,
               "uut_of_mfma": round(uut_flop / uut_ms / 1e9 / MFMA_F64_TFLOPS, 3) if uut_ms > 0 else None}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        h.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
