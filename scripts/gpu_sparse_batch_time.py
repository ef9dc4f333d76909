"""Batched sparse bound against the loop over the one-theta entry point, fp64, SE-ARD d = 8, warm, median of REPS calls.
  * For (N, m) = (8192, 128), (32768, 256), (32768, 1024), (262144, 2048) and B = 8, 32, 128: ONE gphip_sparse_bound_batch call
    of B thetas against B consecutive gphip_sparse_bound calls of the same thetas in the same process (what a batch cost before
    the batched entry point existed).  The two are timed alternately; next to the medians go the loop's own run-to-run spread
    (min and max of its repetitions), the slots of the batch's last group, its chunk and its strips.
  * With option profile = 1: the HIP-event phase split of one B = 32 call at every size.
  * Evaluations per second of the Python nestedSampling on a sparse object at (32768, 256): "LogLikelihoodFunction" as it is
    (one bound_batch per Metropolis step) and replaced by the per-row loop over `bound`.
One JSON line per case; with an argument the lines also go to that file.  SPARSE_BATCH_CASES=small keeps to N <= 32768;
SPARSE_BATCH_REPS sets the repetitions (default 10)."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from bayesianinference_amd import _lib, gaussian_process as gp, nested_sampling as ns, synthetic as syn  # noqa: E402

REPS = int(os.environ.get("SPARSE_BATCH_REPS", "10"))
JITTER = 1e-8


def thetas(B, d, seed=5):
    """B hyper-parameter rows within +-10 % of the timing theta: what one Metropolis step of a sampler hands over"""
    base = syn.default_theta("se_ard", d)
    return base[None, :] * np.random.default_rng(seed).uniform(0.9, 1.1, size=(B, len(base)))


def main():
    small = os.environ.get("SPARSE_BATCH_CASES", "") == "small"
    cases = [(8192, 128), (32768, 256), (32768, 1024)] + ([] if small else [(262144, 2048)])
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for n, m in cases:
        X, y = syn.make_dataset(n, 8)
        h = _lib.SparseHandle(X, y, X[::n // m][:m], "se_ard")
        for B in (8, 32, 128):
            Th = thetas(B, 8)

            def batch():
                F, info = h.bound_batch(Th, JITTER)
                assert np.all(info == 0)
                return F

            def loop():
                return np.array([h.bound(t, JITTER)[0] for t in Th])

            Fb, Fl = batch(), loop()                             # warm: buffers of both routes allocated
            rel = float(np.max(np.abs(Fb - Fl) / np.abs(Fl)))
            tb, tl = [], []
            for _ in range(REPS):
                t0 = time.perf_counter(); batch(); tb.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter(); loop(); tl.append((time.perf_counter() - t0) * 1e3)
            batch()
            rec = {"call": "sparse_bound_batch", "N": n, "m": m, "B": B, "batch_ms": round(statistics.median(tb), 3),
                   "loop_ms": round(statistics.median(tl), 3), "loop_min_ms": round(min(tl), 3), "loop_max_ms": round(max(tl), 3),
                   "batch_min_ms": round(min(tb), 3), "batch_max_ms": round(max(tb), 3), "reps": REPS,
                   "loop_over_batch": round(statistics.median(tl) / statistics.median(tb), 2), "max_rel_diff": rel,
                   "slots": int(h.get_option("last_sparse_slots")), "chunk": int(h.get_option("last_sparse_chunk")),
                   "strips": int(h.get_option("last_sparse_nsplit"))}
            if B == 32:
                h.set_option("profile", 1)
                batch()
                rec["phase_ms"] = {k: round(h.get_option(k), 3) for k in _lib.SPARSE_PHASES}
                h.bound(Th[0], JITTER)
                rec["phase_ms_one_theta"] = {k: round(h.get_option(k), 3) for k in _lib.SPARSE_PHASES}
                h.set_option("profile", 0)
            emit(rec)
        h.close()
    # the Python sampler on a sparse object
    n, m = 32768, 256
    X, y = syn.make_dataset(n, 8)
    variables = [(f"l{k}", 0.5, 2.0) for k in range(8)] + [("sf", 0.5, 2.0), ("sn", 0.05, 0.3)]
    obj = gp.defineSparseGaussianProcess((X, y), "SEARD", X[::n // m][:m], variables=variables, Jitter=JITTER)
    hh = obj["SparseGaussianProcessData"]["HIPHandle"]

    def looped(theta):
        theta = np.asarray(theta, dtype=np.float64)
        f = obj["LogLikelihoodFunction"]
        return np.array([f(t) for t in theta]) if theta.ndim == 2 else f(theta)

    for label, o in (("batched", obj), ("per-row loop", obj.append({"LogLikelihoodFunction": looped}))):
        ns.nestedSampling(o, SamplePoolSize=20, MaxIterations=12, MinIterations=5, Seed=3)          # warm
        t0 = time.perf_counter()
        res = ns.nestedSampling(o, SamplePoolSize=20, MaxIterations=40, MinIterations=10, Seed=3)
        dt = time.perf_counter() - t0
        emit({"call": "nestedSampling (Python) on a sparse object", "N": n, "m": m, "likelihood": label, "seconds": round(dt, 3),
              "evaluations": int(res["LikelihoodEvaluations"]), "evaluations_per_s": round(res["LikelihoodEvaluations"] / dt, 1)})
    hh.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
