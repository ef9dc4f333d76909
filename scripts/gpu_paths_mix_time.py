"""Times the mixture paths object (gphip_paths_create_samples) against the loop route it replaces on a sampled object: one fit +
one paths object per distinct theta, one device call per paths object and evaluation.  Both routes run in this process,
alternating, after a warm-up of every shape; medians, minima and maxima of the repeats are printed as one JSON line each
(the spread of the loop route is the yardstick of a difference).

    python scripts/gpu_paths_mix_time.py [--n 512,2048,8192] [--rows 8,64] [--reps 5] > profiles/paths_mix_time.txt

fp64, SE-ARD with a constant mean, d = 8, F = 1024 features, n = 64 draws dealt evenly over R distinct thetas.
  (a) creation        the loop of fit + sample_paths against one sample_paths_samples
  (b) ascent step     4 starts per draw with gradients: the sum of the parts' eval_own calls against one call
  (c) Thompson        thompsonSampleFromGaussianProcess with its defaults, Batched off and on, on an object of R equally weighted
                      samples (the draws pick the thetas at random: the distinct thetas used are printed)
Needs a GPU: without one the handle cannot be created and the script fails."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from bayesianinference_amd import _lib, gaussian_process as gp, synthetic as syn      # noqa: E402

D, F, DRAWS, STARTS = 8, 1024, 64, 4


def thetas(R):
    ell = np.linspace(0.8, 1.3, D)
    return np.array([list(ell * f) + [1.1, 0.15, 0.2] for f in np.linspace(0.8, 1.25, R)])


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": round(float(np.median(ts)), 3), "min_ms": round(float(ts.min()), 3), "max_ms": round(float(ts.max()), 3)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()                                                    # (every call ends in a device synchronise: the results are on the host)
    return time.perf_counter() - t0, out


def loop_create(h, th, counts, seeds):
    parts = []
    for r in range(len(th)):
        assert h.fit(th[r]) == 0
        parts.append(h.sample_paths(int(counts[r]), F, int(seeds[r])))
    return parts


def one_shape(N, R, reps):
    X, y = syn.make_dataset(N, D)
    th, counts, seeds = thetas(R), np.full(R, DRAWS // R), np.arange(1, R + 1)
    start = np.concatenate([[0], np.cumsum(counts)])
    P = syn.make_test_points(DRAWS * STARTS, D).reshape(DRAWS, STARTS, D)
    h = _lib.Handle(X, y, "se_ard", "const")
    base = {"N": N, "R": R, "draws": DRAWS, "F": F, "d": D}
    # (a) creation, alternating; the first round is the warm-up
    tl, tm = [], []
    for it in range(reps + 1):
        dt, parts = timed(lambda: loop_create(h, th, counts, seeds))
        for p in parts:
            p.close()
        dm, mix = timed(lambda: h.sample_paths_samples(th, counts, seeds, F))
        assert np.all(mix.info == 0)
        groups = h.get_option("last_paths_mix_groups")
        mix.close()
        if it:
            tl.append(dt)
            tm.append(dm)
    print(json.dumps({"what": "(a) creation", **base, "loop": stats(tl), "one_call": stats(tm), "groups": groups}), flush=True)
    # (b) one ascent step: 4 starts per draw, values and gradients
    parts = loop_create(h, th, counts, seeds)
    mix = h.sample_paths_samples(th, counts, seeds, F)
    tl, tm = [], []
    for it in range(4 * reps + 2):
        dt, lo = timed(lambda: [p.eval_own(P[start[r]:start[r + 1]], grad=True) for r, p in enumerate(parts)])
        dm, mo = timed(lambda: mix.eval_own(P, grad=True))
        if it >= 2:
            tl.append(dt)
            tm.append(dm)
    err = max(float(np.abs(np.concatenate([o[k] for o in lo]) - mo[k]).max() / np.abs(mo[k]).max()) for k in (0, 1))
    print(json.dumps({"what": "(b) ascent step, %d starts per draw, with gradients" % STARTS, **base, "loop": stats(tl), "one_call": stats(tm),
                      "max_rel_difference": err}), flush=True)
    for p in parts:
        p.close()
    mix.close()
    h.close()
    # (c) Thompson sampling with the defaults on an object of R equally weighted samples
    names = [("l%d" % k, 0.05, 5.0) for k in range(D)] + [("sf", 0.1, 5.0), ("sn", 0.01, 1.0), ("mu", -1.0, 1.0)]
    obj = gp.defineGaussianProcess((X, y[:, None]), "se_ard", meanFunction="Constant", variables=names)
    obj = obj.append({"Samples": [{"Point": th[r], "CrudePosteriorWeight": 1.0 / R} for r in range(R)]})
    box = np.stack([X.min(axis=0), X.max(axis=0)], axis=1)
    tl, tm, used = [], [], 0
    for it in range(max(reps // 2, 2) + 1):
        dt, a = timed(lambda: gp.thompsonSampleFromGaussianProcess(obj, DRAWS, box, Features=F, seed=7))
        dm, b = timed(lambda: gp.thompsonSampleFromGaussianProcess(obj, DRAWS, box, Features=F, seed=7, Batched=True))
        used = len(np.unique(a["sample"]))
        assert np.array_equal(a["sample"], b["sample"])
        if it:
            tl.append(dt)
            tm.append(dm)
    print(json.dumps({"what": "(c) thompsonSampleFromGaussianProcess, defaults", **base, "distinct_thetas_used": used, "loop": stats(tl),
                      "one_call": stats(tm), "max_abs_difference_of_f": float(np.abs(a["f"] - b["f"]).max())}), flush=True)
    obj["GaussianProcessData"]["HIPHandle"].close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="512,2048,8192")
    ap.add_argument("--rows", default="8,64")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for N in [int(v) for v in a.n.split(",")]:
        for R in [int(v) for v in a.rows.split(",")]:
            one_shape(N, R, a.reps)


if __name__ == "__main__":
    main()
