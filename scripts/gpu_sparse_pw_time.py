"""Sparse bound with point-dependent noise and mean (gphip_sparse_bound_pw / _bound_batch_pw) against the constant calls, fp64,
SE-ARD d = 8, warm, median of REPS calls with their min and max (the protocol of gpu_sparse_batch_time.py: the variants of one size
are timed alternately in one process).
  * One theta at (N, m) = (32768, 256), (32768, 2048), (262144, 2048): gphip_sparse_bound, gphip_sparse_bound_pw with option
    sparse_pw_fused = 1 (the weight inside the contraction) and = 0 (sparse_scale_rows_kernel + the unweighted contraction); with
    option profile = 1 the accumulation phase alone (ms_accumulate) of one call of each.
  * A batch of 32 thetas at (8192, 128) and (32768, 1024): gphip_sparse_bound_batch and the two forms of gphip_sparse_bound_batch_pw.
  * fused_over_const / unfused_over_const: the cost of the weights as ratios of medians; fused_over_unfused decides the default.
The constant calls are what a library built from another commit is compared on: with GPHIP_LIB pointing at a build that has no
_pw entry points only they are timed (SPARSE_PW_BUILD names the build in the records, default "this commit").  One JSON line
per case; with an argument the lines also go to that file.
SPARSE_PW_CASES=small keeps to N <= 32768; SPARSE_PW_REPS sets the repetitions (default 10)."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from bayesianinference_amd import _lib, synthetic as syn  # noqa: E402

REPS = int(os.environ.get("SPARSE_PW_REPS", "10"))
JITTER = 1e-8


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def arrays(X, rows):
    """nu = sn^2 2^(2 sin 3 x_1), m = 0.2 + 0.3 x_1 for every row of thetas (sn: the last entry of an SE-ARD theta without mean)"""
    s = 4.0 ** np.sin(3.0 * X[:, 0])
    return (np.ascontiguousarray(np.tile(0.2 + 0.3 * X[:, 0], (len(rows), 1))),
            np.ascontiguousarray(np.array([r[-1] ** 2 * s for r in rows])))


def timed(variants):
    """{name: fn} -> {name: [ms]}: every variant once per repetition, in turn, after one warm call of each"""
    for fn in variants.values():
        fn()
    ts = {k: [] for k in variants}
    for _ in range(REPS):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    has_pw = hasattr(_lib.load(), "gphip_sparse_bound_pw")
    small = os.environ.get("SPARSE_PW_CASES", "") == "small"
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def variants_of(h, const, pw_call):
        v = {"const": const}
        if has_pw:
            def fused():
                h.set_option("sparse_pw_fused", 1)
                pw_call()

            def unfused():
                h.set_option("sparse_pw_fused", 0)
                pw_call()
            v.update(pw_fused=fused, pw_unfused=unfused)
        return v

    def record(call, n, m, h, variants, extra):
        ts = timed(variants)
        rec = {"build": os.environ.get("SPARSE_PW_BUILD", "this commit"), "call": call, "N": n, "m": m, "reps": REPS, **extra,
               **{k: stats(v) for k, v in ts.items()}}
        h.set_option("profile", 1)
        for k, fn in variants.items():
            fn()
            rec[k]["ms_accumulate"] = round(h.get_option("ms_accumulate"), 3)
        h.set_option("profile", 0)
        if has_pw:
            rec["fused_over_const"] = round(rec["pw_fused"]["median_ms"] / rec["const"]["median_ms"], 3)
            rec["unfused_over_const"] = round(rec["pw_unfused"]["median_ms"] / rec["const"]["median_ms"], 3)
            rec["fused_over_unfused"] = round(rec["pw_fused"]["median_ms"] / rec["pw_unfused"]["median_ms"], 3)
        rec.update(chunk=int(h.get_option("last_sparse_chunk")), strips=int(h.get_option("last_sparse_nsplit")))
        emit(rec)

    base = syn.default_theta("se_ard", 8)
    for n, m in [(32768, 256), (32768, 2048)] + ([] if small else [(262144, 2048)]):
        X, y = syn.make_dataset(n, 8)
        h = _lib.SparseHandle(X, y, X[::n // m][:m], "se_ard")
        mean, nug = arrays(X, base[None, :])

        def const():
            assert h.bound(base, JITTER)[1] == 0

        def pw_call():
            assert h.bound_pw(base, JITTER, mean, nug)[1] == 0
        record("sparse_bound", n, m, h, variants_of(h, const, pw_call), {})
        h.close()
    for n, m in [(8192, 128), (32768, 1024)]:
        X, y = syn.make_dataset(n, 8)
        h = _lib.SparseHandle(X, y, X[::n // m][:m], "se_ard")
        Th = base[None, :] * np.random.default_rng(5).uniform(0.9, 1.1, size=(32, len(base)))
        mean, nug = arrays(X, Th)

        def const():
            assert np.all(h.bound_batch(Th, JITTER)[1] == 0)

        def pw_call():
            assert np.all(h.bound_batch_pw(Th, JITTER, mean, nug)[1] == 0)
        record("sparse_bound_batch", n, m, h, variants_of(h, const, pw_call), {"B": 32})
        h.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
