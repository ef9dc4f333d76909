"""Sparse prediction over posterior samples: ONE gphip_sparse_predict_samples call against the loop of gphip_sparse_fit +
gphip_sparse_predict per sample that predictFromSparseGaussianProcess ran before the call existed.  fp64, SE-ARD d = 8, warm,
median of REPS calls with min - max, the routes alternated in one process (the protocol of scripts/gpu_sparse_batch_time.py).
  * Sizes (N, m, S, M): (8192, 128, 256, 1000), (32768, 256, 256, 1000), (32768, 1024, 64, 1000), (262144, 2048, 32, 1000),
    (32768, 1024, 64, 10000).
  * The batched call twice: with sparse_handover_kernel (option "sparse_samples_handover" = 1, the default) and with the
    device-to-device copy plus norm launch it replaces (= 0), the two swapping places from repetition to repetition; next to
    the whole calls, the HIP-event time of that phase alone.
  * With option profile = 1: the phase split of one batched call per size.
One JSON line per case; with an argument the lines also go to that file.  SPARSE_SAMPLES_CASES=small keeps to N <= 32768;
SPARSE_SAMPLES_REPS sets the repetitions (default 10)."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
from bayesianinference_amd import _lib, synthetic as syn  # noqa: E402

REPS = int(os.environ.get("SPARSE_SAMPLES_REPS", "10"))
JITTER = 1e-8
CASES = [(8192, 128, 256, 1000), (32768, 256, 256, 1000), (32768, 1024, 64, 1000), (262144, 2048, 32, 1000), (32768, 1024, 64, 10000)]


def thetas(S, d, seed=5):
    """S hyper-parameter rows within +-10 % of the timing theta: what the tail of a nested-sampling run leaves"""
    base = syn.default_theta("se_ard", d)
    return base[None, :] * np.random.default_rng(seed).uniform(0.9, 1.1, size=(S, len(base)))


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    small = os.environ.get("SPARSE_SAMPLES_CASES", "") == "small"
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    data = {}
    for n, m, S, M in CASES:
        if small and n > 32768:
            continue
        if n not in data:
            data = {n: syn.make_dataset(n, 8)}
        X, y = data[n]
        h = _lib.SparseHandle(X, y, X[::n // m][:m], "se_ard")
        Th, Xs = thetas(S, 8), syn.make_test_points(M, 8)

        def batched(handover):
            h.set_option("sparse_samples_handover", handover)
            mu, var, info = h.predict_samples(Th, Xs, JITTER)
            assert np.all(info == 0)
            return mu, var

        def loop():
            h.set_option("sparse_samples_handover", 1)          # (the one-theta call runs the same pass and reads the option too)
            mu, var = np.empty((S, M)), np.empty((S, M))
            for s, th in enumerate(Th):
                assert h.fit(th, JITTER) == 0
                mu[s], var[s] = h.predict(Xs)
            return mu, var

        (mb, vb), (mc, vc), (ml, vl) = batched(1), batched(0), loop()            # warm: buffers of every route allocated
        scale_m, scale_v = np.abs(y).max(), (Th[:, 8] ** 2)[:, None]
        t1, t0_, tl = [], [], []
        for rep in range(REPS):                                  # (the two batched forms swap places from repetition to repetition:
            for handover in ((1, 0) if rep % 2 == 0 else (0, 1)):   #  whichever follows the loop pays for what the loop left behind)
                t = time.perf_counter(); batched(handover); (t1 if handover else t0_).append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter(); loop(); tl.append((time.perf_counter() - t) * 1e3)
        rec = {"call": "sparse_predict_samples", "N": n, "m": m, "S": S, "M": M, "reps": REPS, "batched": stats(t1),
               "batched_copy_plus_norm": stats(t0_), "loop_fit_predict": stats(tl),
               "loop_over_batched": round(statistics.median(tl) / statistics.median(t1), 2),
               "max_diff_mean_over_ymax": float(np.abs(mb - ml).max() / scale_m), "max_diff_var_over_sf2": float((np.abs(vb - vl) / scale_v).max()),
               "handover_forms_same_bytes": bool(np.array_equal(mb, mc) and np.array_equal(vb, vc))}
        h.set_option("profile", 1)
        for handover, key in ((1, "phase_ms"), (0, "phase_ms_copy_plus_norm")):
            batched(handover)
            rec[key] = {k: round(h.get_option(k), 3) for k in _lib.SPARSE_PHASES + _lib.SPARSE_SAMPLES_PHASES}
        h.set_option("profile", 0)
        h.set_option("sparse_samples_handover", 1)
        rec.update({"slots": int(h.get_option("last_sparse_slots")), "chunk": int(h.get_option("last_sparse_chunk")),
                    "samples_chunk": int(h.get_option("last_sparse_samples_chunk"))})
        emit(rec)
        h.close()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
