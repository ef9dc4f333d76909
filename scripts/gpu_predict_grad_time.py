"""Gradients of the prediction in the test inputs (gphip_predict_grad / gphip_sparse_predict_grad) against what they replace, fp64,
SE-ARD d = 8, warm, median of REPS calls with their min and max; the variants of one size are timed alternately in one process.
  * Exact object at (N, M) = (8192, 100), (32768, 1000), (32768, 10000); sparse object at (N, m, M) = (32768, 1024, 1000),
    (262144, 2048, 10000).
  * Per size: predict_grad with and without dvar; predict of this build; the 2 d-call difference quotient predict_grad replaces
    (2 d calls of predict at shifted points, QUOT_REPS repetitions); with option profile = 1 the share of the reduction kernel
    (exact: profile class 6 of a predict_grad call minus that of a predict call; sparse: ms_pgrad_reduce next to
    ms_pgrad_backward), and for the sparse object predict_grad with option sparse_pgrad_refine = 0.
  * --parent-lib PATH: a library built from the parent commit.  predict alone is timed at the same sizes in fresh child processes,
    parent build (GPHIP_LIB), this build, parent, this: the two runs of each build show the run-to-run spread the comparison has
    to be read against.
One JSON line per size; with --out FILE the lines also go to that file.
PGRAD_CASES=small keeps to the first size of each object; PGRAD_REPS sets the repetitions (default 7)."""
import json
import os
import statistics
import subprocess
import sys
import time


sys.path.insert(0, os.getcwd())

REPS = int(os.environ.get("PGRAD_REPS", "7"))
QUOT_REPS = 3
D = 8
JITTER = 1e-8
EXACT = [(8192, 100), (32768, 1000), (32768, 10000)]
SPARSE = [(32768, 1024, 1000), (262144, 2048, 10000)]


def stats(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def timed(variants, reps):
    """{name: fn} -> {name: [ms]}: every variant once per repetition, in turn, after one warm call of each (every call ends in
    the library's own stream synchronisation: its results are on the host when it returns)"""
    for fn in variants.values():
        fn()
    ts = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return ts


def make(case):
    from bayesianinference_amd import _lib, synthetic as syn
    th = syn.default_theta("se_ard", D)
    if len(case) == 2:
        n, M = case
        X, y = syn.make_dataset(n, D)
        h = _lib.Handle(X, y, "se_ard")
        assert h.fit(th) == 0
    else:
        n, m, M = case
        X, y = syn.make_dataset(n, D)
        h = _lib.SparseHandle(X, y, X[::n // m][:m], "se_ard")
        assert h.fit(th, JITTER) == 0
    return h, syn.make_test_points(M, D)


def predict_only(case):
    h, Xs = make(case)
    ts = timed({"predict": lambda: h.predict(Xs)}, REPS)
    h.close()
    return stats(ts["predict"])


def measure(case, parent_lib):
    from bayesianinference_amd import _lib
    h, Xs = make(case)
    sparse = len(case) == 3
    step = 1e-4

    def quotient():
        for c in range(D):
            for s in (step, -step):
                P = Xs.copy()
                P[:, c] += s
                h.predict(P)
    variants = {"predict": lambda: h.predict(Xs), "predict_grad": lambda: h.predict_grad(Xs),
                "predict_grad_no_dvar": lambda: h.predict_grad(Xs, variance=False)}
    if sparse:
        def unrefined():
            h.set_option("sparse_pgrad_refine", 0)
            h.predict_grad(Xs)
            h.set_option("sparse_pgrad_refine", 1)
        variants["predict_grad_unrefined"] = unrefined
    ts = timed(variants, REPS)
    rec = {"object": "sparse" if sparse else "exact", "N": case[0], "M": case[-1], "d": D, "reps": REPS, **({"m": case[1]} if sparse else {}),
           **{k: stats(v) for k, v in ts.items()}}
    rec["difference_quotient_2d_calls"] = stats(timed({"q": quotient}, QUOT_REPS)["q"])
    # the reduction kernel's share of a call with dvar, by HIP events
    h.set_option("profile", 1)
    if sparse:
        h.predict_grad(Xs)
        ph = {k: round(h.get_option(k), 3) for k in _lib.SPARSE_SAMPLES_PHASES + _lib.SPARSE_PGRAD_PHASES}
        rec["phase_ms"] = ph
        rec["reduce_kernel_ms"] = ph["ms_pgrad_reduce"]
    else:
        cls6 = _lib.PROFILE_CLASSES.index("predict_epilogue")

        def class6(fn):
            h._lib.gphip_reset_profile(h._h)
            fn()
            import ctypes as C
            ms = C.c_double(0.0)
            h._lib.gphip_get_profile(h._h, cls6, C.byref(ms), None, None, None)
            return ms.value
        rec["reduce_kernel_ms"] = round(class6(lambda: h.predict_grad(Xs)) - class6(lambda: h.predict(Xs)), 3)
    h.set_option("profile", 0)
    rec["reduce_share_of_predict_grad"] = round(rec["reduce_kernel_ms"] / rec["predict_grad"]["median_ms"], 4)
    rec["strips"] = int(h.get_option("last_predict_grad_nsplit"))
    rec["chunk"] = int(h.get_option("last_predict_grad_chunk"))
    h.close()
    if parent_lib:                             # the same protocol for both builds: predict alone in a fresh process, alternating
        def child(lib):
            env = dict(os.environ)
            if lib:
                env["GPHIP_LIB"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(case)], env=env, capture_output=True,
                                 text=True, timeout=900)
            if out.returncode != 0:
                raise RuntimeError("a predict-only child failed:\n" + out.stdout + out.stderr)
            return json.loads(out.stdout.strip().splitlines()[-1])
        rec["predict_alone_parent"] = [child(parent_lib)]
        rec["predict_alone_this"] = [child(None)]
        rec["predict_alone_parent"].append(child(parent_lib))
        rec["predict_alone_this"].append(child(None))
        med = lambda rs: statistics.mean(r["median_ms"] for r in rs)                 # noqa: E731
        rec["predict_over_parent"] = round(med(rec["predict_alone_this"]) / med(rec["predict_alone_parent"]), 3)
    rec["grad_over_predict"] = round(rec["predict_grad"]["median_ms"] / rec["predict"]["median_ms"], 3)
    rec["grad_no_dvar_over_predict"] = round(rec["predict_grad_no_dvar"]["median_ms"] / rec["predict"]["median_ms"], 3)
    rec["quotient_over_grad"] = round(rec["difference_quotient_2d_calls"]["median_ms"] / rec["predict_grad"]["median_ms"], 2)
    return rec


def main():
    args = sys.argv[1:]
    if args[:1] == ["--child"]:
        print(json.dumps(predict_only(tuple(json.loads(args[1])))), flush=True)
        return
    parent = args[args.index("--parent-lib") + 1] if "--parent-lib" in args else None
    out = args[args.index("--out") + 1] if "--out" in args else None
    small = os.environ.get("PGRAD_CASES", "") == "small"
    lines = []
    for case in (EXACT[:1] + SPARSE[:1]) if small else (EXACT + SPARSE):
        rec = measure(case, os.path.abspath(parent) if parent else None)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        if out:                                # (after every size: what has been measured survives a later failure)
            with open(out, "w") as f:
                for r in lines:
                    f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
