"""Timing of gphip_loglik_grad_batch next to the loop it replaces, fp64 SE-ARD, d = 8, p = 10.

  * For (N, B) = (512, 21), (2048, 21), (4096, 8), (8192, 4) and (1024, 300) -- more rows than a context gives slots, so the
    group rule has to split (256 + 44): ONE gphip_loglik_grad_batch call against B consecutive gphip_loglik_grad calls, default
    options, every call blocking (the library synchronises before it returns).
  * gphip_loglik_grad alone at N = 2048 and 8192.
  * --parent-lib PATH: the loop and the one-theta call are ALSO timed on that build of the library (the commit before the
    batched call, built from its own tree): "not slower than the parent's loop" and "the one-theta call did not move" are
    statements about two builds.  Without it the loop of this build is the only baseline.

Method: every (build, what) pair runs in a process of its own (one GPU process at a time), `--rounds` rounds with the pairs
interleaved -- parent loop, batch, loop, parent loop, .. -- so that drift of the shared host hits all of them alike; inside a
process every size is warmed with 2 calls and timed `--repeats` times.  Reported: the median over all timed calls of a pair, and
the SPREAD of a pair = (largest - smallest of its per-round medians) / median, the parent's own run-to-run spread being the
yardstick for any difference.

    python scripts/gpu_grad_batch_time.py --parent-lib /path/to/parent/libgphip.so --out profiles/grad_batch_time.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 8
SIZES = [(512, 21), (2048, 21), (4096, 8), (8192, 4), (1024, 300)]
ONE = [2048, 8192]


def theta_rows(B):
    import numpy as np
    from bayesianinference_amd import synthetic as syn
    th = syn.default_theta("se_ard", D)
    rows = np.tile(th, (B, 1))
    for s in range(B):
        rows[s, :D] *= 1.0 + 0.01 * s
    return rows


def worker(what, repeats, sizes):
    """what: "loop" (B gphip_loglik_grad calls), "batch" (one gphip_loglik_grad_batch call), "one" (one gphip_loglik_grad call)"""
    from bayesianinference_amd import _lib, synthetic as syn
    out = {}
    for n, B in ([(n, 1) for n in ONE] if what == "one" else sizes):
        X, y = syn.make_dataset(n, D)
        Th = theta_rows(B)
        h = _lib.Handle(X, y, "se_ard")

        def call():
            if what == "batch":
                _, _, info = h.loglik_grad_batch(Th)
                assert not info.any()
            else:
                for t in Th:
                    assert h.loglik_grad(t)[2] == 0

        for _ in range(2):
            call()
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            call()
            times.append((time.perf_counter() - t0) * 1e3)
        out[f"{n}x{B}"] = times
        if what == "batch":
            out[f"{n}x{B}/slots"] = [h.get_option("last_grad_batch_slots"), h.get_option("last_grad_batch_route")]
        h.close()
    print("RESULT " + json.dumps(out))


def parse_sizes(text):
    return [tuple(int(v) for v in item.split(":")) for item in text.split(",")] if text else SIZES


def run_worker(what, lib, repeats, sizes):
    env = dict(os.environ)
    env.pop("GPHIP_LIB", None)
    if lib:
        env["GPHIP_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", what, "--repeats", str(repeats)] +
                       (["--sizes", sizes] if sizes else []), env=env,
                       capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        raise RuntimeError(f"worker {what} (lib={lib}) failed with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker")
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sizes", help='other (N, B) pairs than the table\'s, as "N:B,N:B"')
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_batch_time.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.repeats, parse_sizes(a.sizes))
    pairs = [("loop", None), ("batch", None), ("one", None)]
    if a.parent_lib:
        pairs = [("loop", a.parent_lib), ("batch", None), ("loop", None), ("one", a.parent_lib), ("one", None)]
    runs = {p: [] for p in pairs}
    for _ in range(a.rounds):
        for p in pairs:
            runs[p].append(run_worker(p[0], p[1], a.repeats, a.sizes))

    def med(p, key):
        return statistics.median(t for r in runs[p] for t in r[key])

    def spread(p, key):
        m = [statistics.median(r[key]) for r in runs[p]]
        return (max(m) - min(m)) / statistics.median(m)

    base = ("loop", a.parent_lib)
    lines = [f"# scripts/gpu_grad_batch_time.py on one MI355X: fp64 SE-ARD d = {D} (p = {D + 2}), default options, blocking calls, ms.",
             f"# {a.rounds} rounds of interleaved processes x {a.repeats} timed calls after 2 warm-up calls; median over all calls;",
             "# spread = (largest - smallest per-round median) / median.  " +
             ("Baseline: B gphip_loglik_grad calls on the PARENT build." if a.parent_lib else "Baseline: B gphip_loglik_grad calls on this build."),
             "#", f"# {'N':>6} {'B':>4} {'route':>9} | {'parent loop':>12} {'spread':>7} | " +
             (f"{'this loop':>10} {'spread':>7} | " if a.parent_lib else "") + f"{'batch':>9} {'spread':>7} | {'loop/batch':>10}"]
    for n, B in parse_sizes(a.sizes):
        key = f"{n}x{B}"
        g, route = runs[("batch", None)][0][key + "/slots"]
        groups = f"last {int(g)}" if route else "per-row"       # (rows in the last group; per-row: the group rule declined)
        row = f"  {n:>6} {B:>4} {groups:>9} | {med(base, key):>12.3f} {spread(base, key):>7.1%} | "
        if a.parent_lib:
            row += f"{med(('loop', None), key):>10.3f} {spread(('loop', None), key):>7.1%} | "
        row += f"{med(('batch', None), key):>9.3f} {spread(('batch', None), key):>7.1%} | {med(base, key) / med(('batch', None), key):>10.2f}"
        lines.append(row)
    lines += ["#", "# gphip_loglik_grad alone (one call):",
              f"# {'N':>6} | {'parent' if a.parent_lib else 'this':>10} {'spread':>7}" + (f" | {'this':>10} {'spread':>7} | {'this/parent':>11}" if a.parent_lib else "")]
    for n in ONE:
        key = f"{n}x1"
        b1 = ("one", a.parent_lib)
        row = f"  {n:>6} | {med(b1, key):>10.3f} {spread(b1, key):>7.1%}"
        if a.parent_lib:
            row += f" | {med(('one', None), key):>10.3f} {spread(('one', None), key):>7.1%} | {med(('one', None), key) / med(b1, key):>11.3f}"
        lines.append(row)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
