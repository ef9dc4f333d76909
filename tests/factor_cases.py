"""The case table of the factor tests: tests/test_factor_reference.py runs every row through LAPACK and the host emulation
of the blocked algorithm, tests/test_gpu_factor.py through the device.  numpy only.

A row: id, kernel, d, mean, n, sn, dtype, opts (gphip_set_option pairs, in order) and launches = the per-class launch counts
(potrf, trsm, gemm_panel, syrk_trailing) the fit must show in the profile -- which route ran is asserted, never assumed.  The counts
follow from queue_factor / queue_panel / queue_factor_dataflow (csrc/gphip.hip) for Nt = ceil(n / 128) tile columns:
  * a single dataflow launch is ONE gemm_panel record and nothing else (the finalize and the rebuild of the 128-block inverses
    are not profiled);
  * the multi-kernel schedule factors every diagonal tile with one potrf launch -- unless an update launch took it on
    ("fuse_potrf", which the latency GEMM shape never does) -- and solves below it with one trsm launch; every look-ahead or
    in-panel update is a gemm_panel record, every trailing update a syrk_trailing one;
  * a dataflow tail or a dataflow panel ("panel_df") is a gemm_panel record next to the trailing updates: potrf = 0, syrk > 0.
What the launch list cannot show -- a kernel's internal shape (thin_tiles, latency_gemm, dataflow_occ3, left- against right-
looking in-panel updates, 64- against 128-tiles of the single launch) -- is recorded in SAME_LAUNCHES_AS."""
import numpy as np

SF = 1.1
SEED = 20240607
SINGLE = (0, 0, 1, 0)                          # one dataflow launch


def dataset(n, d):
    """X uniform in [-1, 1]^d, y a smooth function of it plus noise; the first rows of a longer draw are the shorter draw"""
    rng = np.random.default_rng(SEED + d)
    X = rng.uniform(-1.0, 1.0, size=(n, d))
    y = np.sin(2.0 * X.sum(axis=1)) + 0.5 * np.cos(3.0 * X[:, 0]) + 0.3 + 0.1 * np.random.default_rng(SEED + 100 + d).standard_normal(n)
    return X, y


def theta(kernel, d, sn, mean="zero"):
    ell = np.sqrt(d) * np.linspace(0.8, 1.3, d)
    if kernel in ("se", "matern52"):
        th = [ell[0], SF, sn]
    elif kernel in ("se_ard", "matern52_ard"):
        th = list(ell) + [SF, sn]
    elif kernel == "rq_ard+const":
        th = list(ell) + [1.5, SF, 0.4, sn]     # alpha, sf, the constant offset c
    else:
        raise ValueError(kernel)
    return np.array(th + ([0.25] if mean == "const" else []))


def _row(id, n, kernel="se_ard", d=3, mean="zero", sn=0.15, dtype=64, opts=(), launches=SINGLE):
    return dict(id=id, kernel=kernel, d=d, mean=mean, n=n, sn=0.3 if dtype == 32 and sn == 0.15 else sn, dtype=dtype,
                opts=tuple(opts), launches=tuple(launches))


# ---- size edges: default options; the ragged last tile, the 64-block seam inside a 128-tile, one to four tile columns ----
SIZE_EDGES = [_row("n%d-f64" % n, n) for n in (1, 2, 63, 64, 65, 127, 128, 129, 257, 385)]
SIZE_EDGES += [_row("n%d-f32" % n, n, dtype=32) for n in (65, 129, 385)]

# ---- the schedule matrix: Nt = 6 (641: a last tile of ONE live row; 700: a ragged one) ----
MK = (("dataflow", 0),)
_SCHEDULES = [
    # id, opts, launches
    ("mk-nolookahead", MK + (("panel", 1), ("lookahead", 0)), (6, 6, 0, 6)),
    ("mk-lookahead", MK + (("panel", 1),), (6, 6, 5, 6)),
    ("mk-nofuse-throughput-gemm", MK + (("panel", 1), ("latency_gemm", 0), ("fuse_potrf", 0)), (6, 6, 5, 6)),
    ("mk-fuse-potrf", MK + (("panel", 1), ("latency_gemm", 0), ("fuse_potrf", 1)), (1, 6, 5, 6)),
    ("mk-thick-tiles", MK + (("panel", 1), ("thin_tiles", 0)), (6, 6, 5, 6)),
    ("mk-panel3-right", MK + (("panel", 3), ("panel_left", 0)), (6, 6, 5, 2)),
    ("mk-panel3-left", MK + (("panel", 3), ("panel_left", 1)), (6, 6, 5, 2)),
    ("mk-panel2", MK + (("panel", 2),), (6, 6, 5, 3)),
    ("single-64", (), SINGLE),
    ("single-128", (("dataflow_fine_nt", 0),), SINGLE),
    ("single-64-occ3", (("dataflow_occ3", 1),), SINGLE),
    ("tail-64", (("panel", 1), ("dataflow_max_nt", 3), ("dataflow_tail", 2)), (4, 4, 4, 4)),
    ("tail-128", (("panel", 1), ("dataflow_max_nt", 4), ("dataflow_tail", 4)), (2, 2, 2, 2)),
    ("panel-df", (("panel", 2), ("dataflow_max_nt", 3), ("panel_df", 1)), (0, 0, 3, 2)),
    ("fused-eval-0", (("fused_eval", 0),), SINGLE),
    ("fused-eval-1", (("fused_eval", 1),), SINGLE),
]
SCHEDULES = [_row("n%d-%s" % (n, sid), n, opts=opts, launches=la) for n in (641, 700) for sid, opts, la in _SCHEDULES]
SCHEDULES += [_row("n%d-f32-single-128" % n, n, dtype=32) for n in (641, 700)]
SCHEDULES += [_row("n%d-f32-mk" % n, n, dtype=32, opts=MK, launches=(6, 6, 5, 2)) for n in (641, 700)]

# rows whose route differs from another row's only INSIDE a kernel: the launch list is the same, the option is read back
SAME_LAUNCHES_AS = {"mk-thick-tiles": "mk-lookahead", "mk-nofuse-throughput-gemm": "mk-lookahead", "mk-panel3-left": "mk-panel3-right",
                    "single-128": "single-64", "single-64-occ3": "single-64", "fused-eval-0": "single-64", "fused-eval-1": "single-64"}

# ---- other covariance forms, N = 385 (Nt = 4: one outer panel on the multi-kernel route) ----
MK385 = (4, 4, 3, 1)
KERNELS = [
    _row("matern52_ard-d2-const", 385, "matern52_ard", 2, "const"),
    _row("matern52_ard-d2-const-mk", 385, "matern52_ard", 2, "const", opts=MK, launches=MK385),
    _row("rq_ard+const-d3", 385, "rq_ard+const", 3),
    _row("rq_ard+const-d3-mk", 385, "rq_ard+const", 3, opts=MK, launches=MK385),
    _row("se-d1-sn0.05", 385, "se", 1, sn=0.05),           # the least favourable for the explicit inverses (cond(K) largest)
]

ALL = SIZE_EDGES + SCHEDULES + KERNELS
assert len({c["id"] for c in ALL}) == len(ALL)


def inputs(case):
    """(X, y, theta) of a row"""
    X, y = dataset(case["n"], case["d"])
    return X, y, theta(case["kernel"], case["d"], case["sn"], case["mean"])


def residual(case, y, th):
    """r = y - mu in the handle's arithmetic type (fp32 handles keep y and mu as float32), widened"""
    mu = th[-1] if case["mean"] == "const" else 0.0
    if case["dtype"] == 32:
        return (y.astype(np.float32) - np.float32(mu)).astype(np.float64)
    return y - mu


def distinct_inputs():
    """one row per distinct matrix of the table (kernel, d, mean, n, sn): what the host tests factor"""
    seen, out = set(), []
    for c in ALL:
        key = (c["kernel"], c["d"], c["mean"], c["n"], c["sn"], c["dtype"])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out
