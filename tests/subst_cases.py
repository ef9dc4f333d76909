"""The case table of the substitution tests: tests/test_subst_reference.py runs every distinct matrix through LAPACK and
both host emulations, tests/test_gpu_subst.py every row through the device.  numpy only.  Inputs: factor_cases.dataset / theta.

A row: id, call ("solve" | "predict"), kernel, d, mean, n, sn, dtype, opts (gphip_set_option pairs, in order, set on BOTH handles
before the fit), count (right-hand sides / test points), route (per chunk of the call) and launches = the (trsm, gemm_panel,
predict_epilogue) launch counts and trsm_flops the call must show in the profile -- which route ran is asserted, never assumed.
They follow from gphip_solve / predict_local and from queue_trsv, launch_dataflow_inverse, queue_forward_panel and
queue_backward_rows (csrc/gphip.hip), with Nt = ceil(n / 128) tile columns, Npad = 128 Nt and mpad = the chunk's rows padded to 128:

  "trsv"  solve only, <= 4 finite right-hand sides, option trsv = 1: two single-vector launches (forward, backward), each ONE trsm
          record with ZERO flops (queue_trsv books bytes only).
  "df"    fp64, option dataflow != 0, predict_df > 0, mpad <= 2 predict_df (Npad <= 8192) and mpad <= Npad: the forward dataflow
          launch is ONE trsm record with mpad Npad^2 flops; a solve adds the backward launch, one more record of the same flops.
  "mk"    otherwise: queue_forward_rows = one trsm record per tile column (its diagonal product with W_b; flops > 0) and one
          gemm_panel record per in-panel update (k1 - k0 - 1 per outer panel [k0, k1)) and per out-of-panel update (every panel
          but the last): Nt - 1 in all WHATEVER the panel width.  A solve adds queue_backward_rows: Nt diagonal products and
          Nt - 1 updates, all gemm_panel records.  So mk shows (Nt, Nt - 1) for a prediction, (Nt, 3 Nt - 2) for a solve.
  every prediction chunk ends with ONE predict_epilogue record (queue_predict_reduce).
  chunks: gphip_solve 2048 right-hand sides; predict_local min(32768, M padded) test points at these sizes (8 GiB / Npad rows
          is far more).  Each chunk takes its route by its own mpad.

What the profile cannot tell apart is listed in SAME_LAUNCHES_AS; there the option that selects the variant is read back."""
import numpy as np

import factor_cases as fc

TB = 128
SOLVE_CHUNK = 2048
PREDICT_CHUNK = 32768
RHS_SEED = 20240911


def nt_of(n):
    return (n + TB - 1) // TB


def chunks(count, cap):
    return [min(cap, count - c0) for c0 in range(0, count, cap)]


def pad(m):
    return (m + TB - 1) // TB * TB


def route_of_chunk(row, mc):
    o = dict(row["opts"])
    npad, mpad = TB * nt_of(row["n"]), pad(mc)
    if row["call"] == "solve" and row["count"] <= 4 and o.get("trsv", 1) and row.get("finite", True):
        return "trsv"
    pdf = o.get("predict_df", 2048)
    if row["dtype"] == 64 and o.get("dataflow", 1) and pdf > 0 and mpad <= 2 * pdf and mpad <= npad:
        return "df"
    return "mk"


def expected(row):
    """((trsm, gemm_panel, predict_epilogue) launches, trsm flops or None = 'positive', the chunks' routes)"""
    nt = nt_of(row["n"])
    npad = TB * nt
    solve = row["call"] == "solve"
    trsm = gemm = epi = 0
    flops, exact, routes = 0.0, True, []
    for mc in chunks(row["count"], SOLVE_CHUNK if solve else PREDICT_CHUNK):
        r = route_of_chunk(row, mc)
        routes.append(r)
        if r == "trsv":
            trsm += 2 * ((mc + 3) // 4)
        elif r == "df":
            trsm += 2 if solve else 1
            flops += (2 if solve else 1) * float(pad(mc)) * npad * npad
        else:
            trsm += nt
            gemm += (nt - 1) + ((2 * nt - 1) if solve else 0)
            exact = False
        epi += 0 if solve else 1
    return (trsm, gemm, epi), (flops if exact else None), tuple(routes)


def staging(nrhs):
    """gphip_solve's staging of a GEMM-shaped chunk: compact rows through rows_to_vblock_kernel while 4 mc <= 3 mpad"""
    return "compact" if 4 * nrhs <= 3 * pad(nrhs) else "transposed"


def wide_panel(row):
    """queue_forward_rows / queue_backward_rows widen the outer panel to >= 12 tile columns from 8 row tiles on"""
    return any(pad(mc) // TB >= 8 for mc in chunks(row["count"], SOLVE_CHUNK if row["call"] == "solve" else PREDICT_CHUNK))


def _row(call, tag, n, count, kernel="se_ard", d=3, mean="zero", sn=0.15, dtype=64, opts=(), finite=True):
    row = dict(call=call, kernel=kernel, d=d, mean=mean, n=n, sn=0.3 if dtype == 32 and sn == 0.15 else sn, dtype=dtype, opts=tuple(opts),
               count=count, finite=finite, tag=tag)
    row["id"] = "%s-n%d-f%d-%s-%s%d" % (call, n, dtype, tag, "r" if call == "solve" else "m", count)
    row["launches"], row["trsm_flops"], row["route"] = expected(row)
    return row


# ---- the producers of the 128-block inverses (options of the FIT) ----
FINE0 = (("dataflow_fine_nt", 0),)                       # the 128-tile single launch: 64-block inverses cut by w128_to_w64_kernel
MKFIT = (("dataflow", 0),)                               # the multi-kernel schedule: inverses written by the potrf128 core
TAIL64 = (("panel", 1), ("dataflow_max_nt", 3), ("dataflow_tail", 2))
PANELDF = (("panel", 2), ("dataflow_max_nt", 3), ("panel_df", 1))
PRODUCERS = (("single64", ()), ("single128", FINE0), ("mkfit", MKFIT), ("tail64", TAIL64), ("paneldf", PANELDF))
NOPDF = (("predict_df", 0),)
NS = (641, 700)                                          # Nt = 6: a last tile of ONE live row; a ragged one
SIZES = (1, 2, 64, 65, 128, 129, 257, 385, 513, 641, 700, 1000)      # Nt = 1 .. 6 and 8: the tile-role ticket list of the single-
#                                                          vector launches is empty below Nt = 5 and has 1, 3, 10 tasks at 5, 6, 8

# ---- solve ----
S = []
S += [_row("solve", "default", n, r) for n in SIZES for r in (1, 4)]
S += [_row("solve", "default", 641, r) for r in (2, 3)]
S += [_row("solve", "default", n, r, dtype=32) for n in (65, 129, 385, 700) for r in (1, 4)]
S += [_row("solve", tag, n, r, opts=o) for tag, o in PRODUCERS[1:] for n in NS for r in (1, 4)]
S += [_row("solve", "trsv0", n, r, opts=(("trsv", 0),)) for n in NS for r in (1, 4)]
DF_NRHS = (5, 64, 65, 96, 97, 128, 129, 700)             # the compact staging ends at 96 of 128
S += [_row("solve", "default", n, r) for n in NS for r in DF_NRHS]
S += [_row("solve", "single128", n, r, opts=FINE0) for n in NS for r in DF_NRHS]
S += [_row("solve", "single128-trsv0", n, r, opts=FINE0 + (("trsv", 0),)) for n in NS for r in (1, 4)]
for _p in (1, 2, 4):
    S += [_row("solve", "nopdf-panel%d" % _p, n, r, opts=(("panel", _p),) + NOPDF) for n in NS for r in (5, 129)]
    S += [_row("solve", "mkfit-panel%d" % _p, n, r, opts=MKFIT + (("panel", _p),)) for n in NS for r in (5, 129)]
S += [_row("solve", "nopdf", n, 1030, opts=NOPDF) for n in NS]
S += [_row("solve", "mkfit", n, 1030, opts=MKFIT) for n in NS]
S += [_row("solve", "default", n, r, dtype=32) for n in (129, 700) for r in (5, 129)]
S += [_row("solve", "seam2048", 257, SOLVE_CHUNK + 130)]
KERNEL_ROWS = (("matern52_ard", 2, "const", 0.15), ("rq_ard+const", 3, "zero", 0.15), ("se", 1, "zero", 0.05))
S += [_row("solve", k.replace("+", "-"), 385, r, kernel=k, d=d, mean=m, sn=sn) for k, d, m, sn in KERNEL_ROWS for r in (1, 5)]
SOLVE = S
SWITCH = (("predict_df", 128),)                          # mpad <= 256 dataflow, beyond it multi-kernel: both on ONE handle
SOLVE_SWITCH = [[_row("solve", "pdf128", n, r, opts=SWITCH) for r in (256, 257)] for n in NS]
SOLVE_NONFINITE = _row("solve", "nonfinite", 385, 3, finite=False)

# ---- predict ----
P = []
P += [_row("predict", "default", n, m) for n in NS for m in (1, 63, 64, 65, 128, 129, 700)]
P += [_row("predict", "single128", n, m, opts=FINE0) for n in NS for m in (1, 129)]
for _p in (1, 2, 4):
    P += [_row("predict", "nopdf-panel%d" % _p, n, m, opts=(("panel", _p),) + NOPDF) for n in NS for m in (1, 129)]
    P += [_row("predict", "mkfit-panel%d" % _p, n, m, opts=MKFIT + (("panel", _p),)) for n in NS for m in (1, 129)]
P += [_row("predict", "nopdf", n, 1030, opts=NOPDF) for n in NS]
P += [_row("predict", "mkfit", n, 1030, opts=MKFIT) for n in NS]
P += [_row("predict", "default", 129, 300)]              # more test tiles than Npad / 64: the dataflow launch is refused
P += [_row("predict", "default", n, m, dtype=32) for n in (129, 700) for m in (1, 129)]
P += [_row("predict", "default", n, 5) for n in SIZES]
P += [_row("predict", "matern52_ard", 385, 65, kernel="matern52_ard", d=2, mean="const"),
      _row("predict", "rq_ard-const", 385, 65, kernel="rq_ard+const", d=3)]
PREDICT = P
PREDICT_SWITCH = [[_row("predict", "pdf128", n, m, opts=SWITCH) for m in (256, 257)] for n in NS]
PREDICT_SEAM = _row("predict", "seam32768", 129, PREDICT_CHUNK + 130)

ALL = SOLVE + [r for pair in SOLVE_SWITCH for r in pair] + [SOLVE_NONFINITE] + PREDICT + [r for pair in PREDICT_SWITCH for r in pair] + [PREDICT_SEAM]
assert len({c["id"] for c in ALL}) == len(ALL)

# variants the (trsm, gemm_panel, predict_epilogue) profile cannot tell from another row: tag -> (the tag it looks like, the witness)
SAME_LAUNCHES_AS = {
    "single128": ("default", "option dataflow_fine_nt read back: the 64-block inverses are cut by w128_to_w64_kernel, not left by the fit"),
    "single128-trsv0": ("trsv0", "option dataflow_fine_nt read back"),
    "tail64": ("default", "the fit's own launch list (factor_cases tail-64); the single-vector launches are the same two records"),
    "paneldf": ("default", "the fit's own launch list (factor_cases panel-df)"),
    "mkfit": ("default", "the fit's own launch list for <= 4 vectors; GEMM-shaped calls differ (mk)"),
    "nopdf-panel2": ("nopdf-panel1", "option panel read back: Nt - 1 updates whatever the panel width; the gemm_panel BYTES differ"),
    "nopdf-panel4": ("nopdf-panel1", "option panel read back"),
    "mkfit-panel1": ("nopdf-panel1", "option dataflow read back"),
    "mkfit-panel2": ("nopdf-panel1", "options dataflow and panel read back"),
    "mkfit-panel4": ("nopdf-panel1", "options dataflow and panel read back"),
    "wide panel (count 1030, the 2048 chunks)": ("the narrow panel", "Mt >= 8 and option panel_wide = 1 read back"),
    "compact staging (4 nrhs <= 3 mpad)": ("the transposed upload", "decided by nrhs alone: staging(nrhs)"),
}


# ---- inputs ----
def inputs(row):
    X, y = fc.dataset(row["n"], row["d"])
    return X, y, fc.theta(row["kernel"], row["d"], row["sn"], row["mean"])


def mu_of(row, th):
    return float(th[-1]) if row["mean"] == "const" else 0.0


def rhs(row, y, th):
    """[n, count]: standard normal at a fixed seed; one column r = y - mu (alpha of the fit is among the solutions); one column
    e_N, the last unit vector, which lands in the ragged tile.  One vector: r.  Two: e_N, r."""
    n, k = row["n"], row["count"]
    B = np.random.default_rng(RHS_SEED + n + k).standard_normal((n, k))
    r = fc.residual(row, y, th)
    e = np.zeros(n)
    e[-1] = 1.0
    if k == 1:
        B[:, 0] = r
    elif k == 2:
        B[:, 0], B[:, 1] = e, r
    else:
        B[:, 1], B[:, 2] = r, e
    return B


def test_points(row, X):
    """uniform in [-1, 1]^d (inside the training range: the form of the k* build cannot change from chunk to chunk), the last
    three (from four points on) training points repeated exactly"""
    n, m, d = row["n"], row["count"], row["d"]
    Xs = np.random.default_rng(RHS_SEED + 7 * n + m).uniform(-1.0, 1.0, size=(m, d))
    if m >= 4:
        Xs[-3:] = X[[0, n // 2, n - 1]]
    return Xs


def stale_theta(row, th):
    """theta_2 of the stale-copy rows: sn x 1.3, every length scale x 0.85"""
    th2 = np.array(th, dtype=np.float64)
    nl = row["d"] if "ard" in row["kernel"] else 1
    th2[:nl] *= 0.85
    th2[len(th2) - (2 if row["mean"] == "const" else 1)] *= 1.3
    return th2


def distinct_inputs():
    """one row per distinct matrix of the table (kernel, d, mean, n, sn, dtype): what the host tests factor"""
    seen, out = set(), []
    for c in ALL:
        key = (c["kernel"], c["d"], c["mean"], c["n"], c["sn"], c["dtype"])
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out
