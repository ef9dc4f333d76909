"""float64 numpy reference for the mixture paths object (include/gphip.h gphip_paths_create_samples): per hyper-parameter row the
reference of tests/paths_reference.py and tests/paths_own_reference.py as they are, stacked in draw order.  No new mathematics:
draw q of row r is draw q of an ordinary paths object at Thetas[r], made from row r's table and its own w and eps."""
import numpy as np

import paths_own_reference as por
import paths_reference as pr


def ell_index(name, d):
    """the positions of the length scales in theta of a case of paths_reference.CASES"""
    if name in ("se", "matern32"):
        return [0]
    if name in ("se_ard", "matern52_ard", "rq_ard"):
        return list(range(d))
    if name == "se_ard*matern32+const":
        return list(range(d)) + [d + 1]
    if name == "se+rq":
        return [0, 2]
    raise ValueError(name)


def rows_of(name, d, theta, factors=(1.0, 0.8, 1.25)):
    """Thetas [R, p]: the case's theta and copies with the length scales multiplied by the factors; the noise is kept, so every
    row factors"""
    th = np.tile(np.asarray(theta, dtype=np.float64), (len(factors), 1))
    idx = ell_index(name, d)
    for r, f in enumerate(factors):
        th[r, idx] *= f
    return th


def row_of_draw(counts):
    return np.repeat(np.arange(len(counts)), counts)


def mix(kernel, thetas, X, y, pts, tables, w, eps, counts, mean="zero", own=False, dtype=np.float64, grad=True, rows=None):
    """{"v" [S, N], "out" [S, M], "dout" [S, M, d]} of the mixture object: tables[r] = row r's {"omega", "phase", "amp"}, w [S, Ftot]
    and eps [S, N] in draw order.  pts [M, d] (all draws at the same points) or, own=True, [S, M, d].  rows: only these rows are
    evaluated (the others' entries stay NaN): a test names the rows it leaves out."""
    counts = np.asarray(counts)
    S, start = int(counts.sum()), np.concatenate([[0], np.cumsum(counts)])
    pts = np.asarray(pts, dtype=np.float64)
    M, d = pts.shape[-2], pts.shape[-1]
    res = {"v": np.full((S, len(X)), np.nan), "out": np.full((S, M), np.nan)}
    if grad:
        res["dout"] = np.full((S, M, d), np.nan)
    for r in (range(len(counts)) if rows is None else rows):
        if counts[r] == 0:
            continue
        sl = slice(start[r], start[r + 1])
        one = pr.paths(kernel, thetas[r], X, y, pts[0, :1] if own else pts, tables[r], w[sl], eps[sl], mean, dtype=dtype, grad=grad and not own)
        res["v"][sl] = one["v"]
        if own:
            one = por.paths_own(kernel, thetas[r], X, y, pts[sl], tables[r], w[sl], eps[sl], mean, dtype=dtype, grad=grad)
        res["out"][sl] = one["out"]
        if grad:
            res["dout"][sl] = one["dout"]
    return res
