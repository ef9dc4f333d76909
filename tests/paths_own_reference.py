"""float64 numpy reference for gphip_paths_eval_own (include/gphip.h): every pathwise draw at ITS OWN points.  Built on
tests/paths_reference.py, which is used as it is: draw s at its points is row s of paths(..) evaluated at those points.

ReferencePaths stands in for _lib.Paths (S, d, eval, eval_own) on the host, so that posteriorFunctionSamples.maximize can be run
end to end without a device: the table comes from _lib.rff_table (host only), w and eps from paths_reference.philox_normal."""
import numpy as np

import paths_reference as pr


def paths_own(kernel, th, X, y, Xs_own, table, w, eps, mean="zero", dtype=np.float64, grad=True):
    """Xs_own [S, M, d] -> {"out" [S, M], "dout" [S, M, d]}: per draw, its row of paths(..) at that draw's points"""
    Xs_own = np.asarray(Xs_own, dtype=np.float64)
    S, M, d = Xs_own.shape
    assert S == len(w)
    # one paths(..) call on the S M stacked points (one factorisation), of which draw s keeps the block of its own points
    r = pr.paths(kernel, th, X, y, Xs_own.reshape(S * M, d), table, w, eps, mean, dtype=dtype, grad=grad)
    rows = np.arange(S)
    res = {"out": r["out"].reshape(S, S, M)[rows, rows]}
    if grad:
        res["dout"] = r["dout"].reshape(S, S, M, d)[rows, rows]
    return res


def host_draw(kernel, d, th, n_train, S, F, seed, mean="zero"):
    """(table, w, eps) of gphip_paths_create(S, F, seed) made on the host: the documented streams"""
    from bayesianinference_amd import _lib
    om, ph, amp = _lib.rff_table(kernel, d, th, F, seed)
    table = {"omega": om, "phase": ph, "amp": amp}
    sn = abs(th[-2 if mean == "const" else -1])
    w = pr.philox_normal(seed, np.arange(S)[:, None], np.arange(len(ph))[None, :])
    eps = sn * pr.philox_normal(pr.rff_key(seed, pr.TAG_EPS), np.arange(S)[:, None], np.arange(n_train)[None, :])
    return table, w, eps


def grid_slack(fgrid, h):
    """the most a grid of spacing h can miss of a maximum: 1/8 h^2 max |f''|, f'' by second differences"""
    f2 = (fgrid[:, 2:] - 2.0 * fgrid[:, 1:-1] + fgrid[:, :-2]) / (h * h)
    return 0.125 * h * h * np.abs(f2).max(axis=1)


class ReferencePaths:
    """the interface of _lib.Paths that posteriorFunctionSamples uses, evaluated by the numpy reference; counts its calls"""

    def __init__(self, kernel, th, X, y, table, w, eps, mean="zero"):
        self.kernel, self.th, self.X, self.y, self.table, self.w, self.eps, self.mean = kernel, th, X, y, table, w, eps, mean
        self.S, self.d = len(w), np.atleast_2d(X).shape[1]
        self.calls = {"eval": 0, "eval_own": 0}

    def eval(self, Xs, grad=False):
        self.calls["eval"] += 1
        r = pr.paths(self.kernel, self.th, self.X, self.y, Xs, self.table, self.w, self.eps, self.mean, grad=grad)
        return (r["out"], r["dout"]) if grad else r["out"]

    def eval_own(self, Xs, grad=False):
        self.calls["eval_own"] += 1
        r = paths_own(self.kernel, self.th, self.X, self.y, Xs, self.table, self.w, self.eps, self.mean, grad=grad)
        return (r["out"], r["dout"]) if grad else r["out"]

    def close(self):
        pass
