"""The cases of the sparse prediction over posterior samples (gphip_sparse_predict_samples): data, inducing points, theta rows,
jitter and test points, shared by tests/test_sparse_samples.py, which checks their numpy side on the CPU (conditioning, the two
reference routes of the prediction), and tests/test_gpu_sparse_samples.py, which runs them on the device.  The references are
computed once per (case, latent) and handed out read-only."""
import functools

import numpy as np

import sparse_batch_cases as cases
import sparse_reference as ref
from bayesianinference_amd import _lib, synthetic as syn

M = 300                                         # test points: not a multiple of 128, three tiles

# the non-stationary run-time compiled body of tests/test_gpu_sparse.py: k(x, x) = sf^2 (1 + c^2 x_0^2) depends on the point AND on theta
NONSTAT_BODY = ("T s = 0; for (int k = 0; k < D; ++k) { const T u = X(k) - Y(k); s += u * u; } "
                "return P(1) * P(1) * exp((T)-0.5 * s / (P(0) * P(0))) * ((T)1 + P(2) * P(2) * X(0) * Y(0));")
NONSTAT_BASE = np.array([0.9, 1.1, 0.7, 0.15])


def nonstat_fn(A, B, p):
    return p[1] ** 2 * np.exp(-0.5 * ((A - B) ** 2).sum(-1) / p[0] ** 2) * (1.0 + p[2] ** 2 * A[..., 0] * B[..., 0])


def nonstat_case():
    """N = 1333, d = 2, m = 150, zero mean, four rows around the base theta that differ in every entry"""
    X, y = syn.make_dataset(1333, 2)
    rows = NONSTAT_BASE[None, :] * np.random.default_rng(20).uniform(0.8, 1.25, size=(4, 4))
    return X, y, cases.inducing(X, 150), _lib.CustomKernel(NONSTAT_BODY, 3, fn=nonstat_fn), rows


# label -> (kernel, X, y, Z, mean, rows, jitter, the rows that are meant to succeed)
LABELS = ["parity%d" % k for k in range(len(cases.PARITY))] + ["nonstat", "failure"]


@functools.lru_cache(maxsize=None)
def case(label):
    if label.startswith("parity"):
        name, n, d, m, mean, B = cases.PARITY[int(label[6:])]
        X, y, Z, kernel, rows = cases.parity_case(name, n, d, m, mean, B)
        return kernel, X, y, Z, mean, rows, cases.JITTER, tuple(range(B))
    if label == "nonstat":
        X, y, Z, kernel, rows = nonstat_case()
        return kernel, X, y, Z, "zero", rows, cases.JITTER, tuple(range(len(rows)))
    if label == "failure":
        X, y, Z, rows = cases.failure_case()
        return "se_ard", X, y, Z, "zero", rows, 0.0, (0, 2, 4)
    raise ValueError(label)


def test_points(d, m=M):
    return syn.make_test_points(m, d)


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(label, latent, m=M):
    """{"mean" [S, m], "var" [S, m], "F" [S], "ymax", "kmax" [S]} by route (a) of tests/sparse_reference.py; the rows that are
    meant to fail are NaN.  ymax = max |y| and kmax[s] = max k(x, x) over the data under row s scale the bars."""
    kernel, X, y, Z, mean, rows, jit, good = case(label)
    Xs = test_points(X.shape[1], m)
    S = len(rows)
    mu, var, F, kmax = np.full((S, m), np.nan), np.full((S, m), np.nan), np.full(S, np.nan), np.full(S, np.nan)
    for s in good:
        mu[s], var[s] = ref.predict_formulas(kernel, rows[s], X, y, Z, jit, Xs, mean, latent)
        F[s] = ref.bound_formulas(kernel, rows[s], X, y, Z, jit, mean)["F"]
        kmax[s] = float(ref.kdiag(kernel, rows[s], X, mean).max())
    return {"mean": _frozen(mu), "var": _frozen(var), "F": _frozen(F), "ymax": float(np.abs(y).max()), "kmax": _frozen(kmax)}


# the seams case: three tile columns of inducing points, 12 row tiles of data, five rows
SEAMS = cases.DETERMINISM


@functools.lru_cache(maxsize=None)
def seams_case():
    name, n, d, m, mean, B = SEAMS
    X, y, Z, kernel, rows = cases.parity_case(name, n, d, m, mean, B)
    Xs = test_points(d)
    mu, var, F = np.empty((B, M)), np.empty((B, M)), np.empty(B)
    for s in range(B):
        mu[s], var[s] = ref.predict_formulas(kernel, rows[s], X, y, Z, cases.JITTER, Xs, mean)
        F[s] = ref.bound_formulas(kernel, rows[s], X, y, Z, cases.JITTER, mean)["F"]
    kmax = np.array([float(ref.kdiag(kernel, th, X, mean).max()) for th in rows])
    return X, y, Z, mean, _frozen(rows), Xs, {"mean": _frozen(mu), "var": _frozen(var), "F": _frozen(F),
                                              "ymax": float(np.abs(y).max()), "kmax": _frozen(kmax)}
