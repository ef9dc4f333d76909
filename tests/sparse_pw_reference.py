"""numpy float64 references for the sparse inducing-point GP with a noise variance nu_i and a mean m_i that depend on the point
(include/gphip.h gphip_sparse_*_pw), next to tests/sparse_reference.py, whose covariance helpers they use.
With Lambda = diag(nu), r = y - m, K_uu = k(Z, Z) + jitter I = L_u L_u^T and V = L_u^-1 k(Z, X), two algebraically different routes:

  (a) the formulas of the header: B = I + V Lambda^-1 V^T = L_B L_B^T, c = L_B^-1 V Lambda^-1 r (optionally in chunks of data points),
      F = -1/2 [N log 2 pi + sum log nu_i + log det B + r^T Lambda^-1 r - c^T c] - 1/2 sum_i (k_ii - |v_i|^2) / nu_i;
  (b) the definition: Q = V^T V dense, F = log N(y | m, Q + Lambda) - 1/2 sum_i (k_ii - Q_ii) / nu_i with an N x N Cholesky.

A None array is the constant of theta (sn^2; mu or 0), broadcast.  Shared by tests/test_sparse_pw.py, which pins the routes against
each other and against the constant reference on the CPU, and tests/test_gpu_sparse_pw.py."""
import numpy as np
import scipy.linalg as sla

import sparse_reference as ref
from bayesianinference_amd import _lib

PARTS = ("logdet_B", "ctc", "rwr", "tr_VWVt", "sum_kxx_w", "sum_log_nu")
SF = 1.1
SE_ARD_BODY = "T s = 0; for (int k = 0; k < D; ++k) { const T u = (X(k) - Y(k)) / P(k); s += u * u; } return P(D) * P(D) * exp((T)-0.5 * s);"

# (kernel, N, d, m, mean of the handle): the device cases of tests/test_gpu_sparse_pw.py, all at jitter 1e-6 sf^2.  N and m are no
# multiples of 128, (700, 3, 1000) has m > N, "custom" is the run-time compiled SE-ARD body.
CASES = [("se_ard", 1333, 3, 150, "const"), ("se_ard", 1500, 3, 300, "zero"), ("se_ard", 700, 3, 1000, "const"),
         ("se_ard", 1500, 1, 60, "zero"), ("matern52_ard", 1333, 3, 150, "zero"), ("se_ard*matern52_ard+const", 1333, 2, 150, "const"),
         ("custom", 1333, 3, 150, "zero")]
JITTER = 1e-6 * SF ** 2


def se_ard_fn(A, B, p):
    d = A.shape[-1]
    return p[d] ** 2 * np.exp(-0.5 * (((A - B) / p[:d]) ** 2).sum(-1))


def kernel_of(name, d):
    return _lib.CustomKernel(SE_ARD_BODY, d + 1, fn=se_ard_fn) if name == "custom" else name


def theta(name, d, mean):
    ell = [0.3] if d == 1 else list(np.linspace(0.8, 1.3, d))
    if name in ("se_ard", "matern52_ard", "custom"):
        th = ell + [SF, 0.15]
    elif name == "se_ard*matern52_ard+const":
        th = ell + [SF] + [1.4 * v for v in ell] + [0.9, 0.3, 0.15]
    else:
        raise ValueError(name)
    return np.array(th + ([0.2] if mean == "const" else []))


def inducing(X, m, extra):
    """m inducing points: every (N // m)-th data point; m > N: the data and the further points `extra`"""
    n = len(X)
    if m <= n:
        return X[::n // m][:m]
    return np.vstack([X, extra[:m - n]])


def noise(X, sn2):
    """nu_i = sn^2 s(x_i)^2 with s = 2^sin(3 x_1) in [0.5, 2]: on random inputs it differs from index to index"""
    X = np.atleast_2d(X)
    return sn2 * 4.0 ** np.sin(3.0 * X[:, 0])


def noise_decades(X, sn2):
    """nu_i = sn^2 10^(2 sin(5 x_1 + x_d)): four decades"""
    X = np.atleast_2d(X)
    return sn2 * 10.0 ** (2.0 * np.sin(5.0 * X[:, 0] + X[:, -1]))


def trend(X):
    """m_i = 0.2 + 0.3 x_{i,1}"""
    return 0.2 + 0.3 * np.atleast_2d(X)[:, 0]


def _arrays(kernel, th, P, mean, mean_arr, nu_arr):
    sn2, mu = ref.noise_and_mean(kernel, th, np.atleast_2d(P).shape[1], mean)
    n = len(np.atleast_2d(P))
    m = np.full(n, mu) if mean_arr is None else np.asarray(mean_arr, dtype=np.float64).reshape(n)
    nu = np.full(n, sn2) if nu_arr is None else np.asarray(nu_arr, dtype=np.float64).reshape(n)
    return m, nu


def bound_formulas(kernel, th, X, y, Z, jitter, mean_arr=None, nu_arr=None, mean="zero", chunk=None):
    """Route (a).  {"F", "parts" (the order of PARTS), "Lu", "LB", "c"}; chunk: data points per pass (None = all at once)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64).ravel()
    n, m = len(X), len(Z)
    mv, nu = _arrays(kernel, th, X, mean, mean_arr, nu_arr)
    Lu, _ = ref.kuu_factor(kernel, th, Z, jitter, mean)
    VWVt, VWr, rwr, skk, sln = np.zeros((m, m)), np.zeros(m), 0.0, 0.0, 0.0
    step = n if chunk is None else int(chunk)
    for c0 in range(0, n, step):
        Xc, r, w = X[c0:c0 + step], (y - mv)[c0:c0 + step], 1.0 / nu[c0:c0 + step]
        V = sla.solve_triangular(Lu, ref.cross(kernel, th, Z, Xc, mean), lower=True)
        VWVt += (V * w) @ V.T
        VWr += V @ (w * r)
        rwr += float(r @ (w * r))
        skk += float((ref.kdiag(kernel, th, Xc, mean) * w).sum())
        sln += float(np.log(nu[c0:c0 + step]).sum())
    tr = float(np.trace(VWVt))
    LB = sla.cholesky(VWVt + np.eye(m), lower=True)
    c = sla.solve_triangular(LB, VWr, lower=True)
    logdet, ctc = 2.0 * float(np.log(np.diag(LB)).sum()), float(c @ c)
    F = -0.5 * (n * ref.LOG_2PI + sln + logdet + rwr - ctc) - 0.5 * (skk - tr)
    return {"F": float(F), "parts": np.array([logdet, ctc, rwr, tr, skk, sln]), "Lu": Lu, "LB": LB, "c": c}


def bound_definition(kernel, th, X, y, Z, jitter, mean_arr=None, nu_arr=None, mean="zero"):
    """Route (b): log N(y | m, Q + Lambda) - 1/2 sum_i (k_ii - Q_ii) / nu_i, Q = K_fu K_uu^-1 K_uf, with an N x N Cholesky."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64).ravel()
    n = len(X)
    mv, nu = _arrays(kernel, th, X, mean, mean_arr, nu_arr)
    Lu, _ = ref.kuu_factor(kernel, th, Z, jitter, mean)
    A = sla.solve_triangular(Lu, ref.cross(kernel, th, Z, X, mean), lower=True)
    Q = A.T @ A
    gap = float(((ref.kdiag(kernel, th, X, mean) - np.diag(Q)) / nu).sum())
    L = sla.cholesky(Q + np.diag(nu), lower=True)
    z = sla.solve_triangular(L, y - mv, lower=True)
    return float(-0.5 * (n * ref.LOG_2PI + 2.0 * np.log(np.diag(L)).sum() + z @ z) - 0.5 * gap)


def predict_formulas(kernel, th, X, y, Z, jitter, Xs, mean_arr=None, nu_arr=None, mean_test=None, nu_test=None, mean="zero", latent=False):
    """Route (a): mean = m(x*) + v2^T c, var = k(x*, x*) [+ nu(x*)] - |v1|^2 + |v2|^2."""
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    ms, nus = _arrays(kernel, th, Xs, mean, mean_test, nu_test)
    f = bound_formulas(kernel, th, X, y, Z, jitter, mean_arr, nu_arr, mean)
    v1 = sla.solve_triangular(f["Lu"], ref.cross(kernel, th, Z, Xs, mean), lower=True)
    v2 = sla.solve_triangular(f["LB"], v1, lower=True)
    var = ref.kdiag(kernel, th, Xs, mean) + (0.0 if latent else nus) - (v1 * v1).sum(axis=0) + (v2 * v2).sum(axis=0)
    return ms + v2.T @ f["c"], var


def predict_definition(kernel, th, X, y, Z, jitter, Xs, mean_arr=None, nu_arr=None, mean_test=None, nu_test=None, mean="zero", latent=False):
    """Route (b): mean = m(x*) + Q*f (Q + Lambda)^-1 r, var = k(x*, x*) [+ nu(x*)] - Q*f (Q + Lambda)^-1 Qf*."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64).ravel()
    mv, nu = _arrays(kernel, th, X, mean, mean_arr, nu_arr)
    ms, nus = _arrays(kernel, th, Xs, mean, mean_test, nu_test)
    Lu, _ = ref.kuu_factor(kernel, th, Z, jitter, mean)
    A = sla.solve_triangular(Lu, ref.cross(kernel, th, Z, X, mean), lower=True)
    As = sla.solve_triangular(Lu, ref.cross(kernel, th, Z, Xs, mean), lower=True)
    cf = sla.cho_factor(A.T @ A + np.diag(nu), lower=True)
    Qsf = As.T @ A
    var = ref.kdiag(kernel, th, Xs, mean) + (0.0 if latent else nus) - np.einsum("ij,ji->i", Qsf, sla.cho_solve(cf, Qsf.T))
    return ms + Qsf @ sla.cho_solve(cf, y - mv), var
