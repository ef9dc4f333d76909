"""numpy float64 references for the sparse inducing-point GP (Titsias 2009; include/gphip.h gphip_sparse_*), built from the CPU
oracle's covariance.  Two algebraically different routes:

  (a) the formulas of the header: L_u, V = L_u^-1 K_uf, B = sn^2 I + V V^T, c = L_B^-1 V r (optionally in chunks of data points);
  (b) the definition: Q = K_fu K_uu^-1 K_uf dense, log N(y | m, Q + sn^2 I) - tr(K_ff - Q) / (2 sn^2) with an N x N Cholesky.

K_uu always means k(Z, Z) + jitter I (the jitter is part of the model).  Shared by tests/test_sparse.py, which pins the routes
against each other and against extended precision, and tests/test_gpu_sparse.py.  The textbook m x m form with an explicit inverse
of K_uu + K_uf K_fu / sn^2 is NOT used: it loses five digits of the mean to rounding."""
import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as orc

LOG_2PI = float(np.log(2.0 * np.pi))
PARTS = ("logdet_B", "ctc", "rtr", "tr_VVt", "sum_kxx")


def cross(kernel, th, A, B, mean):
    """k(a_i, b_j) without any nugget"""
    return orc.k_and_kappa(kernel, th, A, B, mean)[0]


def kdiag(kernel, th, P, mean):
    """k(p_i, p_i) without the nugget"""
    P = np.atleast_2d(np.asarray(P, dtype=np.float64))
    if orc.is_custom(kernel):
        p = np.asarray(th, dtype=np.float64)[:kernel.nparams]
        return np.asarray(kernel.fn(P, P, p), dtype=np.float64)
    return np.full(len(P), cross(kernel, th, P[:1], P[:1], mean)[0, 0])             # (every named family is stationary)


def noise_and_mean(kernel, th, d, mean):
    _, _, sn, mu = orc.split_theta(kernel, d, th, mean)
    return float(sn) ** 2, float(mu)


def kuu_factor(kernel, th, Z, jitter, mean):
    Kuu = cross(kernel, th, Z, Z, mean)
    Kuu[np.diag_indices_from(Kuu)] += jitter
    return sla.cholesky(Kuu, lower=True), Kuu


def bound_formulas(kernel, th, X, y, Z, jitter, mean="zero", chunk=None):
    """Route (a).  {"F", "parts" (the order of PARTS), "Lu", "LB", "c"}; chunk: data points per pass (None = all at once)."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64).ravel()
    n, m = len(X), len(Z)
    sn2, mu = noise_and_mean(kernel, th, X.shape[1], mean)
    Lu, _ = kuu_factor(kernel, th, Z, jitter, mean)
    VVt, Vr, rtr, skk = np.zeros((m, m)), np.zeros(m), 0.0, 0.0
    step = n if chunk is None else int(chunk)
    for c0 in range(0, n, step):
        Xc, r = X[c0:c0 + step], y[c0:c0 + step] - mu
        V = sla.solve_triangular(Lu, cross(kernel, th, Z, Xc, mean), lower=True)
        VVt += V @ V.T
        Vr += V @ r
        rtr += float(r @ r)
        skk += float(kdiag(kernel, th, Xc, mean).sum())
    tr = float(np.trace(VVt))
    B = VVt + sn2 * np.eye(m)
    LB = sla.cholesky(B, lower=True)
    c = sla.solve_triangular(LB, Vr, lower=True)
    logdet, ctc = 2.0 * float(np.log(np.diag(LB)).sum()), float(c @ c)
    F = -0.5 * (n * LOG_2PI + (n - m) * np.log(sn2) + logdet + (rtr - ctc) / sn2) - (skk - tr) / (2.0 * sn2)
    return {"F": float(F), "parts": np.array([logdet, ctc, rtr, tr, skk]), "Lu": Lu, "LB": LB, "c": c}


def bound_definition(kernel, th, X, y, Z, jitter, mean="zero"):
    """Route (b): log N(y | m, Q + sn^2 I) - tr(K_ff - Q) / (2 sn^2), Q = K_fu K_uu^-1 K_uf, with an N x N Cholesky."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64).ravel()
    n = len(X)
    sn2, mu = noise_and_mean(kernel, th, X.shape[1], mean)
    Lu, _ = kuu_factor(kernel, th, Z, jitter, mean)
    A = sla.solve_triangular(Lu, cross(kernel, th, Z, X, mean), lower=True)
    Q = A.T @ A
    tr_gap = float((kdiag(kernel, th, X, mean) - np.diag(Q)).sum())
    S = Q + sn2 * np.eye(n)
    L = sla.cholesky(S, lower=True)
    r = y - mu
    z = sla.solve_triangular(L, r, lower=True)
    return float(-0.5 * (n * LOG_2PI + 2.0 * np.log(np.diag(L)).sum() + z @ z) - tr_gap / (2.0 * sn2))


def predict_formulas(kernel, th, X, y, Z, jitter, Xs, mean="zero", latent=False):
    """Route (a): mean = m(x*) + v2^T c, var = k(x*, x*) [+ sn^2] - |v1|^2 + sn^2 |v2|^2."""
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    sn2, mu = noise_and_mean(kernel, th, Xs.shape[1], mean)
    f = bound_formulas(kernel, th, X, y, Z, jitter, mean)
    v1 = sla.solve_triangular(f["Lu"], cross(kernel, th, Z, Xs, mean), lower=True)
    v2 = sla.solve_triangular(f["LB"], v1, lower=True)
    var = kdiag(kernel, th, Xs, mean) + (0.0 if latent else sn2) - (v1 * v1).sum(axis=0) + sn2 * (v2 * v2).sum(axis=0)
    return mu + v2.T @ f["c"], var


def predict_definition(kernel, th, X, y, Z, jitter, Xs, mean="zero", latent=False):
    """Route (b): mean = m(x*) + Q*f (Q + sn^2 I)^-1 r, var = k(x*, x*) [+ sn^2] - Q*f (Q + sn^2 I)^-1 Qf*, Q*f = k(x*, Z) K_uu^-1 K_uf."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64).ravel()
    sn2, mu = noise_and_mean(kernel, th, X.shape[1], mean)
    Lu, _ = kuu_factor(kernel, th, Z, jitter, mean)
    A = sla.solve_triangular(Lu, cross(kernel, th, Z, X, mean), lower=True)
    As = sla.solve_triangular(Lu, cross(kernel, th, Z, Xs, mean), lower=True)
    S = A.T @ A + sn2 * np.eye(len(X))
    Qsf = As.T @ A
    cf = sla.cho_factor(S, lower=True)
    mean_s = mu + Qsf @ sla.cho_solve(cf, y - mu)
    var = kdiag(kernel, th, Xs, mean) + (0.0 if latent else sn2) - np.einsum("ij,ji->i", Qsf, sla.cho_solve(cf, Qsf.T))
    return mean_s, var


def case_theta(d, sn=0.15, sf=1.1, mu=None):
    """SE-ARD hyper-parameters of the pinned cases: l = linspace(0.8, 1.3, d) (d = 1: 0.3), sf, sn [, mu]"""
    ell = np.array([0.3]) if d == 1 else np.linspace(0.8, 1.3, d)
    return np.concatenate([ell, [sf, sn]] + ([[mu]] if mu is not None else []))
