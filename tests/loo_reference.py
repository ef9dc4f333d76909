"""numpy references for leave-one-out cross-validation (Rasmussen & Williams, GPML §5.4.2), built from the CPU oracle's covariance.
Shared by tests/test_loo.py (which pins them against brute-force refits and finite differences) and tests/test_gpu_loo.py."""
import numpy as np
import scipy.linalg as sla

from oracle import gp_oracle as orc

LOG_2PI = float(np.log(2.0 * np.pi))


def covariance(kernel, th, X, mean):
    K = orc.covariance_matrix(kernel, th, X, mean)
    return np.diag(K) if K.ndim == 1 else K               # (the null kernel comes back as its diagonal)


def loo_closed_form(kernel, th, X, y, mean="const"):
    """{"mean", "var", "logp", "total"} from ONE inverse: mu_-i = y_i - alpha_i / k_i, var_-i = 1 / k_i."""
    K = covariance(kernel, th, X, mean)
    r = orc.residual(kernel, th, X, y, mean)
    L = sla.cholesky(K, lower=True)
    Linv = sla.solve_triangular(L, np.eye(len(K)), lower=True)
    k = (Linv * Linv).sum(axis=0)                          # diag(K^-1) = column norms of L^-1
    alpha = sla.cho_solve((L, True), r)
    logp = 0.5 * np.log(k) - 0.5 * alpha * alpha / k - 0.5 * LOG_2PI
    return {"mean": np.asarray(y, dtype=np.float64).ravel() - alpha / k, "var": 1.0 / k, "logp": logp, "total": float(logp.sum())}


def loo_brute_force(kernel, th, X, y, mean="const"):
    """The definition: every point predicted from a fresh Cholesky of the other N - 1 (noisy-observation variance)."""
    K = covariance(kernel, th, X, mean)
    r = orc.residual(kernel, th, X, y, mean)
    y = np.asarray(y, dtype=np.float64).ravel()
    n = len(K)
    mu, var = np.zeros(n), np.zeros(n)
    for i in range(n):
        keep = np.arange(n) != i
        c = sla.cho_factor(K[np.ix_(keep, keep)], lower=True)
        kv = K[keep, i]
        mu[i] = (y[i] - r[i]) + kv @ sla.cho_solve(c, r[keep])
        var[i] = K[i, i] - kv @ sla.cho_solve(c, kv)
    logp = -0.5 * np.log(var) - 0.5 * (y - mu) ** 2 / var - 0.5 * LOG_2PI
    return {"mean": mu, "var": var, "logp": logp, "total": float(logp.sum())}


def loo_grad_formula(kernel, th, X, y, mean="const"):
    """dL_LOO/dtheta by the regrouped form of R&W eq. 5.13:  1/2 sum_ab (alpha_a beta_b + beta_a alpha_b - M_ab) dK_ab/dtheta_j
    with g = alpha / k, beta = K^-1 g, c = 1 / k + g^2, M = K^-1 diag(c) K^-1; d/dmu = sum beta.  dK/dtheta_j: 4th-order central
    differences of the oracle's covariance matrix (entries are smooth in theta: error ~1e-11 relative)."""
    th = np.asarray(th, dtype=np.float64)
    K = covariance(kernel, th, X, mean)
    r = orc.residual(kernel, th, X, y, mean)
    Kinv = np.linalg.inv(K)
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha, k = Kinv @ r, np.diag(Kinv)
    g = alpha / k
    beta = Kinv @ g
    W = np.outer(alpha, beta) + np.outer(beta, alpha) - (Kinv * (1.0 / k + g * g)) @ Kinv
    nk = len(th) - (1 if mean == "const" else 0)
    grad = np.zeros(len(th))
    for j in range(nk):
        h = 1e-3 * max(abs(th[j]), 0.1)

        def Kat(t):
            tt = th.copy()
            tt[j] += t
            return covariance(kernel, tt, X, mean)
        dK = (-Kat(2 * h) + 8.0 * Kat(h) - 8.0 * Kat(-h) + Kat(-2 * h)) / (12.0 * h)
        grad[j] = 0.5 * float(np.sum(W * dK))
    if mean == "const":
        grad[-1] = float(beta.sum())
    return grad


def device_total(logp):
    """The documented summation order of gphip_loo's *out (include/gphip.h): partial sum t of 1024 adds logp[t], logp[t + 1024], ..
    in order, then a binary tree p[t] += p[t + off], off = 512 .. 1."""
    v = np.zeros((-(-len(logp) // 1024)) * 1024)
    v[:len(logp)] = logp
    p = np.zeros(1024)
    for row in v.reshape(-1, 1024):
        p = p + row
    off = 512
    while off >= 1:
        p = p[:off] + p[off:2 * off]
        off //= 2
    return float(p[0])
