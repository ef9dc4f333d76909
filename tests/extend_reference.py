"""float64 CPU statement of what gphip_extend assembles (include/gphip.h), on oracle/gp_oracle.py.

With K = L L^T the covariance of the N old points, k = k(X, X_new), V = L^-1 k, z = L^-1 (y - m) and
Sigma = k(X_new, X_new) + sn^2 I - V^T V = L_S L_S^T, the factor of the covariance K' of the N + M points [X; X_new] is

    L' = [ L    0   ]      z' = [ z ; L_S^-1 (y_new - mu) ]      log det K' = log det K + log det Sigma
         [ V^T  L_S ]      mu = m + V^T z  (the predictive mean at X_new)

assembled(..) builds the right-hand sides from the parts, direct(..) factors K' itself; tests/test_extend.py holds them together.
reference(..) is the numpy reference of tests/test_gpu_predict_joint.py, which the device tests apply to the concatenated data.
pivot_cholesky(..) is a Cholesky under the library's pivot rule: a pivot that is not above 64 eps (k(x, x) + sn^2) fails."""
import numpy as np
import scipy.linalg as sla

from bayesianinference_amd import _lib, synthetic as syn
from oracle import gp_oracle as orc

SE_ARD_BODY = "T s = 0; for (int k = 0; k < D; ++k) { const T u = (X(k) - Y(k)) / P(k); s += u * u; } return P(D) * P(D) * exp((T)-0.5 * s);"
EPS = {64: 2.220446049250313e-16, 32: 1.1920929e-07}

# (N, M) of the device tests: rows offset 44 inside a tile and new rows over two tile rows; an aligned N whose one new point opens
# a tile row; no new tile row; one point in the old last tile and one in a new one
SHAPES = [(300, 130), (256, 1), (300, 1), (383, 2)]
CHAIN = (255, 3)                       # three single-point extensions, 255 -> 258: crosses a tile boundary
# (kernel, d, mean) at (300, 130)
KERNELS = [("se_ard", 3, "zero"), ("se_ard", 3, "const"), ("matern52_ard", 8, "zero"), ("se_ard+const", 2, "zero"), ("custom", 3, "zero")]


def se_ard_fn(A, B, p):
    d = A.shape[-1]
    return p[d] ** 2 * np.exp(-0.5 * (((A - B) / p[:d]) ** 2).sum(-1))


def kernel_of(kname, d):
    return _lib.CustomKernel(SE_ARD_BODY, d + 1, fn=se_ard_fn) if kname == "custom" else kname


def theta_of(kname, d, mean="zero"):
    base = syn.default_theta("se_ard", d)           # [l.., sf, sn]
    th = np.concatenate([base[:-1], [0.3], base[-1:]]) if kname == "se_ard+const" else base
    return np.concatenate([th, [0.2]]) if mean == "const" else th


def case_data(n, m, d, m_test=40):
    """(X, y, X_new, y_new, Xs): n training points, m new observations and m_test test points, all distinct, seeded"""
    X, y = syn.make_dataset(n, d)
    Xn = syn.make_test_points(m, d)
    yn = syn.make_outputs(Xn, row0=n)
    Xs = syn.make_inputs(m_test, d, stream=syn.STREAM_TEST, row0=100000)
    return X, y, Xn, yn, Xs


def _kss(kernel, th, Xs, mean):
    if orc.is_custom(kernel):
        return orc.custom_kernel_matrix(kernel, th, Xs, Xs)
    return orc.general_kernel_matrix(kernel, th, Xs, Xs, mean)


def reference(kernel, th, X, y, Xs, mean="zero"):
    """(mu, Sigma of noisy observations, sn^2) in numpy: Cholesky of K, V = L^-1 k."""
    K = orc.covariance_matrix(kernel, th, X, mean)
    k, _ = orc.k_and_kappa(kernel, th, X, Xs, mean)
    _, _, sn, mu0 = orc.split_theta(kernel, X.shape[1], th, mean)
    r = orc.residual(kernel, th, X, y, mean)
    L = sla.cholesky(K, lower=True, overwrite_a=True)
    V = sla.solve_triangular(L, k, lower=True)
    z = sla.solve_triangular(L, r, lower=True)
    S = _kss(kernel, th, Xs, mean) - V.T @ V
    S[np.diag_indices_from(S)] += sn * sn
    return mu0 + V.T @ z, S, sn * sn


def pivot_tolerance(kxx, sn2, dtype=64):
    return 64.0 * EPS[dtype] * (abs(kxx) + sn2)


def pivot_cholesky(A, tol):
    """(L, info): right-looking Cholesky of the lower triangle; info = 1 as soon as a pivot is not above tol (the rule of the
    device's factorisation kernels), L is then void."""
    A = np.array(A, dtype=np.float64)
    n = len(A)
    for j in range(n):
        if not A[j, j] > tol:
            return None, 1
        A[j, j] = np.sqrt(A[j, j])
        A[j + 1:, j] /= A[j, j]
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    return np.tril(A), 0


def assembled(kernel, th, X, y, Xn, yn, mean="zero"):
    """{"L", "z", "logdet", "logp", "info"} of the N + M points from the parts, as gphip_extend puts them together"""
    K = orc.covariance_matrix(kernel, th, X, mean)
    L = sla.cholesky(K, lower=True)
    z = sla.solve_triangular(L, orc.residual(kernel, th, X, y, mean), lower=True)
    mu, S, sn2 = reference(kernel, th, X, y, Xn, mean)
    V = sla.solve_triangular(L, orc.k_and_kappa(kernel, th, X, Xn, mean)[0], lower=True)
    LS, info = pivot_cholesky(S, pivot_tolerance(_kss(kernel, th, Xn[:1], mean)[0, 0], sn2))
    if info:
        return {"info": info}
    zn = sla.solve_triangular(LS, yn - mu, lower=True)
    n, m = len(X), len(Xn)
    Lp = np.zeros((n + m, n + m))
    Lp[:n, :n], Lp[n:, :n], Lp[n:, n:] = L, V.T, LS
    ld_s = 2.0 * np.log(np.diag(LS)).sum()
    return {"L": Lp, "z": np.concatenate([z, zn]), "logdet": 2.0 * np.log(np.diag(L)).sum() + ld_s,
            "logp": -0.5 * (m * np.log(2.0 * np.pi) + ld_s + zn @ zn), "info": 0}


def direct(kernel, th, X, y, Xn, yn, mean="zero"):
    """the same from scipy's Cholesky of the oracle's K on the concatenated data, and the two log likelihoods"""
    Xc, yc = np.vstack([X, Xn]), np.concatenate([y, yn])
    L = sla.cholesky(orc.covariance_matrix(kernel, th, Xc, mean), lower=True)
    z = sla.solve_triangular(L, orc.residual(kernel, th, Xc, yc, mean), lower=True)
    return {"L": L, "z": z, "logdet": 2.0 * np.log(np.diag(L)).sum(),
            "loglik": orc.log_likelihood(kernel, th, Xc, yc, mean), "loglik_parent": orc.log_likelihood(kernel, th, X, y, mean)}


def refusal_case():
    """Sigma that the pivot rule refuses while the parent factors: N = 64 points on a d = 1 grid with spacing 50 l (K = I to the
    last bit), SE with sf = 1, sn = 1e-9, and the same far-away new point twice: the second pivot of Sigma is 2e-18 in exact
    arithmetic (0 in fp64), under 64 eps (sf^2 + sn^2) = 1.4e-14.  (kernel, mean, theta, X, y, X_new, y_new)"""
    X = 50.0 * np.arange(64, dtype=np.float64)[:, None]
    y = syn.make_outputs(X / 3200.0)
    Xn = np.array([[-1000.0], [-1000.0]])
    return "se", "zero", np.array([1.0, 1.0, 1e-9]), X, y, Xn, np.array([0.1, -0.2])
