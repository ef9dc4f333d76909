"""numpy float64 references for the JOINT predictive distribution of the sparse inducing-point GP (include/gphip.h
gphip_sparse_predict_cov / _draws / _logpdf), built on tests/sparse_reference.py.  Two algebraically different routes:

  (a) the formulas of the header: V1 = L_u^-1 k(Z, X*), V2 = L_B^-1 V1,
          mu = m(X*) + V2^T c,    Sigma = k(X*, X*) [+ sn^2 I] - V1^T V1 + sn^2 V2^T V2;
  (b) the definition: Q = K_*u K_uu^-1 K_uf dense and an N x N Cholesky of S = Q_ff + sn^2 I,
          mu = m(X*) + Q_*f S^-1 r,    Sigma = k(X*, X*) [+ sn^2 I] - Q_*f S^-1 Q_f*.

K_uu always means k(Z, Z) + jitter I; the jitter is NOT added to k(X*, X*).  Shared by tests/test_sparse_joint.py, which pins the
routes against each other, and tests/test_gpu_sparse_joint.py."""
import functools

import numpy as np
import scipy.linalg as sla

import sparse_reference as ref
from bayesianinference_amd import gaussian_process as gp, synthetic as syn

SF = 1.1
SE_ARD_BODY = "T s = 0; for (int k = 0; k < D; ++k) { const T u = (X(k) - Y(k)) / P(k); s += u * u; } return P(D) * P(D) * exp((T)-0.5 * s);"


def se_ard_fn(A, B, p):
    d = A.shape[-1]
    return p[d] ** 2 * np.exp(-0.5 * (((A - B) / p[:d]) ** 2).sum(-1))


def joint_formulas(kernel, th, X, y, Z, jitter, Xs, mean="zero", latent=False):
    """Route (a): (mu [M], Sigma [M, M])."""
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    sn2, mu = ref.noise_and_mean(kernel, th, Xs.shape[1], mean)
    f = ref.bound_formulas(kernel, th, X, y, Z, jitter, mean)
    V1 = sla.solve_triangular(f["Lu"], ref.cross(kernel, th, Z, Xs, mean), lower=True)
    V2 = sla.solve_triangular(f["LB"], V1, lower=True)
    S = ref.cross(kernel, th, Xs, Xs, mean) - V1.T @ V1 + sn2 * (V2.T @ V2)
    if not latent:
        S[np.diag_indices_from(S)] += sn2
    return mu + V2.T @ f["c"], 0.5 * (S + S.T)


def joint_definition(kernel, th, X, y, Z, jitter, Xs, mean="zero", latent=False):
    """Route (b): (mu [M], Sigma [M, M]) with an N x N Cholesky."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64).ravel()
    sn2, mu = ref.noise_and_mean(kernel, th, X.shape[1], mean)
    Lu, _ = ref.kuu_factor(kernel, th, Z, jitter, mean)
    A = sla.solve_triangular(Lu, ref.cross(kernel, th, Z, X, mean), lower=True)
    As = sla.solve_triangular(Lu, ref.cross(kernel, th, Z, Xs, mean), lower=True)
    cf = sla.cho_factor(A.T @ A + sn2 * np.eye(len(X)), lower=True)
    Qsf = As.T @ A
    S = ref.cross(kernel, th, Xs, Xs, mean) - Qsf @ sla.cho_solve(cf, Qsf.T)
    if not latent:
        S[np.diag_indices_from(S)] += sn2
    return mu + Qsf @ sla.cho_solve(cf, y - mu), 0.5 * (S + S.T)


# (label, N, d, m, M, kernel name, mean): the cases of the device test's comparison against the reference -- one tile, a ragged
# second tile row, a third tile row with a true off-diagonal tile, m_pad = 128 (the segment boundary after one tile column),
# m_pad = 256 -- and the shapes of its other tests
CASES = [("one-tile", 700, 3, 60, 1, "se_ard", "zero"), ("ragged", 700, 3, 60, 130, "se_ard", "zero"),
         ("three-rows", 700, 3, 60, 257, "se_ard", "zero"), ("const-mean", 900, 2, 130, 257, "se_ard", "const"),
         ("matern", 1500, 2, 200, 300, "matern52_ard", "zero"), ("composed", 700, 2, 60, 130, "se_ard+const", "zero"),
         ("custom", 700, 3, 60, 130, "custom", "zero")]
STRIPS = ("strips", 2000, 3, 300, 130, "se_ard", "zero")
DRAWS = ("draws", 900, 2, 130, 64, "se_ard", "zero")


def kernel_of(name, d):
    from bayesianinference_amd import _lib
    return _lib.CustomKernel(SE_ARD_BODY, d + 1, fn=se_ard_fn) if name == "custom" else name


def theta_of(name, d, mean):
    """sparse_reference.case_theta for the SE-ARD-shaped kernels; `se_ard+const` appends its constant's amplitude before sn"""
    mu = 0.2 if mean == "const" else None
    th = ref.case_theta(d, sf=SF, mu=mu)
    if name == "se_ard+const":
        th = np.concatenate([th[:d + 1], [0.3], th[d + 1:]])
    return th


@functools.lru_cache(maxsize=None)
def case_data(n, d, m, M, name, mean):
    """(X, y, Z, Xs, ys, kernel, theta, jitter) of a case; computed once and shared, never modified"""
    X, y = syn.make_dataset(n, d)
    Xs = syn.make_test_points(M, d)
    ys = syn.make_outputs(Xs)
    Z = gp.selectInducingPoints(X, m, seed=1)
    for a in (X, y, Z, Xs, ys):
        a.setflags(write=False)
    return X, y, Z, Xs, ys, kernel_of(name, d), theta_of(name, d, mean), 1e-8 * SF ** 2


@functools.lru_cache(maxsize=None)
def case_reference(n, d, m, M, name, mean, latent=False):
    """route (a) of a case, computed once"""
    X, y, Z, Xs, _, kernel, th, jit = case_data(n, d, m, M, name, mean)
    mu, S = joint_formulas(kernel, th, X, y, Z, jit, Xs, mean, latent)
    mu.setflags(write=False)
    S.setflags(write=False)
    return mu, S
