"""float64 numpy reference for the pathwise posterior function draws (include/gphip.h gphip_paths_create / gphip_paths_eval),
built on tests/predict_grad_reference.py (kernels, cases, data).  Given the table (omega, phase, amp) and the draw (w, eps):

    f~_s(x) = sum_j a_j w_sj cos(Omega_j . x + b_j)
    v_s     = K^-1 (y - m - f~_s(X) - eps_s)
    f_s(x)  = m + f~_s(x) + k(x, X) v_s                 df_s/dx = -sum_j a_j w_sj sin(..) Omega_j + sum_i v_si dk(x, x_i)/dx

and the exact linear-Gaussian moments of f_s(X*) over (w, eps) for a FIXED table:  with Phi(X) = [a_j cos(Omega_j . x + b_j)],
G = k* K^-1, A = Phi(X*) - G Phi(X), B = -G:  f_s = m + G (y - m) + A w_s + B eps_s,  cov = A A^T + sn^2 B B^T.

dtype = np.float32 evaluates the same formulas in float32 arithmetic (the inputs rounded to float32, every product and the
solve in float32): the yardstick of the fp32 handles' test, measured against the float64 evaluation, never against the device."""
import numpy as np
import scipy.linalg as sla

import predict_grad_reference as pg
import sparse_reference as ref
import sparse_zgrad_reference as zg
from oracle import gp_oracle as orc


RFF_KEY = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1
TAG_DIRECTION, TAG_RADIAL, TAG_PHASE, TAG_EPS = 0, 1, 8, 9      # (+ 4 for the second term of a sum or product)


def rff_key(seed, tag):
    """the Philox key of stream `tag` of the feature table (csrc/gphip_hostlogic.inc); gphip_paths_create draws eps under TAG_EPS"""
    return (int(seed) ^ (RFF_KEY * (tag + 1))) & MASK64


def _philox4x32(key, c0, c1, c2):
    """Philox4x32-10 (Salmon et al., SC'11) written from the paper: counter (c0, c1, c2, 0), 64-bit key; four uint64 arrays that
    hold 32-bit words"""
    lo = np.uint64(0xFFFFFFFF)
    c0, c1 = np.broadcast_arrays(np.asarray(c0, dtype=np.uint64), np.asarray(c1, dtype=np.uint64))
    c2, c3 = np.full(c0.shape, c2, dtype=np.uint64), np.zeros(c0.shape, dtype=np.uint64)
    k0, k1 = int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & lo, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & lo
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox_normal(key, s, j):
    """the library's standard normal of (key, s, j): counter (j, s, "JOIN", 0), Box-Muller from two 53-bit uniforms.  s and j
    broadcast.  Equal to the library's value up to the rounding of log, sqrt and cos (a few ulp), not bit for bit."""
    c0, c1, c2, c3 = _philox4x32(key, j, s, 0x4A4F494E)
    a, b = ((c0 << np.uint64(32)) | c1) >> np.uint64(11), ((c2 << np.uint64(32)) | c3) >> np.uint64(11)
    u1, u2 = (a.astype(np.float64) + 0.5) * 2.0 ** -53, b.astype(np.float64) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def philox_uniform(key, s, j):
    """the library's uniform on [0, 1) of (key, s, j): counter (j, s, "UNIF", 0), the first output word (exact)"""
    return _philox4x32(key, j, s, 0x554E4946)[0].astype(np.float64) * 2.0 ** -32


def features(table, X, dtype=np.float64):
    """Phi(X)[i, j] = a_j cos(Omega_j . x_i + b_j)  and the phases"""
    om, b, a = (np.asarray(table[k], dtype=dtype) for k in ("omega", "phase", "amp"))
    ph = np.asarray(X, dtype=dtype) @ om.T + b
    return a * np.cos(ph), ph


def paths(kernel, th, X, y, Xs, table, w, eps, mean="zero", dtype=np.float64, grad=True):
    """{"v" [S, N], "out" [S, M], "dout" [S, M, d]}"""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    th = np.asarray(th, dtype=np.float64)
    mu = ref.noise_and_mean(kernel, th, X.shape[1], mean)[1]
    K = orc.covariance_matrix(kernel, th, X, mean).astype(dtype)
    ks = ref.cross(kernel, th, Xs, X, mean).astype(dtype)                       # M x N
    w, eps = np.asarray(w, dtype=dtype), np.asarray(eps, dtype=dtype)
    PhiX, _ = features(table, X, dtype)
    PhiS, phS = features(table, Xs, dtype)
    r = (np.asarray(y, dtype=np.float64) - mu).astype(dtype)
    R = r[None, :] - w @ PhiX.T - eps                                           # S x N
    v = sla.cho_solve(sla.cho_factor(K, lower=True), R.T).T.astype(dtype)
    out = (dtype(mu) + w @ PhiS.T + v @ ks.T).astype(dtype)
    res = {"v": v, "out": out}
    if grad:
        om, a = np.asarray(table["omega"], dtype=dtype), np.asarray(table["amp"], dtype=dtype)
        dPhi = -(a * np.sin(phS))[:, :, None] * om[None, :, :]                  # M x Ftot x d
        dk = zg.dk_da(kernel, th, Xs, X, mean).astype(dtype)                    # M x N x d
        res["dout"] = (np.einsum("sj,tjc->stc", w, dPhi) + np.einsum("si,tic->stc", v, dk)).astype(dtype)
    return res


def moments(kernel, th, X, y, Xs, table, mean="zero"):
    """{"mean" [M], "cov" [M, M], "A" [M, Ftot], "B" [M, N], "sn2", "mu"}: exact over (w, eps) for the given table"""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    th = np.asarray(th, dtype=np.float64)
    sn2, mu = ref.noise_and_mean(kernel, th, X.shape[1], mean)
    K = orc.covariance_matrix(kernel, th, X, mean)
    ks = ref.cross(kernel, th, Xs, X, mean)
    G = sla.cho_solve(sla.cho_factor(K, lower=True), ks.T).T                    # M x N
    A = features(table, Xs)[0] - G @ features(table, X)[0]
    B = -G
    return {"mean": mu + G @ (np.asarray(y, dtype=np.float64) - mu), "cov": A @ A.T + sn2 * B @ B.T, "A": A, "B": B, "sn2": sn2, "mu": mu}


def exact_latent_cov(kernel, th, X, Xs, mean="zero"):
    """the latent posterior covariance of the exact GP: k** - k* K^-1 k*^T"""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    K = orc.covariance_matrix(kernel, th, X, mean)
    ks = ref.cross(kernel, th, Xs, X, mean)
    return ref.cross(kernel, th, Xs, Xs, mean) - ks @ sla.cho_solve(sla.cho_factor(K, lower=True), ks.T)


def kernel_of_offsets(kernel, th, delta, mean="zero"):
    """k(delta_i, 0) without the nugget"""
    delta = np.atleast_2d(np.asarray(delta, dtype=np.float64))
    return ref.cross(kernel, th, delta, np.zeros((1, delta.shape[1])), mean)[:, 0]


CASES = pg.CASES
case_id = pg.case_id
case_reference = pg.case_reference
