"""Fixture of the sparse prediction-gradient tests (CPU only; run from the repository root):

    python scripts/make_predict_grad_golden.py      -> tests/golden/predict_grad_mpmath.npz

The default-jitter case of tests/test_gpu_sparse_predict_grad.py -- SE, d = 1, N = 300, m = 40, M = 130, jitter = 1e-10 k(x, x),
cond(K_uu) ~ 1e10 -- evaluated a second time by the formulas of include/gphip.h (gphip_sparse_predict_grad) in 30-digit mpmath:
hand-written Cholesky and substitutions on plain lists, the kernel's derivative written out.  Stored: dmean and dvar rounded to
float64, cond(K_uu), and the disagreement of the float64 reference (tests/predict_grad_reference.sparse) with them, which sets
the device's bar (10 x that: the device cannot be asked to beat the arithmetic it shares).  np.longdouble stands in where
mpmath is not importable (the file then says so in "arithmetic")."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import predict_grad_reference as pg  # noqa: E402
import sparse_reference as ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "predict_grad_mpmath.npz")
CASE = ("se", 1, "zero")               # pg.CASES[0]


def mp_gradients(X, y, Z, Xs, th, jitter, dps=30):
    """(dmean, dvar) [M][d] as nested lists of mpf: SE with one length scale, zero mean"""
    import mpmath as mp
    mp.mp.dps = dps
    n, d, m = len(X), X.shape[1], len(Z)
    f = lambda v: mp.mpf(float(v))                                  # noqa: E731
    ell, sf, sn = f(th[0]), f(th[1]), f(th[2])
    sn2 = sn * sn

    def k(a, b):
        r2 = sum(((f(a[j]) - f(b[j])) / ell) ** 2 for j in range(d))
        return sf * sf * mp.exp(-r2 / 2)

    def cholesky(L):
        for j in range(len(L)):
            Lj = L[j]
            dj = mp.sqrt(Lj[j] - mp.fdot(Lj[:j], Lj[:j]))
            Lj[j] = dj
            for i in range(j + 1, len(L)):
                L[i][j] = (L[i][j] - mp.fdot(L[i][:j], Lj[:j])) / dj
        return L

    def forward(L, b):                                              # L z = b
        z = [None] * len(L)
        for i in range(len(L)):
            z[i] = (b[i] - mp.fdot(L[i][:i], z[:i])) / L[i][i]
        return z

    def backward(L, b):                                             # L^T z = b
        z = [None] * len(L)
        for i in reversed(range(len(L))):
            z[i] = (b[i] - sum(L[j][i] * z[j] for j in range(i + 1, len(L)))) / L[i][i]
        return z

    Lu = [[k(Z[i], Z[j]) for j in range(i + 1)] for i in range(m)]
    for i in range(m):
        Lu[i][i] += f(jitter)
    cholesky(Lu)
    cols = [forward(Lu, [k(Z[i], X[t]) for i in range(m)]) for t in range(n)]
    rows = [[cols[t][i] for t in range(n)] for i in range(m)]
    r = [f(v) for v in y]
    B = [[mp.fdot(rows[i], rows[j]) for j in range(i + 1)] for i in range(m)]
    for i in range(m):
        B[i][i] += sn2
    cholesky(B)
    c = forward(B, [mp.fdot(rows[i], r) for i in range(m)])
    a_mu = backward(Lu, backward(B, c))
    dmean, dvar = [], []
    for p in Xs:
        ks = [k(Z[i], p) for i in range(m)]
        v1 = forward(Lu, ks)
        v2 = forward(B, v1)
        lb = backward(B, v2)
        W = backward(Lu, [v1[i] - sn2 * lb[i] for i in range(m)])
        dk = [[-ks[i] * (f(p[j]) - f(Z[i][j])) / (ell * ell) for j in range(d)] for i in range(m)]
        dmean.append([mp.fdot(a_mu, [dk[i][j] for i in range(m)]) for j in range(d)])
        dvar.append([-2 * mp.fdot(W, [dk[i][j] for i in range(m)]) for j in range(d)])
    return dmean, dvar


def longdouble_gradients(X, y, Z, Xs, th, jitter):
    """the same in np.longdouble (where mpmath is missing): dense Cholesky by hand"""
    ld = np.longdouble
    X, y, Z, Xs = (np.asarray(a, dtype=ld) for a in (X, y, Z, Xs))
    ell, sf, sn2 = ld(th[0]), ld(th[1]), ld(th[2]) ** 2

    def kern(A, Bp):
        return sf * sf * np.exp(-(((A[:, None, :] - Bp[None, :, :]) / ell) ** 2).sum(2) / 2)

    def chol(A):
        L = np.zeros_like(A)
        for j in range(len(A)):
            L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        return L

    def fwd(L, Bm):
        out = np.zeros_like(Bm)
        for i in range(len(L)):
            out[i] = (Bm[i] - L[i, :i] @ out[:i]) / L[i, i]
        return out

    def bwd(L, Bm):
        out = np.zeros_like(Bm)
        for i in reversed(range(len(L))):
            out[i] = (Bm[i] - L[i + 1:, i] @ out[i + 1:]) / L[i, i]
        return out
    m = len(Z)
    Lu = chol(kern(Z, Z) + ld(jitter) * np.eye(m, dtype=ld))
    V = fwd(Lu, kern(Z, X))
    LB = chol(V @ V.T + sn2 * np.eye(m, dtype=ld))
    c = fwd(LB, (V @ y)[:, None])
    a_mu = bwd(Lu, bwd(LB, c))[:, 0]
    ks = kern(Z, Xs)
    v1 = fwd(Lu, ks)
    W = bwd(Lu, v1 - sn2 * bwd(LB, fwd(LB, v1)))
    dk = -ks[:, :, None] * (Xs[None, :, :] - Z[:, None, :]) / (ell * ell)          # [m, M, d]
    return np.einsum("k,ktc->tc", a_mu, dk), -2 * np.einsum("kt,ktc->tc", W, dk)


def main():
    name, d, mean = CASE
    c = pg.sparse_case_reference(name, d, mean, pg.SPARSE_M, None)
    _, Kuu = ref.kuu_factor(name, c["theta"], c["Z"], c["jitter"], mean)
    cond = float(np.linalg.cond(Kuu))
    try:
        import mpmath  # noqa: F401
        dm, dv = mp_gradients(c["X"], c["y"], c["Z"], c["Xs"], c["theta"], c["jitter"])
        dm = np.array([[float(v) for v in row] for row in dm])
        dv = np.array([[float(v) for v in row] for row in dv])
        arithmetic = "mpmath, 30 digits"
    except ImportError:
        dm, dv = (np.asarray(a, dtype=np.float64) for a in longdouble_gradients(c["X"], c["y"], c["Z"], c["Xs"], c["theta"], c["jitter"]))
        arithmetic = "numpy longdouble"
    em = float(np.abs(c["dmean"] - dm).max() / np.abs(dm).max())
    ev = float(np.abs(c["dvar"] - dv).max() / np.abs(dv).max())
    print(f"{arithmetic}: cond(K_uu) = {cond:.3e}, jitter = {c['jitter']:.3e}; the float64 reference differs by {em:.3e} (dmean) "
          f"{ev:.3e} (dvar) of max |.|")
    np.savez(GOLDEN, dmean=dm, dvar=dv, cond_kuu=np.array(cond), jitter=np.array(c["jitter"]), float64_dmean_error=np.array(em),
             float64_dvar_error=np.array(ev), arithmetic=np.array(arithmetic), kernel=np.array(name), d=np.array(d), m=np.array(pg.SPARSE_M))


if __name__ == "__main__":
    main()
