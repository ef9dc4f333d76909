"""float64 CPU references for the gradient of the sparse GP bound F in the inducing LOCATIONS Z (include/gphip.h
gphip_sparse_bound_grad_inducing), built on tests/sparse_reference.py and tests/sparse_grad_reference.py.  Three routes:

  analytic(...)      numpy: the header's formula with G and H built as sparse_grad_reference.analytic builds them,

      dF/dz_k = sum_i G_ki dk(z_k, x_i)/dz_k + 2 sum_l H_kl dk(z_k, z_l)/dz_k
      dk(a, b)/da_c = -sf^2 m2dg(r^2) (a_c - b_c) / l_c^2  per term,  m2dg = -2 dg/dr^2;  sums / products by the product rule

                     for every named family and composed form (any kernel of the oracle's grammar);
  autograd(...)      torch float64 on the CPU: reverse-mode differentiation of the bound restated in torch -- it shares no
                     derivative formula with the first route;
  differences(...)   4th-order central differences of sparse_reference.bound_formulas in single entries of Z (a sanity check:
                     the quotient is limited by F's own rounding at cond(K_uu) up to ~5e8).

The jitter is held fixed in all three."""
import math

import numpy as np
import scipy.linalg as sla

import sparse_grad_reference as sg
import sparse_reference as ref
from oracle import gp_oracle as orc

# the nine pinned cases with a named or composed kernel (the run-time compiled ones have no gradient in Z)
CASES = [c for c in sg.CASES if c[0] not in ("custom", "nonstat")]


def _family(term):
    return term[:-4] if term.endswith("_ard") else term


def _g_m2dg(term, r2, alpha):
    """g(r2) and m2dg(r2) = -2 dg/dr2 of one family (next to sparse_grad_reference._dk, which has the length-scale derivatives)"""
    fam = _family(term)
    if fam == "se":
        g = np.exp(-0.5 * r2)
        return g, g
    if fam == "matern52":
        s5 = np.sqrt(5.0 * r2)
        e = np.exp(-s5)
        return (1.0 + s5 + 5.0 / 3.0 * r2) * e, (5.0 / 3.0) * (1.0 + s5) * e
    if fam == "matern32":
        s3 = np.sqrt(3.0 * r2)
        e = np.exp(-s3)
        return (1.0 + s3) * e, 3.0 * e
    if fam == "rq":
        q = r2 / (2.0 * alpha)
        g = np.power(1.0 + q, -alpha)
        return g, g / (1.0 + q)
    raise ValueError(term)


def dk_da(kernel, th, A, B, mean="zero"):
    """d k(a_i, b_j) / d a_i for all pairs: [na, nb, d]"""
    A = np.atleast_2d(np.asarray(A, dtype=np.float64))
    B = np.atleast_2d(np.asarray(B, dtype=np.float64))
    terms, op, _, _, _ = orc.split_general(kernel, A.shape[1], th, mean)
    ks, ds = [], []
    for t, ell, alpha, sf in terms:
        diff = A[:, None, :] - B[None, :, :]
        r2 = ((diff / ell) ** 2).sum(axis=2)
        g, m2dg = _g_m2dg(t, r2, alpha)
        ks.append(sf * sf * g)
        ds.append(-(sf * sf * m2dg)[:, :, None] * diff / ell ** 2)
    if op is None:
        return ds[0]
    if op == "+":
        return ds[0] + ds[1]
    return ds[0] * ks[1][:, :, None] + ds[1] * ks[0][:, :, None]


def weights(kernel, th, X, y, Z, jitter, mean="zero"):
    """G (m x N) and H (m x m) of the header, by substitutions with L_u as sparse_grad_reference.analytic"""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    y = np.asarray(y, dtype=np.float64).ravel()
    m = len(Z)
    sn2, mu = ref.noise_and_mean(kernel, th, X.shape[1], mean)
    f = ref.bound_formulas(kernel, th, X, y, Z, jitter, mean)
    Lu, LB, c = f["Lu"], f["LB"], f["c"]
    r = y - mu
    fwd = lambda M: sla.solve_triangular(Lu, M, lower=True)                 # noqa: E731
    bwd = lambda M: sla.solve_triangular(Lu, M, lower=True, trans="T")      # noqa: E731
    V = fwd(ref.cross(kernel, th, Z, X, mean))
    a = sla.solve_triangular(LB, c, lower=True, trans="T")
    Binv = sla.cho_solve((LB, True), np.eye(m))
    B = V @ V.T + sn2 * np.eye(m)
    w = (r - V.T @ a) / sn2
    D = np.eye(m) / sn2 - Binv
    G = bwd(D @ V + np.outer(a, w))
    inner = np.eye(m) - 0.5 * sn2 * Binv - 0.5 * np.outer(a, a) - B / (2.0 * sn2)
    H = bwd(bwd(inner).T)
    return G, H, f["F"]


def analytic(kernel, th, X, y, Z, jitter, mean="zero"):
    """dF/dZ [m, d]"""
    th = np.asarray(th, dtype=np.float64)
    G, H, _ = weights(kernel, th, X, y, Z, jitter, mean)
    return (np.einsum("ki,kij->kj", G, dk_da(kernel, th, Z, X, mean)) +
            2.0 * np.einsum("kl,klj->kj", H, dk_da(kernel, th, Z, Z, mean)))


def differences(kernel, th, X, y, Z, jitter, mean, entries):
    """{(k, c): dF/dz_kc} by 4th-order central differences of bound_formulas, step 1e-3 max(|z_kc|, 0.1)"""
    out = {}
    for (k, c) in entries:
        h = 1e-3 * max(abs(Z[k, c]), 0.1)

        def f(t):
            Q = Z.copy()
            Q[k, c] += t
            return ref.bound_formulas(kernel, th, X, y, Q, jitter, mean)["F"]
        out[(k, c)] = (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)
    return out


# ---- the independent route: the bound restated in torch float64, differentiated by autograd ----
def _torch_kernel(kernel, d, th, A, B, mean):
    import torch
    terms, op, offset = orc.parse_kernel(kernel)
    o, ks = 0, []
    for t in terms:
        nl = orc.n_lengthscales(t, d)
        ell = th[o:o + nl]
        o += nl
        alpha = None
        if t.startswith("rq"):
            alpha = th[o]
            o += 1
        sf = th[o]
        o += 1
        r2 = (((A[:, None, :] - B[None, :, :]) / ell) ** 2).sum(2)
        fam = _family(t)
        if fam == "se":
            g = torch.exp(-0.5 * r2)
        elif fam == "matern52":
            s5 = torch.sqrt(5.0 * r2 + 1e-300)          # (the square root's derivative at r = 0)
            g = (1.0 + s5 + 5.0 / 3.0 * r2) * torch.exp(-s5)
        elif fam == "matern32":
            s3 = torch.sqrt(3.0 * r2 + 1e-300)
            g = (1.0 + s3) * torch.exp(-s3)
        else:
            g = torch.pow(1.0 + r2 / (2.0 * alpha), -alpha)
        ks.append(sf * sf * g)
    K = ks[0] if op is None else (ks[0] + ks[1] if op == "+" else ks[0] * ks[1])
    if offset:
        K = K + th[o]
        o += 1
    sn = th[o]
    mu = th[o + 1] if mean == "const" else 0.0
    return K, sn, mu


def autograd(kernel, th, X, y, Z, jitter, mean="zero"):
    """(F, dF/dtheta, dF/dZ) from torch's reverse mode on the CPU"""
    import torch
    X = torch.tensor(np.atleast_2d(np.asarray(X, dtype=np.float64)))
    y = torch.tensor(np.asarray(y, dtype=np.float64).ravel())
    Zt = torch.tensor(np.atleast_2d(np.asarray(Z, dtype=np.float64)), requires_grad=True)
    tht = torch.tensor(np.asarray(th, dtype=np.float64), requires_grad=True)
    n, d = X.shape
    m = len(Zt)
    eye = torch.eye(m, dtype=torch.float64)
    Kuu, sn, mu = _torch_kernel(kernel, d, tht, Zt, Zt, mean)
    Kuf, _, _ = _torch_kernel(kernel, d, tht, Zt, X, mean)
    kxx = _torch_kernel(kernel, d, tht, X[:1], X[:1], mean)[0][0, 0]            # (every named family is stationary)
    Lu = torch.linalg.cholesky(Kuu + jitter * eye)
    V = torch.linalg.solve_triangular(Lu, Kuf, upper=False)
    sn2 = sn * sn
    LB = torch.linalg.cholesky(sn2 * eye + V @ V.T)
    r = y - mu
    c = torch.linalg.solve_triangular(LB, (V @ r)[:, None], upper=False)[:, 0]
    F = (-0.5 * (n * math.log(2.0 * math.pi) + (n - m) * torch.log(sn2) + 2.0 * torch.log(torch.diag(LB)).sum() + (r @ r - c @ c) / sn2) -
         (n * kxx - (V * V).sum()) / (2.0 * sn2))
    F.backward()
    return float(F.detach()), tht.grad.numpy().copy(), Zt.grad.numpy().copy()


_cache = {}


def case_reference(name, n, d, m, mean, jrel=sg.JREL):
    """The references of one pinned case, computed once per process: {"X", "y", "Z", "theta", "jitter", "kernel", "F",
    "gradZ" (numpy analytic), "gradZ_torch", "route_difference" (max|gradZ - gradZ_torch| / max|gradZ|)}."""
    key = (name, n, d, m, mean, jrel)
    if key not in _cache:
        from bayesianinference_amd import synthetic as syn
        X, y = syn.make_dataset(n, d)
        th, Z = sg.theta_of(name, d, mean), sg.inducing_of(X, m)
        jit = jrel * sg.SF ** 2
        gz = analytic(name, th, X, y, Z, jit, mean)
        Ft, _, gt = autograd(name, th, X, y, Z, jit, mean)
        _cache[key] = {"X": X, "y": y, "Z": Z, "theta": th, "jitter": jit, "kernel": name,
                       "F": ref.bound_formulas(name, th, X, y, Z, jit, mean)["F"], "F_torch": Ft, "gradZ": gz, "gradZ_torch": gt,
                       "route_difference": float(np.abs(gz - gt).max() / np.abs(gz).max())}
    return _cache[key]
