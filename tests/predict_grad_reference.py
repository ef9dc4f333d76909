"""float64 CPU references for the gradients of the predictive mean and variance in the TEST inputs (include/gphip.h
gphip_predict_grad, gphip_sparse_predict_grad), built on oracle/gp_oracle.py, tests/sparse_reference.py and
tests/sparse_zgrad_reference.dk_da.  Two routes that share no derivative formula:

  exact(...) / sparse(...)                    numpy: the header's formulas,
      exact:   dmu = sum_i alpha_i dk(x*, x_i)/dx*,      dvar = -2 sum_i w_i dk(x*, x_i)/dx*,      w = K^-1 k*
      sparse:  dmu = sum_k (a_mu)_k dk(x*, z_k)/dx*,     dvar = -2 sum_k W_k dk(x*, z_k)/dx*,
               a_mu = L_u^-T L_B^-T c,   W = L_u^-T (V1 - sn^2 L_B^-T V2)
  exact_autograd(...) / sparse_autograd(...)  torch float64 on the CPU: reverse mode through mu and sigma^2 restated in torch;

and central differences of the numpy PREDICTION (differences(...)) as a sanity check.  The pinned cases cover every named
family, a product and a sum of two terms, the additive constant, both means, d = 1 .. 20 (d = 20 with two terms takes the
device's global-memory window form) and one test point that coincides with a training point."""
import numpy as np
import scipy.linalg as sla

import sparse_reference as ref
import sparse_zgrad_reference as zg
from oracle import gp_oracle as orc

SF, SN = 1.1, 0.15                    # sn / sf = 0.14 >= 0.05
N, M = 300, 130                       # Npad = 384 with a ragged last tile; two 128-tiles of test points, the last one ragged
COINCIDE = (7, 11)                    # test point 7 = training point 11
# (kernel, d, mean)
CASES = [("se", 1, "zero"), ("se_ard", 3, "const"), ("matern52_ard", 8, "zero"), ("matern32", 2, "const"), ("rq_ard", 3, "zero"),
         ("se_ard*matern32+const", 3, "const"), ("se+rq", 20, "zero")]
SPARSE_M = 40                         # inducing points of the sparse cases (m_pad = 128)
SPARSE_TWO_TILES = ("se_ard", 3, "const", 200)
JREL = 1e-6


def case_id(case):
    return "%s-d%d-%s" % case[:3]


def theta_of(name, d, mean):
    ell = [0.3] if d == 1 else list(np.linspace(0.8, 1.3, d))
    if name == "se":
        th = [0.3 if d == 1 else 0.9, SF, SN]
    elif name in ("se_ard", "matern52_ard"):
        th = ell + [SF, SN]
    elif name == "matern32":
        th = [0.7, SF, SN]
    elif name == "rq_ard":
        th = ell + [1.7, SF, SN]
    elif name == "se_ard*matern32+const":
        th = ell + [SF] + [0.9, 0.9] + [0.3, SN]
    elif name == "se+rq":
        th = [2.5, SF] + [3.5, 1.7, 0.8] + [SN]
    else:
        raise ValueError(name)
    return np.array(th + ([0.2] if mean == "const" else []))


def case_data(name, d, mean, n=N, m_test=M):
    """(X, y, Xs, theta): seeded inputs; test point COINCIDE[0] is training point COINCIDE[1]"""
    from bayesianinference_amd import synthetic as syn
    X, y = syn.make_dataset(n, d)
    Xs = syn.make_test_points(m_test, d).copy()
    if m_test > COINCIDE[0]:
        Xs[COINCIDE[0]] = X[COINCIDE[1]]
    return X, y, Xs, theta_of(name, d, mean)


def inducing_of(X, m):
    return X[::len(X) // m][:m].copy()


# ---- route 1: numpy, the header's formulas ----
def exact(kernel, th, X, y, Xs, mean="zero"):
    """{"mean", "var" (noisy), "dmean" [M, d], "dvar" [M, d]}"""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    th = np.asarray(th, dtype=np.float64)
    K = orc.covariance_matrix(kernel, th, X, mean)
    k, kappa = orc.k_and_kappa(kernel, th, X, Xs, mean)                 # k: N x M
    cf = sla.cho_factor(K, lower=True)
    alpha = sla.cho_solve(cf, orc.residual(kernel, th, X, y, mean))
    w = sla.cho_solve(cf, k)                                            # N x M
    mu = ref.noise_and_mean(kernel, th, X.shape[1], mean)[1]
    dk = zg.dk_da(kernel, th, Xs, X, mean)                              # [M, N, d]
    return {"mean": mu + alpha @ k, "var": kappa - np.sum(k * w, axis=0),
            "dmean": np.einsum("i,tic->tc", alpha, dk), "dvar": -2.0 * np.einsum("it,tic->tc", w, dk)}


def sparse(kernel, th, X, y, Z, jitter, Xs, mean="zero"):
    """the same for the sparse object (var: of a noisy observation)"""
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    th = np.asarray(th, dtype=np.float64)
    sn2, _ = ref.noise_and_mean(kernel, th, Xs.shape[1], mean)
    f = ref.bound_formulas(kernel, th, X, y, Z, jitter, mean)
    Lu, LB, c = f["Lu"], f["LB"], f["c"]
    v1 = sla.solve_triangular(Lu, ref.cross(kernel, th, Z, Xs, mean), lower=True)
    v2 = sla.solve_triangular(LB, v1, lower=True)
    a_mu = sla.solve_triangular(Lu, sla.solve_triangular(LB, c, lower=True, trans="T"), lower=True, trans="T")
    W = sla.solve_triangular(Lu, v1 - sn2 * sla.solve_triangular(LB, v2, lower=True, trans="T"), lower=True, trans="T")   # m x M
    dk = zg.dk_da(kernel, th, Xs, Z, mean)                              # [M, m, d]
    mu, var = ref.predict_formulas(kernel, th, X, y, Z, jitter, Xs, mean)
    return {"mean": mu, "var": var, "dmean": np.einsum("k,tkc->tc", a_mu, dk), "dvar": -2.0 * np.einsum("kt,tkc->tc", W, dk)}


# ---- route 2: torch float64 autograd through the prediction itself ----
def _rows_grad(fn, Xs):
    """gradient of every row's own scalar: fn(Xs)[t] depends on Xs[t] only, so the gradient of the sum holds all of them"""
    import torch
    P = torch.tensor(np.atleast_2d(np.asarray(Xs, dtype=np.float64)), requires_grad=True)
    fn(P).sum().backward()
    return P.grad.numpy().copy()


def exact_autograd(kernel, th, X, y, Xs, mean="zero"):
    import torch
    Xt = torch.tensor(np.atleast_2d(np.asarray(X, dtype=np.float64)))
    yt = torch.tensor(np.asarray(y, dtype=np.float64).ravel())
    tht = torch.tensor(np.asarray(th, dtype=np.float64))
    d = Xt.shape[1]
    K, sn, mu = zg._torch_kernel(kernel, d, tht, Xt, Xt, mean)
    L = torch.linalg.cholesky(K + sn * sn * torch.eye(len(Xt), dtype=torch.float64))
    z = torch.linalg.solve_triangular(L, (yt - mu)[:, None], upper=False)[:, 0]

    def v_of(P):
        return torch.linalg.solve_triangular(L, zg._torch_kernel(kernel, d, tht, Xt, P, mean)[0], upper=False)     # N x M

    def var_of(P):
        kss = torch.stack([zg._torch_kernel(kernel, d, tht, P[t:t + 1], P[t:t + 1], mean)[0][0, 0] for t in range(len(P))])
        return kss + sn * sn - (v_of(P) ** 2).sum(0)
    return {"dmean": _rows_grad(lambda P: mu + v_of(P).T @ z, Xs), "dvar": _rows_grad(var_of, Xs)}


def sparse_autograd(kernel, th, X, y, Z, jitter, Xs, mean="zero"):
    import torch
    Xt = torch.tensor(np.atleast_2d(np.asarray(X, dtype=np.float64)))
    Zt = torch.tensor(np.atleast_2d(np.asarray(Z, dtype=np.float64)))
    yt = torch.tensor(np.asarray(y, dtype=np.float64).ravel())
    tht = torch.tensor(np.asarray(th, dtype=np.float64))
    d, m = Xt.shape[1], len(Zt)
    eye = torch.eye(m, dtype=torch.float64)
    Kuu, sn, mu = zg._torch_kernel(kernel, d, tht, Zt, Zt, mean)
    Lu = torch.linalg.cholesky(Kuu + jitter * eye)
    V = torch.linalg.solve_triangular(Lu, zg._torch_kernel(kernel, d, tht, Zt, Xt, mean)[0], upper=False)
    sn2 = sn * sn
    LB = torch.linalg.cholesky(sn2 * eye + V @ V.T)
    c = torch.linalg.solve_triangular(LB, (V @ (yt - mu))[:, None], upper=False)[:, 0]

    def v12(P):
        v1 = torch.linalg.solve_triangular(Lu, zg._torch_kernel(kernel, d, tht, Zt, P, mean)[0], upper=False)
        return v1, torch.linalg.solve_triangular(LB, v1, upper=False)

    def var_of(P):
        v1, v2 = v12(P)
        kss = torch.stack([zg._torch_kernel(kernel, d, tht, P[t:t + 1], P[t:t + 1], mean)[0][0, 0] for t in range(len(P))])
        return kss + sn2 - (v1 ** 2).sum(0) + sn2 * (v2 ** 2).sum(0)
    return {"dmean": _rows_grad(lambda P: mu + v12(P)[1].T @ c, Xs), "dvar": _rows_grad(var_of, Xs)}


# ---- sanity: central differences of the numpy prediction ----
def differences(predict, Xs, entries, rel=1e-4):
    """{(t, c): (dmean, dvar)} by 4th-order central differences of predict(P) -> (mean, var), step rel x max(|x_tc|, 0.1)"""
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    out = {}
    for (t, c) in entries:
        h = rel * max(abs(Xs[t, c]), 0.1)

        def f(s):
            P = Xs[t:t + 1].copy()
            P[0, c] += s
            mu, var = predict(P)
            return np.array([mu[0], var[0]])
        out[(t, c)] = (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)
    return out


def exact_predict(kernel, th, X, y, mean):
    def predict(P):
        mu, sd = orc.predict_internal(kernel, th, X, y, P, mean)
        return mu, sd * sd
    return predict


# ---- the pinned cases, computed once per process and left unchanged ----
_cache = {}


def _frozen(dct):
    for v in dct.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return dct


def case_reference(name, d, mean):
    """{"kernel", "mean_kind", "X", "y", "Xs", "theta", "mean", "var", "dmean", "dvar"} of one exact case"""
    key = ("exact", name, d, mean)
    if key not in _cache:
        X, y, Xs, th = case_data(name, d, mean)
        out = exact(name, th, X, y, Xs, mean)
        out.update({"kernel": name, "mean_kind": mean, "X": X, "y": y, "Xs": Xs, "theta": th})
        _cache[key] = _frozen(out)
    return _cache[key]


def sparse_case_reference(name, d, mean, m=SPARSE_M, jrel=JREL):
    """the same for the sparse object, plus "Z" and "jitter" (jrel x SF^2; jrel = None: the library's default, 1e-10 x k(x, x))"""
    key = ("sparse", name, d, mean, m, jrel)
    if key not in _cache:
        X, y, Xs, th = case_data(name, d, mean)
        Z = inducing_of(X, m)
        jit = (1e-10 * float(ref.kdiag(name, th, X[:1], mean)[0])) if jrel is None else jrel * SF ** 2
        out = sparse(name, th, X, y, Z, jit, Xs, mean)
        out.update({"kernel": name, "mean_kind": mean, "X": X, "y": y, "Xs": Xs, "theta": th, "Z": Z, "jitter": jit})
        _cache[key] = _frozen(out)
    return _cache[key]
