"""An analytic gradient of the log marginal likelihood in theta for EVERY kernel form of the oracle's grammar: the likelihood of
oracle/gp_oracle.py (BGP:181-199) restated in torch float64 on tests/sparse_zgrad_reference._torch_kernel -- which parses the whole
grammar, [c +] k1 [(+|*) k2], both means -- and differentiated by reverse mode on the CPU.

    log p(y | theta) = -1/2 (N log 2 pi + log det K + r^T K^-1 r),      K = k(X, X) + sn^2 I,   r = y - mu

oracle.gp_oracle.log_likelihood_grad is analytic for SE and Matern-5/2 only and takes 4th-order central differences for everything
else (good to ~1e-6, and 4 p likelihoods per gradient); this one shares no derivative formula with it and is exact to rounding,
eps x cond(K) x N, for every form.  tests/test_dim_dispatch.py pins the two against each other where both are analytic."""
import math

import numpy as np

import sparse_zgrad_reference as zg


def loglik_and_grad(kernel, theta, X, y, mean="zero"):
    """(log likelihood, d/dtheta [p]) in theta's own layout"""
    import torch
    Xt = torch.tensor(np.atleast_2d(np.asarray(X, dtype=np.float64)))
    yt = torch.tensor(np.asarray(y, dtype=np.float64).ravel())
    tht = torch.tensor(np.asarray(theta, dtype=np.float64), requires_grad=True)
    n, d = Xt.shape
    K, sn, mu = zg._torch_kernel(kernel, d, tht, Xt, Xt, mean)
    L = torch.linalg.cholesky(K + sn * sn * torch.eye(n, dtype=torch.float64))
    z = torch.linalg.solve_triangular(L, (yt - mu)[:, None], upper=False)[:, 0]
    ll = -0.5 * (n * math.log(2.0 * math.pi) + 2.0 * torch.log(torch.diag(L)).sum() + z @ z)
    ll.backward()
    return float(ll.detach()), tht.grad.numpy().copy()


def log_likelihood_grad(kernel, theta, X, y, mean="zero"):
    return loglik_and_grad(kernel, theta, X, y, mean)[1]
