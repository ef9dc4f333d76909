"""tests/factor_reference.py pinned before it judges a kernel; no GPU.

1. chol_ld against a 40-digit mpmath Cholesky.
2. Every distinct matrix of the case table (tests/factor_cases.py) through LAPACK in the handle's arithmetic and through the host
   emulation of the blocked algorithm with explicit inverses: all five checks pass; the headroom is printed.
3. Every check bites: a factor whose pivot, whose sub-diagonal entry in the last tile row, or whose z / W entry / scalar is off by
   1e-11 (fp32: 1e-3) fails ITS check and no other.
4. The table's own health: cond(K) <= 1e7 and a median off-diagonal correlation in [0.1, 0.9]."""
import numpy as np
import pytest
from scipy.linalg import solve_triangular

import factor_cases as fc
import factor_reference as fr
from oracle import gp_oracle as orc

pytestmark = pytest.mark.skipif(not fr.HAVE_LD, reason=fr.SKIP_REASON)

INPUTS = fc.distinct_inputs()
IDS = [c["id"] for c in INPUTS]
_cache = {}


def host_K(case):
    """the oracle's K of a row, as the handle's arithmetic holds it (fp32: rounded to float32, widened)"""
    key = case["id"]
    if key not in _cache:
        X, y, th = fc.inputs(case)
        K = orc.covariance_matrix(case["kernel"], th, X, case["mean"])
        if case["dtype"] == 32:
            K = K.astype(np.float32).astype(np.float64)
        _cache[key] = (K, fc.residual(case, y, th))
    return _cache[key]


def _scalars(L, z, T):
    """log det and the quadratic form as a device would form them: in the arithmetic type, from the factor and the row it has"""
    return float(2 * np.sum(np.log(np.diag(L).astype(T)), dtype=T)), float(np.dot(z.astype(T), z.astype(T)))


def lapack_route(K, r, dtype):
    T = np.float64 if dtype == 64 else np.float32
    L = np.linalg.cholesky(K.astype(T)).astype(T)
    z = solve_triangular(L, r.astype(T), lower=True).astype(T)
    W = [solve_triangular(b.astype(T), np.eye(fr.TB, dtype=T), lower=True) for b in fr.diag_blocks(L)]
    return (L.astype(np.float64), z.astype(np.float64), [w.astype(np.float64) for w in W]) + _scalars(L, z, T)


def emulation_route(K, r, dtype, pivot_error=None):
    T = np.float64 if dtype == 64 else np.float32
    L, W = fr.emulate(K, dtype, pivot_error)
    z = fr.solve_like_device(L, W, r, dtype)
    return (L.astype(np.float64), z.astype(np.float64), [w.astype(np.float64) for w in W]) + _scalars(L, z, T)


def test_long_double_is_wider_than_the_kernels():
    assert fr.EPS_LD < 1.1e-19 and np.finfo(np.longdouble).nmant >= 63


def test_chol_ld_matches_mpmath():
    mp = pytest.importorskip("mpmath")
    n = 24
    X, _ = fc.dataset(n, 3)
    K = orc.covariance_matrix("se_ard", fc.theta("se_ard", 3, 0.15), X)
    with mp.workdps(40):
        ref = mp.cholesky(mp.matrix(K.tolist()))
        L = fr.chol_ld(K)
        wide = lambda v: mp.mpf(float(np.float64(v))) + mp.mpf(float(v - np.longdouble(np.float64(v))))      # noqa: E731
        err = max(abs(wide(L[i, j]) - ref[i, j]) for i in range(n) for j in range(i + 1)) / max(abs(ref[i, i]) for i in range(n))
    # forward error of a Cholesky factor: n eps cond(K) relative to the norm of the factor (Higham 10.8, to first order)
    bar = n * fr.EPS_LD * float(np.linalg.cond(K))
    print("chol_ld against mpmath (40 digits), n = 24: largest error / max L_ii %.2e, bar n eps cond(K) = %.2e" % (float(err), bar))
    assert float(err) <= bar <= 1e-14                           # (and the bar itself sits two decades under float64)


def test_chol_ld_own_backward_error():
    K, _ = host_K(fc.SIZE_EDGES[8])                               # n = 257
    L = fr.chol_ld(K)
    om = float(np.max(fr._ratio(np.abs(np.tril(K).astype(fr.LD) - np.tril(fr._lower_product(L, L))),
                                np.tril(fr._lower_product(np.abs(L), np.abs(L))))))
    print("chol_ld n = 257: omega_factor %.2e (long double eps %.2e)" % (om, fr.EPS_LD))
    assert om <= 258 * fr.EPS_LD


@pytest.mark.parametrize("case", INPUTS, ids=IDS)
def test_lapack_and_emulation_pass_every_check(case):
    K, r = host_K(case)
    for name, route in (("LAPACK", lapack_route), ("emulation", emulation_route)):
        L, z, W, logdet, quad = route(K, r, case["dtype"])
        checks = fr.run_checks(K, L, z, r, W, logdet, quad, case["dtype"])
        print(fr.report("%s %s" % (case["id"], name), checks))
        assert fr.failed(checks) == [], (name, checks)


# (not the se, d = 1, sn = 0.05 row: its late pivots have L_jj^2 = 2e-3 K_jj, and a pivot's relative error reaches the residual
#  scaled by exactly that share -- 1e-11 there is a backward error of 4e-14, inside the bar by right)
BITE = [c for c in INPUTS if c["id"] in ("n385-f64", "n385-f32", "n641-mk-nolookahead")]


@pytest.mark.parametrize("case", BITE, ids=[c["id"] for c in BITE])
def test_every_check_bites(case):
    K, r = host_K(case)
    dt, n = case["dtype"], case["n"]
    eps = 1e-11 if dt == 64 else 1e-3
    T = np.float64 if dt == 64 else np.float32
    run = lambda L, z, W, ld, q: fr.failed(fr.run_checks(K, L, z, r, W, ld, q, dt))      # noqa: E731
    L, z, W, logdet, quad = emulation_route(K, r, dt)
    assert run(L, z, W, logdet, quad) == []
    # one pivot wrong, everything after it computed from it: the factor no longer reproduces K, all else is consistent
    for j in (0, 200 % n, n - 1):
        assert run(*emulation_route(K, r, dt, (j, eps))) == ["factor"], j
    assert run(*emulation_route(K, r, dt, (None, eps))) == ["factor"]
    # one sub-diagonal entry of the last tile row (it feeds nothing but the last diagonal block); z solved from that factor
    i = n - 1
    t0 = (i // fr.TB) * fr.TB                                     # its columns left of the last diagonal block
    weight = np.abs(L[i, :t0] * np.diag(L)[:t0]) / (np.abs(L[:t0, :t0]) @ np.abs(L[i, :t0]))      # share of entry (i, j) in its own residual's normaliser
    j = int(np.argmax(weight))
    assert eps * weight[j] > 2 * fr.bar_factor(n, dt)             # (else the defect is below what ANY backward-error test can see)
    L2 = L.copy()
    L2[i, j] = T(L2[i, j] * (1 + eps))
    z2 = fr.solve_like_device(L2.astype(T), [w.astype(T) for w in W], r, dt).astype(np.float64)
    assert run(L2, z2, W, logdet, _scalars(L2, z2, T)[1]) == ["factor"]
    # one entry of z, the scalar formed from the row as it stands
    z3 = z.copy()
    k = int(np.argmax(np.abs(L[np.arange(n), np.arange(n)] * z) / (np.abs(L) @ np.abs(z))))
    z3[k] = T(z3[k] * (1 + eps))
    assert run(L, z3, W, logdet, _scalars(L, z3, T)[1]) == ["solve"]
    # one entry of one explicit inverse
    W4 = [w.copy() for w in W]
    W4[-1][0, 0] = T(W4[-1][0, 0] * (1 + eps))
    assert run(L, z, W4, logdet, quad) == ["inverse"]
    W5 = [w.copy() for w in W]
    W5[0][77, 77] = T(W5[0][77, 77] * (1 + eps))
    assert run(L, z, W5, logdet, quad) == ["inverse"]
    # the two scalars
    assert run(L, z, W, logdet * (1 + eps), quad) == ["logdet"]
    assert run(L, z, W, logdet, quad * (1 + eps)) == ["quad"]


def test_a_dropped_newton_step_is_seen():
    """fast_rsqrt without its Newton step leaves the seed's 5e-8: four decades over the bar at every n of the table"""
    case = fc.SIZE_EDGES[9]
    K, r = host_K(case)
    L, z, W, logdet, quad = emulation_route(K, r, 64, (None, 5e-8))
    checks = fr.run_checks(K, L, z, r, W, logdet, quad, 64)
    print(fr.report("every pivot off by 5e-8", checks))
    assert fr.failed(checks) == ["factor"] and checks["factor"][0] > 1e3 * checks["factor"][1]


@pytest.mark.parametrize("case", INPUTS, ids=IDS)
def test_the_table_is_neither_diagonal_nor_singular(case):
    K, _ = host_K(case)
    n = case["n"]
    cond = float(np.linalg.cond(K))
    Kf = K - case["sn"] ** 2 * np.eye(n)
    sd = np.sqrt(np.diag(Kf))
    corr = (Kf / np.outer(sd, sd))[~np.eye(n, dtype=bool)]
    med = float(np.median(corr)) if n > 1 else float("nan")
    print("%s: cond(K) %.2e, median off-diagonal correlation %.3f" % (case["id"], cond, med))
    assert cond <= 1e7
    assert n == 1 or 0.1 <= med <= 0.9


def test_launch_table_is_complete():
    ids = {c["id"] for c in fc.SCHEDULES}
    for n in (641, 700):
        for sid, _, _ in fc._SCHEDULES:
            assert "n%d-%s" % (n, sid) in ids
    for a, b in fc.SAME_LAUNCHES_AS.items():
        la = {sid: l for sid, _, l in fc._SCHEDULES}
        assert la[a] == la[b] or a == "mk-nofuse-throughput-gemm", (a, b)
