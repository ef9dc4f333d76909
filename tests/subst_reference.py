"""The substitutions behind solve and predict under test: judged against the device's OWN factor in long double.
numpy only, no GPU.  Extends tests/factor_reference.py (LD, U, TB, bar_solve, _ratio, HAVE_LD, emulate come from there).

With L-hat and z-hat readable (Handle.factor) no check needs the oracle's K: cond(K) drops out of the backward check and enters
the forward checks only through a bound that is COMPUTED from the factor (M = |L^-1| |L|), never guessed.  Everything that decides
is np.longdouble; only normalisers and error bars that are sums of non-negative products (|L| |L^T| |X|, M |y|, ..) use float64
BLAS, which delivers them to 1e-13 of themselves.

Notation: u = 2^-53 (fp32 handles 2^-24), g = bar_solve(n) = (n + 1) u, L = tril(L-hat) widened, Li = L^-1 in long double,
M = |Li| |L|, rho = g ||M||_inf (asserted <= 0.1 for every matrix the module is given).

  omega_solve2   max |B - L (L^T X)| / (|L| (|L^T| |X|))                                   <= 2 g + g^2
      Higham, Accuracy and Stability (2nd ed.), Thm 8.5 on each triangle: substitution in ANY order gives (L + D1) y^ = b and
      (L^T + D2) x^ = y^ with |Di| <= gamma_n |L|.  So b = (L + D1)(L^T + D2) x^ and
      |b - L L^T x^| <= |D1| |L^T| |x^| + |L| |D2| |x^| + |D1| |D2| |x^| <= (2 gamma + gamma^2) |L| |L^T| |x^|;
      gamma_n <= g for every n u the tables reach (the one spare u is the widening / the residual's own rounding).
      B is the right-hand side ROUNDED TO THE HANDLE'S TYPE (fp32 handles narrow it before they substitute).
  phi_solve      max |X - x*| / e_x with y* = Li B, x* = Li^T y*                            <= 1
      e_y = g M |y*| / (1 - rho):   y^ - y* = -Li D1 y^, |y^| <= |y*| + |y^ - y*|; the division by (1 - rho) is what makes
      Higham's bound, which has the COMPUTED vector on its right, usable with the exact one.
      e_x = (g |Li^T| (|L^T| |x*|) + |Li^T| e_y) / (1 - rho):   x^ - x* = (x^ - Li^T y^) + Li^T (y^ - y*).
  predict        v* = Li k*_t, e_v = g M |v*| / (1 - rho); predict_finish_kernel forms mean = mu + v . z and
                 var = k(x*, x*) + nugget - ||v||^2 with fp64 sums of n terms in some order:
      mean bar   e_v . |z| + (n + 2) u (|v*| + e_v) . |z| + 2^-53 |m*|,                       m* = mu + v* . z
      var bar    2 e_v . |v*| + e_v . e_v + (n + 2) u (|v*| + e_v) . (|v*| + e_v) + 2 2^-53 kappa_t,   var* = kappa_t - v* . v*
      value = the largest error / bar over the test points, mean and var separately     <= 1

The bars are derived, not fitted, and live HERE only; tests/test_subst_reference.py pins this module before it judges a kernel."""
import numpy as np

from factor_reference import HAVE_LD, LD, TB, U, _ratio, bar_solve, emulate      # noqa: F401  (re-exported to the tests)

RHO_MAX = 0.1
U64 = 2.0 ** -53


def bar_solve2(n, dtype=64):
    g = bar_solve(n, dtype)
    return 2.0 * g + g * g


def _T(dtype):
    return np.float64 if dtype == 64 else np.float32


# ---- long-double products with a lower-triangular matrix, skipping the zero half ----
def _dot(A, Vf):
    """A Vf in the operands' type; for long double numpy has no BLAS, and its dot runs ~9x faster over contiguous rows of A and
    contiguous columns of Vf than its matmul over row-major operands"""
    return np.dot(np.ascontiguousarray(A), Vf)


def _lv(L, V, block=64):
    """L V for lower-triangular L, in the type of the operands"""
    out = np.zeros(V.shape, dtype=L.dtype)
    Vf = np.asfortranarray(V)
    for j in range(0, L.shape[0], block):
        je = min(j + block, L.shape[0])
        out[j:je] = _dot(L[j:je, :je], Vf[:je])
    return out


def _ltv(L, V, block=64):
    """L^T V for lower-triangular L"""
    out = np.zeros(V.shape, dtype=L.dtype)
    Vf, LT = np.asfortranarray(V), np.ascontiguousarray(L.T)
    for j in range(0, L.shape[0], block):
        je = min(j + block, L.shape[0])
        out[j:je] = _dot(LT[j:je, j:], Vf[j:])
    return out


def _cols(A):
    A = np.asarray(A)
    return A.reshape(A.shape[0], -1)


def widen(L):
    return np.tril(np.asarray(L)).astype(LD)


def inverse_ld(L):
    """L^-1 in long double: row-wise substitution over the identity, all columns of a row at once"""
    L = widen(L)
    n = L.shape[0]
    Li = np.zeros((n, n), dtype=LD)
    for i in range(n):
        row = -(L[i, :i] @ Li[:i, :i]) if i else np.zeros(0, dtype=LD)
        Li[i, :i] = row / L[i, i]
        Li[i, i] = LD(1) / L[i, i]
    return Li


class Factor:
    """one factor prepared for the checks: L and Li in long double, M = |Li| |L| (float64: a sum of non-negative products), rho"""

    def __init__(self, L, dtype=64, Li=None):
        self.L = widen(L)
        self.n = self.L.shape[0]
        self.dtype = dtype
        self.Li = inverse_ld(self.L) if Li is None else np.asarray(Li, dtype=LD)
        self.absL = np.abs(self.L).astype(np.float64)
        self.absLi = np.abs(self.Li).astype(np.float64)
        self.M = self.absLi @ self.absL
        self.g = bar_solve(self.n, dtype)
        self.rho = self.g * float(np.max(np.sum(self.M, axis=1)))
        assert self.rho <= RHO_MAX, "rho = g ||M||_inf = %.3e: the forward bounds need a better-conditioned matrix" % self.rho


def _factor(L, Li, dtype):
    return L if isinstance(L, Factor) else Factor(L, dtype, Li)


# ---- the checks ----
def omega_solve2_cols(L, X, B):
    """per right-hand side: max_i |B - L (L^T X)|_i / (|L| (|L^T| |X|))_i"""
    Lw = L.L if isinstance(L, Factor) else widen(L)
    aL = L.absL if isinstance(L, Factor) else np.abs(Lw).astype(np.float64)
    X, B = _cols(X), _cols(B)
    res = np.abs(B.astype(LD) - _lv(Lw, _ltv(Lw, X.astype(LD))))
    den = aL @ (aL.T @ np.abs(X.astype(np.float64)))
    return np.max(_ratio(res, den), axis=0).astype(np.float64)


def omega_solve2(L, X, B):
    return float(np.max(omega_solve2_cols(L, X, B)))


def exact_solve(F, B):
    """(y*, x*) = (Li B, Li^T y*) in long double"""
    y = _lv(F.Li, _cols(B).astype(LD))
    return y, _ltv(F.Li, y)


def phi_solve_cols(L, Li, X, B, dtype=64):
    F = _factor(L, Li, dtype)
    X = _cols(X)
    y, x = exact_solve(F, B)
    e_y = F.g * (F.M @ np.abs(y).astype(np.float64)) / (1.0 - F.rho)
    e_x = (F.g * (F.absLi.T @ (F.absL.T @ np.abs(x).astype(np.float64))) + F.absLi.T @ e_y) / (1.0 - F.rho)
    return np.max(_ratio(np.abs(X.astype(LD) - x), e_x), axis=0).astype(np.float64)


def phi_solve(L, Li, X, B, dtype=64):
    return float(np.max(phi_solve_cols(L, Li, X, B, dtype)))


def predict_bars(L, Li, z, kstar, kappa, mu, dtype=64, wide=LD):
    """(m*, mean bar, var*, var bar) per test point.  wide = np.float64 is the cheap form for very many points: the caller
    multiplies the bars by 4 for the rounding of a float64 check of a float64 result."""
    F = _factor(L, Li, dtype)
    n, u = F.n, U[dtype]
    z = np.asarray(z).astype(wide)
    kstar = _cols(kstar)
    v = _lv(F.Li.astype(wide), kstar.astype(wide))
    av = np.abs(v).astype(np.float64)
    az = np.abs(z).astype(np.float64)
    e_v = F.g * (F.M @ av) / (1.0 - F.rho)
    m_star = wide(mu) + z @ v
    var_star = np.asarray(kappa).astype(wide) - np.sum(v * v, axis=0)
    w = av + e_v
    mean_bar = az @ e_v + (n + 2) * u * (az @ w) + U64 * np.abs(m_star).astype(np.float64)
    var_bar = 2.0 * np.sum(e_v * av, axis=0) + np.sum(e_v * e_v, axis=0) + (n + 2) * u * np.sum(w * w, axis=0) + 2.0 * U64 * np.asarray(kappa, dtype=np.float64)
    return m_star, mean_bar, var_star, var_bar


def predict_checks(L, Li, z, kstar, kappa, mu, mean, var, dtype=64, wide=LD, scale=1.0):
    """{"mean": (value, 1), "var": (value, 1), "worst": (t_mean, t_var)}: the largest error / bar over the test points"""
    m_star, mean_bar, var_star, var_bar = predict_bars(L, Li, z, kstar, kappa, mu, dtype, wide)
    rm = _ratio(np.abs(np.asarray(mean).astype(wide) - m_star), scale * mean_bar)
    rv = _ratio(np.abs(np.asarray(var).astype(wide) - var_star), scale * var_bar)
    return {"mean": (float(np.max(rm)), 1.0), "var": (float(np.max(rv)), 1.0), "worst": (int(np.argmax(rm)), int(np.argmax(rv))),
            "ratios": (np.asarray(rm, dtype=np.float64), np.asarray(rv, dtype=np.float64))}


def slack(L, Li, z, kstar, kappa, mu, dtype=64):
    """how loose the forward bars are, relative to what they bound: (max var bar / kappa_t, max mean bar / max(|m*|, ||z||_inf)).
    The case tables cap both at 1e-9 (fp32: u32 / u64 times that), so a bar can never go slack through an ill-conditioned row."""
    m_star, mean_bar, _, var_bar = predict_bars(L, Li, z, kstar, kappa, mu, dtype)
    zmax = float(np.max(np.abs(z)))
    return (float(np.max(var_bar / np.asarray(kappa, dtype=np.float64))),
            float(np.max(mean_bar / np.maximum(np.abs(m_star).astype(np.float64), zmax))))


def slack_cap(dtype=64):
    return 1e-9 * (U[dtype] / U[64])


def solve_checks(L, Li, X, B, dtype=64):
    """{check: (value, bar)} of a solve: B already rounded to the handle's type"""
    F = _factor(L, Li, dtype)
    return {"omega2": (omega_solve2(F, X, B), bar_solve2(F.n, dtype)), "phi": (phi_solve(F, None, X, B, dtype), 1.0)}


def failed(checks):
    return sorted(k for k, v in checks.items() if k not in ("worst", "ratios") and not v[0] <= v[1])


def report(tag, checks):
    return tag + ": " + ", ".join("%s %.2e / %.2e (%.1fx)" % (k, v[0], v[1], v[1] / v[0] if v[0] > 0 else float("inf"))
                                  for k, v in checks.items() if k not in ("worst", "ratios"))


def round_rhs(B, dtype=64):
    """the right-hand side as the handle substitutes it"""
    B = np.asarray(B, dtype=np.float64)
    return B if dtype == 64 else B.astype(np.float32).astype(np.float64)


# ---- this project's algorithm on the host: both triangles through the explicit block inverses ----
def cut_w64(Ws):
    """the 64-block inverses as w128_to_w64_kernel cuts them out of the 128-block ones: the two diagonal 64 x 64 blocks of W_b
    ARE the inverses of the diagonal 64 x 64 blocks of L_bb; the coupling L_bb[64:, :64] stays in the factor"""
    out = []
    for W in Ws:
        out += [W[:64, :64], W[64:, 64:]]
    return out


def substitute_like_device(L, Ws, B, dtype=64, tb=TB, skip=None, w_of=None):
    """x = L^-T (L^-1 b) by blocks of tb rows with explicit inverses, in the handle's arithmetic:
         y_b = W_b (b_b - sum_{k<b} L_bk y_k);   x_b = W_b^T (y_b - sum_{k>b} L_kb^T x_k).
    Ws: one inverse per block (tb = 128: emulate()'s; tb = 64: cut_w64 of them).  Returns (y, x).
    The tests' models of a defect: skip = (b, c) leaves the contribution of tile L(b, c), b > c, out of the BACKWARD pass;
    w_of = {b: b2} uses block b2's inverse for block b (both passes)."""
    T = _T(dtype)
    L = np.asarray(L).astype(T)
    B = _cols(B).astype(T)
    n = L.shape[0]
    blocks = [(b0, min(b0 + tb, n)) for b0 in range(0, n, tb)]
    W = lambda i, m: Ws[(w_of or {}).get(i, i)][:m, :m].astype(T)      # noqa: E731
    y = np.zeros(B.shape, dtype=T)
    for i, (b0, b1) in enumerate(blocks):
        y[b0:b1] = W(i, b1 - b0) @ (B[b0:b1] - L[b0:b1, :b0] @ y[:b0])
    x = np.zeros(B.shape, dtype=T)
    for i in reversed(range(len(blocks))):
        b0, b1 = blocks[i]
        acc = y[b0:b1].copy()
        for k in range(i + 1, len(blocks)):
            k0, k1 = blocks[k]
            if skip is not None and (k0 // TB, b0 // TB) == tuple(skip):
                continue
            acc -= L[k0:k1, b0:b1].T @ x[k0:k1]
        x[b0:b1] = W(i, b1 - b0).T @ acc
    return y.astype(np.float64), x.astype(np.float64)


def predict_like_device(L, Ws, z, kstar, kappa, mu, dtype=64, tb=TB, drop_strip=None, nugget_twice=0.0, no_mu=False):
    """(mean, var) as predict does: v = L^-1 k* by blocks in the handle's type, then fp64 sums (predict_partial_kernel widens).
    Defect models: drop_strip = (t, s) leaves rows [64 s, 64 s + 64) of v out of ||v||^2 for test point t; no_mu omits mu."""
    kstar = _cols(kstar)
    T = _T(dtype)
    Lt = np.asarray(L).astype(T)
    n = Lt.shape[0]
    v = np.zeros(kstar.shape, dtype=T)
    ks = kstar.astype(T)
    for i, b0 in enumerate(range(0, n, tb)):
        b1 = min(b0 + tb, n)
        v[b0:b1] = Ws[i][:b1 - b0, :b1 - b0].astype(T) @ (ks[b0:b1] - Lt[b0:b1, :b0] @ v[:b0])
    v = v.astype(np.float64)
    mean = (0.0 if no_mu else mu) + np.asarray(z, dtype=np.float64) @ v
    sq = v * v
    if drop_strip is not None:
        t, s = drop_strip
        sq[64 * s:64 * s + 64, t] = 0.0
    var = np.asarray(kappa, dtype=np.float64) + nugget_twice - np.sum(sq, axis=0)
    return mean, var
