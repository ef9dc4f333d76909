"""The Cholesky factor under test: a long-double reference, the five checks and their bars.  numpy only, no GPU.

Everything that decides a verdict is computed in np.longdouble (x86: the 80-bit format, eps = 1.08e-19), so the rounding of the
CHECK sits four decades under the float64 unit roundoff it judges.  The one exception is the normaliser |L| |L|^T of omega_factor, a
sum of non-negative products that float64 BLAS delivers to 1e-13 relative: it moves omega by that fraction of itself.

The checks (componentwise backward errors: independent of cond(K)) and their bars, u = 2^-53 for fp64 handles, 2^-24 for fp32:

  omega_factor   max_{i>=j} |K - L L^T|_ij / (|L| |L|^T)_ij           <= (n + 1) u + 2 delta_rsq
      Higham, Accuracy and Stability of Numerical Algorithms (2nd ed.), Thm 10.3: the computed factor of ANY ordering of the
      Cholesky sums satisfies |K - L L^T| <= gamma_{n+1} |L| |L|^T.  The theorem assumes a correctly rounded square root; the
      pivots here come from fast_rsqrt (hardware seed + one Newton step, relative error delta_rsq = 4e-15 by its own comment;
      fp32: the library rsqrt, 2 u), and a pivot off by delta moves the diagonal residual by 2 delta L_jj^2 <= 2 delta (|L||L|^T)_jj.
  omega_solve    max_i |L z - r|_i / (|L| |z|)_i                       <= (n + 1) u
      Higham Thm 8.5 (substitution in any order: gamma_n) with one more rounding for the widening / the residual's own.
  omega_inverse  min(max |W Lbb - I| / (|W| |Lbb|), max |Lbb W - I| / (|Lbb| |W|))   <= 129 u     (per 128-block)
      Higham 14.2: every standard triangular inversion method satisfies ONE of the two residual bounds with gamma_{n+1}, n = 128.
  logdet tie     |logdet - 2 sum log L_ii|                             <= (n + 2) u 2 sum |log L_ii|
  quad tie       |quad - z^T z|                                         <= (n + 2) u z^T z
      a sum of n terms in any order (gamma_{n-1}), each term one rounded log / product, the doubling, the export.

The bars are derived, not fitted, and live HERE only; tests/test_factor_reference.py pins this module before it judges a kernel."""
import numpy as np

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
HAVE_LD = EPS_LD < 1e-18                       # 80-bit (or wider) long double; a float64 alias cannot judge a float64 kernel
assert EPS_LD <= float(np.finfo(np.float64).eps)
SKIP_REASON = "np.longdouble is float64 on this platform: the reference has no precision to spare over the kernels it judges"

U = {64: 2.0 ** -53, 32: 2.0 ** -24}
DELTA_RSQ = {64: 4e-15, 32: 2.0 * 2.0 ** -24}
TB = 128                                       # the diagonal blocks whose explicit inverses the panel solves multiply by


# ---- the bars ----
def bar_factor(n, dtype=64):
    return (n + 1) * U[dtype] + 2.0 * DELTA_RSQ[dtype]


def bar_solve(n, dtype=64):
    return (n + 1) * U[dtype]


def bar_inverse(dtype=64):
    return (TB + 1) * U[dtype]


def bar_logdet(L, dtype=64):
    n = L.shape[0]
    return (n + 2) * U[dtype] * 2.0 * float(np.sum(np.abs(np.log(np.diag(L).astype(LD)))))


def bar_quad(z, dtype=64):
    return (len(z) + 2) * U[dtype] * float(quad_from(z))


# ---- the reference factorisation ----
def chol_ld(K):
    """Unblocked right-looking Cholesky in long double: the lower factor of K (only its lower triangle is read)."""
    A = np.tril(np.asarray(K)).astype(LD)
    n = A.shape[0]
    for j in range(n):
        if not A[j, j] > 0:
            raise np.linalg.LinAlgError("not positive definite at pivot %d" % j)
        A[j, j] = np.sqrt(A[j, j])
        if j + 1 < n:
            A[j + 1:, j] /= A[j, j]
            c = A[j + 1:, j]
            A[j + 1:, j + 1:] -= np.tril(np.outer(c, c))
    return A


def _lower_product(A, B, dtype=LD, block=64):
    """the lower triangle (block-wise: a little more) of A B^T for lower-triangular A, B, skipping the zero half of the sums"""
    n = A.shape[0]
    A, B = np.asarray(A).astype(dtype), np.asarray(B).astype(dtype)
    P = np.zeros((n, n), dtype=dtype)
    for j in range(0, n, block):
        je = min(j + block, n)
        P[j:, j:je] = A[j:, :je] @ B[j:je, :je].T
    return P


def _ratio(num, den):
    """max of num / den over the entries given, 0 / 0 = 0 (an entry nothing contributes to), x / 0 = inf"""
    num, den = np.asarray(num, dtype=LD), np.asarray(den, dtype=LD)
    out = np.zeros(num.shape, dtype=LD)
    nz = den > 0
    out[nz] = num[nz] / den[nz]
    out[~nz & (num > 0)] = np.inf
    out[~np.isfinite(num)] = np.inf
    return out


# ---- the five checks ----
def omega_factor_map(K, L):
    """|K - L L^T|_ij / (|L| |L|^T)_ij on the lower triangle (zeros above): which entries miss a bar is read off this map"""
    L = np.tril(np.asarray(L))
    res = np.abs(np.tril(np.asarray(K)).astype(LD) - np.tril(_lower_product(L, L)))
    den = np.tril(_lower_product(np.abs(L), np.abs(L), dtype=np.float64))
    return _ratio(res, den)


def omega_factor(K, L):
    return float(np.max(omega_factor_map(K, L)))


def omega_solve(L, z, r):
    L, z, r = np.tril(np.asarray(L)).astype(LD), np.asarray(z).astype(LD), np.asarray(r).astype(LD)
    return float(np.max(_ratio(np.abs(L @ z - r), np.abs(L) @ np.abs(z))))


def omega_inverse(Lbb, W):
    """one diagonal block and its explicit inverse: the smaller of the left and the right componentwise residual"""
    Lb, Wb = np.asarray(Lbb).astype(LD), np.asarray(W).astype(LD)
    eye = np.eye(Lb.shape[0], dtype=LD)
    left = np.max(_ratio(np.abs(Wb @ Lb - eye), np.abs(Wb) @ np.abs(Lb)))
    right = np.max(_ratio(np.abs(Lb @ Wb - eye), np.abs(Lb) @ np.abs(Wb)))
    return float(min(left, right))


def diag_blocks(L):
    """the 128 x 128 diagonal blocks of the factor of the PADDED matrix (identity beyond n), as the library inverts them"""
    n = L.shape[0]
    out = []
    for b0 in range(0, n, TB):
        blk = np.eye(TB)
        m = min(TB, n - b0)
        blk[:m, :m] = np.tril(L[b0:b0 + m, b0:b0 + m])
        out.append(blk)
    return out


def omega_inverse_all(L, W):
    """the largest omega_inverse over the diagonal blocks; W[b] = the inverse of block b, row-major [i, j]"""
    blocks = diag_blocks(L)
    assert len(blocks) == len(W)
    return max(omega_inverse(Lb, Wb) for Lb, Wb in zip(blocks, W))


def logdet_from(L):
    return 2 * np.sum(np.log(np.diag(np.asarray(L)).astype(LD)))


def quad_from(z):
    z = np.asarray(z).astype(LD)
    return z @ z


def run_checks(K, L, z, r, W, logdet, quad, dtype=64):
    """{check: (value, bar)} for the five checks of one factor"""
    n = L.shape[0]
    return {
        "factor": (omega_factor(K, L), bar_factor(n, dtype)),
        "solve": (omega_solve(L, z, r), bar_solve(n, dtype)),
        "inverse": (omega_inverse_all(L, W), bar_inverse(dtype)),
        "logdet": (float(abs(LD(logdet) - logdet_from(L))), bar_logdet(L, dtype)),
        "quad": (float(abs(LD(quad) - quad_from(z))), bar_quad(z, dtype)),
    }


def failed(checks):
    return sorted(k for k, (v, bar) in checks.items() if not v <= bar)


def report(tag, checks):
    return tag + ": " + ", ".join("%s %.2e / %.2e (%.1fx)" % (k, v, bar, bar / v if v > 0 else float("inf")) for k, (v, bar) in checks.items())


# ---- this project's algorithm on the host: 128-blocks, the explicit inverse of each diagonal block, X = A W^T ----
def emulate(K, dtype=64, pivot_error=None):
    """Blocked right-looking Cholesky as the multi-kernel route does it, in the handle's arithmetic with LAPACK / BLAS for the
    pieces: potrf of the diagonal block, its explicit inverse W by triangular solve of the identity, the panel X = A W^T, the
    trailing update.  Returns (L, [W_b padded to 128 x 128]).  pivot_error = (j, eps) scales pivot j by (1 + eps), j = None
    every pivot, and carries on with it as a device with a wrong reciprocal square root would (W, the panel below and the
    trailing update all use the wrong pivot): the tests' model of a defect."""
    from scipy.linalg import solve_triangular
    T = np.float64 if dtype == 64 else np.float32
    A = np.tril(np.asarray(K)).astype(T)
    A = A + np.tril(A, -1).T
    n = A.shape[0]
    Ws = []
    for b0 in range(0, n, TB):
        b1 = min(b0 + TB, n)
        Lbb = np.linalg.cholesky(A[b0:b1, b0:b1]).astype(T)
        if pivot_error is not None:
            j, eps = pivot_error
            for jj in (range(b1 - b0) if j is None else [j - b0] if b0 <= j < b1 else []):
                Lbb[jj, jj] = T(Lbb[jj, jj] * (1.0 + eps))
        W = solve_triangular(Lbb, np.eye(b1 - b0, dtype=T), lower=True).astype(T)
        A[b0:b1, b0:b1] = Lbb
        Wp = np.eye(TB, dtype=T)
        Wp[:b1 - b0, :b1 - b0] = W
        Ws.append(Wp)
        if b1 < n:
            X = (A[b1:, b0:b1] @ W.T).astype(T)
            A[b1:, b0:b1] = X
            A[b1:, b1:] -= X @ X.T
    return np.tril(A), Ws


def solve_like_device(L, Ws, r, dtype=64):
    """z = L^-1 r by blocks with the explicit inverses, as the bordered row is solved: z_b = (r_b - sum L_bk z_k) W_b^T"""
    T = np.float64 if dtype == 64 else np.float32
    n = L.shape[0]
    z = np.zeros(n, dtype=T)
    r = np.asarray(r).astype(T)
    for i, b0 in enumerate(range(0, n, TB)):
        b1 = min(b0 + TB, n)
        rhs = r[b0:b1] - L[b0:b1, :b0].astype(T) @ z[:b0]
        z[b0:b1] = Ws[i][:b1 - b0, :b1 - b0].astype(T) @ rhs
    return z
