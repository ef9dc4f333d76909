"""CPU side of the batched sparse bound (gphip_sparse_bound_batch, gphip_sparse_nested_sampling): the symbols and their status
contract without a device, the one-call batching of make_sparse_log_likelihood against a stub handle, and the numpy side of the
cases tests/test_gpu_sparse_batch.py runs on the device -- conditioning and agreement of the two reference routes for every row
that is meant to succeed (the guard of tests/test_gpu_sparse.py), the small pivot of the row that is meant to fail."""
import ctypes
import math

import numpy as np
import pytest

import sparse_batch_cases as cases
import sparse_reference as ref
from bayesianinference_amd import _lib, build, gaussian_process as gp, nested_sampling as ns


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_new_symbols_are_declared_exported_and_signed(lib):
    names = _lib.declared_symbols()
    for name in ("gphip_sparse_bound_batch", "gphip_sparse_nested_sampling"):
        assert name in names, f"{name} is not declared in include/gphip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib._SIGNATURES, f"{name} has no ctypes signature"


def test_null_handles_are_argument_errors_without_a_device(lib):
    th, out, info = np.ones(4), np.zeros(1), np.zeros(1, dtype=np.int32)
    assert lib.gphip_sparse_bound_batch(None, _lib._d(th), 1, 4, -1.0, _lib._d(out), None, info.ctypes.data_as(_lib._ip)) == 1
    o = _lib.NsOptions()
    assert lib.gphip_ns_default_options(ctypes.byref(o)) == 0
    box, pts, ll = np.array([[0.0, 1.0]]), np.zeros((200, 1)), np.zeros(200)
    n = ctypes.c_int64(0)
    assert lib.gphip_sparse_nested_sampling(None, -1.0, _lib._d(box), None, None, None, ctypes.byref(o), None, 200, _lib._d(pts),
                                            _lib._d(ll), None, None, ctypes.byref(n), None, None) == 1


class StubHandle:
    """records the calls make_sparse_log_likelihood makes"""

    def __init__(self, values, info):
        self.values, self.info, self.calls = np.asarray(values, dtype=np.float64), np.asarray(info, dtype=np.int32), []

    def bound_batch(self, Theta, jitter=-1.0, parts=False):
        self.calls.append(("bound_batch", np.array(Theta), jitter))
        return self.values.copy(), self.info.copy()

    def bound(self, theta, jitter=-1.0):
        self.calls.append(("bound", np.array(theta), jitter))
        return -12.5, 0


def test_a_batch_is_one_bound_batch_call_with_sentinel_and_clip():
    """Rows: info = 1; NaN; the largest finite double (= -MACHINE_LOG_ZERO: no finite double lies above the clip's upper end,
    so the clip is checked at its end); +inf, the one value above it, which is non-finite and therefore the sentinel, as for the
    one-theta closure; an ordinary value."""
    top = -gp.MACHINE_LOG_ZERO
    stub = StubHandle([-3.0, np.nan, top, np.inf, -7.25], [1, 0, 0, 0, 0])
    f = gp.make_sparse_log_likelihood(stub, 1e-6)
    Theta = np.arange(15, dtype=np.float64).reshape(5, 3)
    out = f(Theta)
    assert [c[0] for c in stub.calls] == ["bound_batch"]            # ONE call, and no per-row `bound`
    assert np.array_equal(stub.calls[0][1], Theta) and stub.calls[0][2] == 1e-6
    assert out.shape == (5,) and out.dtype == np.float64
    assert out[0] == gp.MACHINE_LOG_ZERO and out[1] == gp.MACHINE_LOG_ZERO and out[3] == gp.MACHINE_LOG_ZERO
    assert out[2] == top and out[4] == -7.25
    assert np.all(out >= gp.MACHINE_LOG_ZERO) and np.all(out <= top)


def test_a_single_theta_is_still_one_bound_call():
    stub = StubHandle([0.0], [0])
    f = gp.make_sparse_log_likelihood(stub, -1.0)
    assert f(np.array([0.5, 1.0, 0.1])) == -12.5
    assert [c[0] for c in stub.calls] == ["bound"]


@pytest.mark.parametrize("name,n,d,m,mean,B", cases.PARITY + [cases.DETERMINISM])
def test_parity_rows_are_well_conditioned_and_the_reference_routes_agree(name, n, d, m, mean, B):
    X, y, Z, kernel, rows = cases.parity_case(name, n, d, m, mean, B)
    for s, th in enumerate(rows):
        _, Kuu = ref.kuu_factor(kernel, th, Z, cases.JITTER, mean)
        cond = np.linalg.cond(Kuu)
        a = ref.bound_formulas(kernel, th, X, y, Z, cases.JITTER, mean)["F"]
        b = ref.bound_definition(kernel, th, X, y, Z, cases.JITTER, mean)
        print(f"{name} N={n} m={m} row {s}: cond(K_uu) {cond:.2e}, routes differ by {abs(a - b) / abs(b):.1e}")
        assert cond <= 1e10 and abs(a - b) / abs(b) <= 1e-10


def test_failure_case_rows_are_what_they_claim():
    X, y, Z, rows = cases.failure_case()
    for s in (0, 2, 4):                        # well conditioned WITHOUT jitter
        _, Kuu = ref.kuu_factor("se_ard", rows[s], Z, 0.0, "zero")
        cond = np.linalg.cond(Kuu)
        a = ref.bound_formulas("se_ard", rows[s], X, y, Z, 0.0, "zero")["F"]
        b = ref.bound_definition("se_ard", rows[s], X, y, Z, 0.0, "zero")
        print(f"row {s}: cond(K_uu) {cond:.2e}, routes differ by {abs(a - b) / abs(b):.1e}")
        assert cond <= 1e10 and abs(a - b) / abs(b) <= 1e-10
    assert np.isnan(rows[1]).sum() == 1
    Kuu = ref.cross("se_ard", rows[3], Z, Z, "zero")
    kxx = rows[3][2] ** 2
    col = cases.first_small_pivot(Kuu, cases.PIVOT_TOL_REL * kxx, 20)
    print("row 3: first pivot <= 64 eps k(x, x) at column", col)
    assert col is not None and col < 20


def test_the_split_rule_helper_counts_workgroups():
    # m = 300 -> 3 tile rows -> 9 output tiles; a chunk of 1536 rows has 12 row tiles; 256 CUs want 512 workgroups
    assert cases.expected_nsplit(384, 1536, 1, 256) == 12
    assert cases.expected_nsplit(384, 1536, 5, 256) == 12           # 45 workgroups: 12 strips of one row tile
    assert cases.expected_nsplit(384, 1536, 5, 20) == 1             # 45 >= 40: no strips
    assert cases.expected_nsplit(1024, 32768, 32, 256) == 1         # 32 rows at m = 1024: 44 tiles x 32 >= 512
    assert cases.expected_nsplit(384, 1536, 5, 256, option=4) == 4


def test_the_sampler_case_has_a_converged_grid():
    """The sampler's GPU test measures the log evidence against the 24^3 midpoint grid with an allowance of 4 se + 0.25.  That
    is a reference only if the grid resolves the posterior, so the same integral on the 36^3 grid (which shares no point with
    the 24^3 one) has to agree to 0.025, a tenth of the allowance's constant.  The grid values come from a numpy route that
    shares the m x m work along sn; it is held to the reference's bound at points spread over the box first."""
    X, y, Z, box = cases.sampler_case()
    assert X.shape == (400, 1) and Z.shape == (32, 1)
    vals = cases.sampler_grid_bound(X, y, Z, cases.SAMPLER_GRID, cases.SAMPLER_JITTER)
    axes, grid = cases.sampler_grid(cases.SAMPLER_GRID)
    assert np.all(grid[:, 0] > box[0, 0]) and np.all(grid[:, 2] < box[2, 1])
    top = np.unravel_index(np.argmax(vals), vals.shape)
    for a, s, k in [(0, 0, 0), (23, 23, 23), (9, 4, 17), (23, 0, 0), (0, 23, 11), top]:
        th = np.array([axes[0][a], axes[1][s], axes[2][k]])
        want = ref.bound_formulas("se", th, X, y, Z, cases.SAMPLER_JITTER, "zero")["F"]
        assert abs(vals[a, s, k] - want) <= 1e-8 * abs(want), (th, vals[a, s, k], want)
    z24 = ns.log_sum_exp(vals.ravel()) - math.log(vals.size)
    fine = cases.sampler_grid_bound(X, y, Z, 36, cases.SAMPLER_JITTER)
    z36 = ns.log_sum_exp(fine.ravel()) - math.log(fine.size)
    print(f"log evidence on the 24^3 grid {z24:.5f}, on the 36^3 grid {z36:.5f}; the largest bound on the grid at "
          f"l {axes[0][top[0]]:.3f} sf {axes[1][top[1]]:.3f} sn {axes[2][top[2]]:.3f}")
    assert abs(z24 - z36) <= 0.025
    assert 2 <= top[2] <= 21                              # the mode in sn lies inside the box, not on its edge
