"""The seams of the one group evaluator behind every sparse bound (csrc/gphip_sparse.inc): the one-theta
entry points are that evaluator with one slot in resident mode, gphip_sparse_bound_batch loops it in batch mode.  What differs
between the modes must not depend on the number of rows in a group: a batch of one row is still a batch (no fit stays resident),
a one-theta call whose K_uu does not factor stops before the chunk loop and leaves the object usable, and the HIP-event phase
times are reset per call by their named ranges.  Bars: 1e-12 relative between the batched and the one-theta evaluation of the
same theta (the file-wide bar of tests/test_gpu_sparse_batch.py); the phase times are compared with zero only."""
import numpy as np
import pytest

import sparse_batch_cases as cases
from bayesianinference_amd import _lib, synthetic as syn

pytestmark = pytest.mark.gpu

JIT = cases.JITTER
FORWARD, GRAD, JOINT = _lib.SPARSE_PHASES, _lib.SPARSE_GRAD_PHASES, _lib.SPARSE_JOINT_PHASES


def _rel(a, b):
    return abs(a - b) / abs(b)


def _small():
    X, y = syn.make_dataset(300, 2)
    rows = np.array([[0.9, 1.1, 1.0, 0.12], [1.0, 1.0, 1.1, 0.2], [1.2, 0.8, 0.9, 0.15], [0.8, 1.3, 1.2, 0.1]])
    return X, y, cases.inducing(X, 40), rows


def _predict_status(h, Xs):
    with pytest.raises(_lib.GphipError) as e:
        h.predict(Xs)
    return e.value.status


def test_a_batch_of_one_row_is_still_a_batch():
    X, y, Z, rows = _small()
    h = _lib.SparseHandle(X, y, Z, "se_ard", "zero")
    th = rows[0]
    one, info1 = h.bound(th, JIT)
    assert info1 == 0 and h.fit(th, JIT) == 0
    h.predict(X[:5])
    F, info = h.bound_batch(th[None], JIT)
    print(f"one row: batch {F[0]:.12f} one-theta {one:.12f} rel {_rel(F[0], one):.2e}")
    assert info[0] == 0 and _rel(F[0], one) <= 1e-12
    assert h.get_option("last_sparse_slots") == 1
    assert _predict_status(h, X[:5]) == 4                        # the batch dropped the fit, although its group had one row
    # three rows in groups of two: the last group has one row
    free, info = h.bound_batch(rows[:3], JIT)
    assert np.all(info == 0) and h.get_option("last_sparse_slots") == 3
    h.set_option("sparse_batch_slots", 2)
    Fa, ia = h.bound_batch(rows[:3], JIT)
    assert h.get_option("last_sparse_slots") == 1
    Fb, ib = h.bound_batch(rows[:3], JIT)
    print(f"group of one: {Fa[2]:.12f} unrestricted {free[2]:.12f} rel {_rel(Fa[2], free[2]):.2e}")
    assert np.all(ia == 0) and _rel(Fa[2], free[2]) <= 1e-12
    assert np.array_equal(Fa, Fb) and np.array_equal(ia, ib)
    assert _predict_status(h, X[:5]) == 4
    h.close()


def test_one_theta_failure_then_reuse():
    X, y, Z, rows = cases.failure_case()
    h = _lib.SparseHandle(X, y, Z, "se_ard", "zero")
    h.set_option("profile", 1)
    F, parts, info = h.bound_parts(rows[3], 0.0)
    assert info == _lib.INFO_NOT_SPD and np.isnan(F) and np.all(np.isnan(parts))
    ms = {k: h.get_option(k) for k in FORWARD}
    print("phases after the failed call", ms)
    assert ms["ms_cross"] == 0 and ms["ms_accumulate"] == 0 and ms["ms_b_factor"] == 0       # it stopped before the chunk loop
    assert ms["ms_kuu_factor"] > 0
    assert _predict_status(h, X[:5]) == 4
    assert h.fit(rows[0], 0.0) == 0
    mean, var = h.predict(X[:5])
    fresh = _lib.SparseHandle(X, y, Z, "se_ard", "zero")
    assert fresh.fit(rows[0], 0.0) == 0
    mean0, var0 = fresh.predict(X[:5])
    fresh.close()
    assert np.array_equal(mean, mean0) and np.array_equal(var, var0)
    F, grad, info = h.bound_grad(rows[3], 0.0)
    assert info == _lib.INFO_NOT_SPD and np.isnan(F) and grad.shape == (4,) and np.all(np.isnan(grad))
    h.close()


def test_phase_times_reset_and_accumulate_per_call():
    X, y, Z, rows = _small()
    h = _lib.SparseHandle(X, y, Z, "se_ard", "zero")
    h.set_option("profile", 1)
    th = rows[0]

    def read(names):
        return [h.get_option(k) for k in names]

    assert h.bound(th, JIT)[1] == 0
    assert all(v > 0 for v in read(FORWARD)) and all(v == 0 for v in read(GRAD)) and all(v == 0 for v in read(JOINT))
    assert h.bound_grad(th, JIT)[2] == 0
    assert all(v > 0 for v in read(FORWARD)) and all(v > 0 for v in read(GRAD)) and all(v == 0 for v in read(JOINT))
    F, info = h.bound_batch(rows, JIT)
    assert np.all(info == 0)
    assert all(v > 0 for v in read(FORWARD)) and all(v == 0 for v in read(GRAD)) and all(v == 0 for v in read(JOINT))
    assert h.fit(th, JIT) == 0
    Xs = syn.make_test_points(10, 2)
    h.predict_cov(Xs)
    print("joint phases", dict(zip(JOINT, read(JOINT))))
    assert all(v > 0 for v in read(JOINT[:3])) and h.get_option(JOINT[3]) == 0     # (the covariance itself factors nothing)
    assert h.predict_logpdf(Xs, np.zeros(10))[1] == 0
    assert all(v > 0 for v in read(JOINT))
    h.close()
