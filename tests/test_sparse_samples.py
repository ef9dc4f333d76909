"""CPU side of the sparse prediction over posterior samples (gphip_sparse_predict_samples): the symbol, its signature and binding
without a device, and the numpy side of the cases tests/test_gpu_sparse_samples.py runs on the device -- for every row that is
meant to succeed cond(K_uu) <= 1e10 and the two reference routes of the prediction agree to 1e-10 of max |y| (means) and of
max k(x, x) (variances), the thresholds of the existing sparse tests.  Measured: cond <= 5.3e8 on every row, the routes differ by
at most 3.4e-13 / 3.5e-15; the failure case's rows 0, 2, 4 at jitter 0 have cond = 57 and variances >= 0.013; k(x*, x*) of the
non-stationary case varies 0.84 - 1.92 across points and rows."""
import numpy as np
import pytest

import sparse_reference as ref
import sparse_samples_cases as sc
from bayesianinference_amd import _lib, build


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_the_symbol_is_declared_exported_signed_and_bound(lib):
    name = "gphip_sparse_predict_samples"
    assert name in _lib.declared_symbols(), f"{name} is not declared in include/gphip.h"
    assert hasattr(lib, name), f"{name} is not exported"
    assert name in _lib._SIGNATURES, f"{name} has no ctypes signature"
    assert callable(getattr(_lib.SparseHandle, "predict_samples", None))


def test_a_null_handle_is_an_argument_error_without_a_device(lib):
    th, xs, out, info = np.ones((1, 4)), np.zeros((1, 2)), np.zeros(1), np.zeros(1, dtype=np.int32)
    rc = lib.gphip_sparse_predict_samples(None, _lib._d(th), 1, 4, -1.0, xs.ctypes.data, 1, 0, _lib._d(out), _lib._d(out), None,
                                          info.ctypes.data_as(_lib._ip))
    assert rc == 1


@pytest.mark.parametrize("label", sc.LABELS)
def test_rows_are_well_conditioned_and_the_prediction_routes_agree(label):
    kernel, X, y, Z, mean, rows, jit, good = sc.case(label)
    Xs = sc.test_points(X.shape[1])
    want = sc.reference(label, False)
    for s in good:
        th = rows[s]
        cond = np.linalg.cond(ref.kuu_factor(kernel, th, Z, jit, mean)[1])
        dm, dv = ref.predict_definition(kernel, th, X, y, Z, jit, Xs, mean)
        em = np.abs(want["mean"][s] - dm).max() / want["ymax"]
        ev = np.abs(want["var"][s] - dv).max() / want["kmax"][s]
        kss = ref.kdiag(kernel, th, Xs, mean)
        print(f"{label} row {s}: cond(K_uu) {cond:.2e}, routes differ by {em:.1e} (mean) {ev:.1e} (var), "
              f"k(x*, x*) {kss.min():.3f} - {kss.max():.3f}, min var {want['var'][s].min():.3e}")
        assert cond <= 1e10 and em <= 1e-10 and ev <= 1e-10
        assert np.all(want["var"][s] > 0.0)
    assert all(np.all(np.isnan(want["mean"][s])) for s in range(len(rows)) if s not in good)


def test_the_non_stationary_case_has_a_diagonal_that_depends_on_point_and_row():
    kernel, X, _, _, mean, rows, _, _ = sc.case("nonstat")
    Xs = sc.test_points(X.shape[1])
    kss = np.array([ref.kdiag(kernel, th, Xs, mean) for th in rows])
    assert kss.std(axis=1).min() > 0.01 and kss.std(axis=0).min() > 0.01      # across the points of a row, across the rows at a point
