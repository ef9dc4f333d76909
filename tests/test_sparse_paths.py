"""Pathwise posterior draws of the sparse object, the parts that need no GPU: the two new symbols, argument validation in front
of the library, and the numpy reference of tests/sparse_paths_reference.py pinned against the sparse object's own predictive
law (tests/sparse_joint_reference.py).

Measured here (float64, m = 70, N = 300, d = 3, SE-ARD, the default jitter 1e-10 k(x, x)), in units of max Sigma_ii:
    l = (0.7, 0.9, 1.1)   with zeta 3e-12   without zeta 2e-6
    l = (1.5, 2.0, 2.5)   with zeta 6e-10   without zeta 2e-4
(the test prints them; the closed form carries L_u^-1 Cov(g) L_u^-T as a computed matrix, whose rounding grows with cond(K_uu),
so that dropping zeta changes a number and not a formula).  Bar: 1e-9 of max Sigma_ii."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import paths_reference as pr
import sparse_joint_reference as sj
import sparse_paths_reference as spr
from bayesianinference_amd import _lib, gaussian_process as gp

NEW = ("gphip_sparse_paths_create", "gphip_sparse_paths_get")
LAW_BAR = 1e-9


def test_symbols_are_declared_exported_signed_and_bound():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for name in NEW:
        assert name in declared and name in _lib._SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name][1] and getattr(lib, name).restype is C.c_int
    assert len(_lib._SIGNATURES["gphip_sparse_paths_create"][1]) == 6 and len(_lib._SIGNATURES["gphip_sparse_paths_get"][1]) == 3
    with open(_lib.HEADER) as f:
        header = f.read()
    assert re.search(r"int gphip_sparse_paths_create\(gphip_sparse_handle h, int S, int F, uint64_t seed, gphip_paths_handle\* out, int\* info\);", header)
    assert re.search(r"int gphip_sparse_paths_get\(gphip_paths_handle q, double\* xi[^,]*, double\* zeta[^)]*\);", header)
    for fn in ("sample_paths",):
        assert callable(getattr(_lib.SparseHandle, fn))
    assert callable(gp.samplePathsFromSparseGaussianProcess) and callable(gp.thompsonSampleFromSparseGaussianProcess)
    # the host code lives in its own file, behind gphip_paths.inc
    csrc = os.path.join(os.path.dirname(_lib.__file__), "csrc")
    with open(os.path.join(csrc, "gphip.hip")) as f:
        tail = f.read()
    assert tail.index('#include "gphip_paths.inc"') < tail.index('#include "gphip_sparse_paths.inc"')
    # without a device: NULL arguments are refused before anything else
    q, info = C.c_void_p(), C.c_int(0)
    assert lib.gphip_sparse_paths_create(None, 4, 8, 0, C.byref(q), C.byref(info)) == 1 and not q.value
    assert lib.gphip_sparse_paths_get(None, None, None) == 1


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def test_validation_raises_before_the_library_is_touched():
    h = _lib.SparseHandle.__new__(_lib.SparseHandle)
    h._lib, h._h, h.N, h.d, h.m = _NoLibrary(), None, 10, 3, 4
    for s, f in ((0, 8), (-1, 8), (2049, 8), (4, 0)):
        with pytest.raises(ValueError):
            h.sample_paths(s, f)
    p = _lib.Paths.__new__(_lib.Paths)
    p._parent, p._lib, p._q, p.S, p.d, p._sparse = h, _NoLibrary(), None, 4, 3, True
    for shape in ((4, 5), (3, 5, 3), (4, 5, 2), (4, 0, 3)):
        with pytest.raises(ValueError):
            p.eval_own(np.zeros(shape), grad=True)
    with pytest.raises(_lib.GphipError):
        p.eval(np.zeros((5, 2)))                                  # the sparse parent's own check of the dimension
    # the Python layer returns None without a sparse object, draws or a theta to fit
    assert gp.samplePathsFromSparseGaussianProcess({"not": "an object"}, 4) is None
    assert gp.thompsonSampleFromSparseGaussianProcess(None, 4, [[0.0, 1.0]]) is None


@pytest.mark.parametrize("ell", [spr.ELL_NARROW, spr.ELL_WIDE], ids=["narrow", "wide"])
def test_law_with_an_exact_prior_is_the_sparse_predictive_law(ell):
    """m = 70, N = 300, d = 3: the closed-form mean and covariance of the draws equal the sparse mean and the latent Sigma of
    gphip_sparse_predict_cov's reference; with the sqrt(j) zeta term dropped the covariance does not."""
    m, d = 70, 3
    X, y, Z, Xs = spr.case_data(m, d)
    th = spr.theta_of("se_ard", d, "const", ell)
    jit = spr.JREL * spr.SF ** 2
    mu, S = sj.joint_formulas("se_ard", th, X, y, Z, jit, Xs, "const", latent=True)
    smax = float(np.max(np.diag(S)))
    lm, lc = spr.law("se_ard", th, X, y, Z, jit, Xs, "const")
    _, lc0 = spr.law("se_ard", th, X, y, Z, jit, Xs, "const", zeta=False)
    e, e0, em = np.abs(lc - S).max() / smax, np.abs(lc0 - S).max() / smax, np.abs(lm - mu).max() / np.abs(mu).max()
    print(f"l = {ell}: covariance off by {e:.3e} of max Sigma_ii = {smax:.3e}; without zeta {e0:.3e}; mean {em:.3e}")
    assert e <= LAW_BAR and em <= 1e-12
    assert e0 > 10 * LAW_BAR                                      # the test sees the zeta term


def test_reference_draws_follow_their_closed_form_moments():
    """The draw-by-draw reference against the closed-form moments for a fixed table: the sample mean and covariance of
    S = 4096 reference draws (numpy's Philox streams) within Monte-Carlo error (5 sigma, fixed seed)."""
    m, d, S, F = 70, 3, 4096, 32
    X, y, Z, Xs = spr.case_data(m, d)
    Xs = Xs[:6]
    th = spr.theta_of("se_ard", d, "const", spr.ELL_NARROW)
    jit = 1e-6 * spr.SF ** 2
    om, ph, amp = _lib.rff_table("se_ard", d, th, F, 7)
    table = {"omega": om, "phase": ph, "amp": amp}
    w = pr.philox_normal(7, np.arange(S)[:, None], np.arange(len(amp))[None, :])
    xi, zeta = spr.philox_streams(7, S, m)
    out = spr.paths("se_ard", th, X, y, Z, jit, Xs, table, w, xi, zeta, "const", grad=False)["out"]
    mo = spr.moments("se_ard", th, X, y, Z, jit, Xs, table, "const")
    cmax = np.max(np.diag(mo["cov"]))
    em, ec = np.abs(out.mean(axis=0) - mo["mean"]).max(), np.abs(np.cov(out.T) - mo["cov"]).max()
    print(f"sample mean off by {em:.3e} (bar {5 * np.sqrt(cmax / S):.3e}), covariance by {ec:.3e} (bar {5 * np.sqrt(2.0 / S) * cmax:.3e})")
    assert em <= 5.0 * np.sqrt(cmax / S) and ec <= 5.0 * np.sqrt(2.0 / S) * cmax


def test_reference_gradient_is_the_derivative_of_the_reference():
    m, d, S, F = 70, 3, 3, 16
    X, y, Z, Xs = spr.case_data(m, d)
    Xs = Xs[:5]
    th = spr.theta_of("matern52+rq_ard+const", d, "zero")
    om, ph, amp = _lib.rff_table("matern52+rq_ard+const", d, th, F, 2)
    table = {"omega": om, "phase": ph, "amp": amp}
    w = pr.philox_normal(2, np.arange(S)[:, None], np.arange(len(amp))[None, :])
    xi, zeta = spr.philox_streams(2, S, m)
    f = lambda P: spr.paths("matern52+rq_ard+const", th, X, y, Z, 1e-8, P, table, w, xi, zeta, "zero")      # noqa: E731
    g = f(Xs)["dout"]
    for c in range(d):
        e = np.zeros(d)
        e[c] = 1e-5
        fd = (f(Xs + e)["out"] - f(Xs - e)["out"]) / 2e-5
        assert np.abs(fd - g[:, :, c]).max() <= 1e-7 * np.abs(g).max(), c


def test_xi_and_zeta_differ_from_every_stream_the_table_uses():
    """tags 10 and 11 against w (the seed itself), the table's tags 0, 1, 4, 5, 8 and eps's tag 9: all keys distinct, and the
    normals of the same counters differ by O(1)"""
    seed, S, m = 5, 6, 40
    xi, zeta = spr.philox_streams(seed, S, m)
    keys = [seed & pr.MASK64] + [pr.rff_key(seed, t) for t in (0, 1, 4, 5, 8, pr.TAG_EPS)]
    mine = [pr.rff_key(seed, spr.TAG_XI), pr.rff_key(seed, spr.TAG_ZETA)]
    assert len(set(keys + mine)) == len(keys) + 2
    assert mine[0] == (seed ^ (11 * pr.RFF_KEY)) & pr.MASK64 and mine[1] == (seed ^ (12 * pr.RFF_KEY)) & pr.MASK64
    s, i = np.arange(S)[:, None], np.arange(m)[None, :]
    assert np.abs(xi - zeta).min() > 1e-6
    for key in keys:
        other = pr.philox_normal(key, s, i)
        assert np.abs(xi - other).min() > 1e-6 and np.abs(zeta - other).min() > 1e-6
    assert abs(xi.std() - 1.0) <= 0.2 and abs(zeta.std() - 1.0) <= 0.2


def test_extended_precision_evaluation_agrees_where_the_problem_is_well_conditioned():
    """paths_mp (the yardstick of the device test's ill-conditioned case) against the float64 reference at cond(K_uu) ~ 1e3: they
    agree to 1e-12, so a larger gap at l = (3, 4, 5) is the float64 reference's own rounding"""
    m, d, S, F = 20, 3, 2, 8
    X, y, Z, Xs = spr.case_data(m, d, n=40, m_test=5)
    th = spr.theta_of("se_ard", d, "const", spr.ELL_NARROW)
    jit = spr.JREL * spr.SF ** 2
    om, ph, amp = _lib.rff_table("se_ard", d, th, F, 3)
    table = {"omega": om, "phase": ph, "amp": amp}
    w = pr.philox_normal(3, np.arange(S)[:, None], np.arange(len(amp))[None, :])
    xi, zeta = spr.philox_streams(3, S, m)
    r = spr.paths("se_ard", th, X, y, Z, jit, Xs, table, w, xi, zeta, "const", grad=False)
    e = spr.paths_mp("se_ard", th, X, y, Z, jit, Xs, table, w, xi, zeta, "const")
    assert np.abs(r["out"] - e["out"]).max() <= 1e-12 * np.abs(e["out"]).max()
    assert np.abs(r["v"] - e["v"]).max() <= 1e-11 * np.abs(e["v"]).max()
