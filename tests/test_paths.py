"""Pathwise posterior function draws, the parts that need no GPU: the random-Fourier-feature table behind the C ABI
(gphip_rff_table, csrc/gphip_hostlogic.inc) against the kernels' own values, and the numpy reference (tests/paths_reference.py)
against itself.

Recorded, not asserted (test_rff_error_of_the_posterior_covariance_is_recorded prints them): the relative error of the RFF
covariance A A^T + sn^2 B B^T against the exact latent covariance, N = 60, sn = 0.1, M = 40, se_ard d = 2, in units of max
Sigma_ii -- an O(1 / sqrt(F)) approximation of the prior that the conditioning does not remove."""
import ctypes as C

import numpy as np
import pytest

import paths_reference as pr
from bayesianinference_amd import _lib

F_LAW = 65536
TWO_PI = 2.0 * np.pi


def _offsets(d, n=50, seed=5):
    return np.random.default_rng(seed).uniform(-3.0, 3.0, size=(n, d))


def _theta(name, d):
    """sf = 1, sn = 0.1, alpha = 1.7"""
    ard = name.endswith("_ard")
    ell = list(np.linspace(0.7, 1.6, d)) if ard else [1.2]
    return np.array(ell + ([1.7] if name.startswith("rq") else []) + [1.0, 0.1])


@pytest.mark.parametrize("name", ["se", "matern52", "matern32", "rq", "se_ard", "matern52_ard", "matern32_ard", "rq_ard"])
def test_spectral_law_of_every_family(name):
    d = 3
    th = _theta(name, d)
    om, ph, amp = _lib.rff_table(name, d, th, F_LAW, seed=11)
    assert om.shape == (F_LAW, d) and np.all(amp == np.sqrt(2.0 / F_LAW))
    delta = _offsets(d)
    g = pr.kernel_of_offsets(name, th, delta)                       # sf = 1: g(|delta / l|^2)
    est = np.cos(delta @ om.T).mean(axis=1)
    # a mean of F independent terms of variance <= 1: 5 sigma
    assert np.max(np.abs(est - g)) <= 5.0 / np.sqrt(F_LAW), (name, np.max(np.abs(est - g)))
    assert np.all(ph >= 0.0) and np.all(ph < TWO_PI)
    assert abs(ph.mean() - np.pi) <= 5.0 * (TWO_PI / np.sqrt(12.0)) / np.sqrt(F_LAW)


@pytest.mark.parametrize("name,d,th,scale", [
    ("se+rq", 3, [2.5, 1.1, 3.5, 1.7, 0.8, 0.15], 1.1 ** 2 + 0.8 ** 2),
    ("se_ard*matern32+const", 3, [0.8, 1.05, 1.3, 1.1, 0.9, 0.9, 0.3, 0.15], (1.1 * 0.9) ** 2),
    ("se+rq", 20, [2.5, 1.1, 3.5, 1.7, 0.8, 0.15], 1.1 ** 2 + 0.8 ** 2),
    ("matern52_ard", 20, list(np.linspace(2.0, 4.0, 20)) + [1.3, 0.15], 1.3 ** 2)])
def test_spectral_law_of_composed_kernels_weighted_by_amplitude(name, d, th, scale):
    """k(delta) = sum_j a_j^2 / 2 cos(Omega_j . delta) over the random features + the offset feature's a^2 (its phase is 0)"""
    th = np.array(th)
    om, ph, amp = _lib.rff_table(name, d, th, F_LAW, seed=3)
    offs = name.endswith("+const")
    nreg = len(amp) - (1 if offs else 0)
    assert len(amp) == (2 if "+rq" in name else 1) * F_LAW + (1 if offs else 0)
    delta = _offsets(d)
    est = (np.cos(delta @ om[:nreg].T) * (0.5 * amp[:nreg] ** 2)).sum(axis=1)
    if offs:
        assert np.all(om[-1] == 0.0) and ph[-1] == 0.0
        est = est + amp[-1] ** 2
    k = pr.kernel_of_offsets(name, th, delta)
    # every term's mean of F cosines has a standard deviation <= sf_t^2 / sqrt(F); scale = their sum (a product: sf_1^2 sf_2^2)
    assert np.max(np.abs(est - k)) <= 5.0 * scale / np.sqrt(F_LAW), (name, d, np.max(np.abs(est - k)))
    assert np.all(ph[:nreg] >= 0.0) and np.all(ph[:nreg] < TWO_PI)
    assert abs(ph[:nreg].mean() - np.pi) <= 5.0 * (TWO_PI / np.sqrt(12.0)) / np.sqrt(nreg)


def test_table_is_deterministic_in_its_arguments():
    th = _theta("rq_ard", 3)
    a = _lib.rff_table("rq_ard", 3, th, 300, seed=7)
    b = _lib.rff_table("rq_ard", 3, th, 300, seed=7)
    c = _lib.rff_table("rq_ard", 3, th, 300, seed=8)
    for u, v, w in zip(a, b, c):
        assert u.tobytes() == v.tobytes()
    assert a[0].tobytes() != c[0].tobytes() and a[1].tobytes() != c[1].tobytes()
    # small alpha takes the boosted gamma sampler
    om = _lib.rff_table("rq", 2, [1.0, 0.4, 1.0, 0.1], 2000, seed=1)[0]
    assert np.all(np.isfinite(om))


def test_table_streams_are_the_documented_philox_counters():
    """The table's documented keys against numpy's own Philox4x32-10 (paths_reference.philox_normal / philox_uniform): for SE the
    direction is the normal itself, so omega l = philox_normal(key of tag 0, j, c), and the second term of a sum draws under
    tag 4; the phase is 2 pi philox_uniform(key of tag 8, j, 0), exactly.  The normals agree up to the rounding of log, sqrt and
    cos (1e-13 absolute: see tests/test_gpu_paths.py).  The key that gphip_paths_create gives eps (tag 9) is no key of the table."""
    d, F, seed = 3, 500, 0xDEADBEEF12345
    ell = np.array([0.7, 1.1, 1.6])
    om, ph, amp = _lib.rff_table("se_ard+se_ard", d, np.concatenate([ell, [1.3], 2.0 * ell, [0.6], [0.1]]), F, seed=seed)
    j, c = np.arange(F)[:, None], np.arange(d)[None, :]
    assert np.abs(om[:F] * ell - pr.philox_normal(pr.rff_key(seed, pr.TAG_DIRECTION), j, c)).max() <= 1e-13
    assert np.abs(om[F:] * 2.0 * ell - pr.philox_normal(pr.rff_key(seed, pr.TAG_DIRECTION + 4), j, c)).max() <= 1e-13
    assert np.array_equal(ph, TWO_PI * pr.philox_uniform(pr.rff_key(seed, pr.TAG_PHASE), np.arange(2 * F), 0))
    keys = [pr.rff_key(seed, t) for t in (0, 1, 4, 5, 8)]
    assert pr.rff_key(seed, pr.TAG_EPS) not in keys and seed not in keys and pr.rff_key(seed, pr.TAG_EPS) != seed
    # Matern-5/2: the radial variable is the sum of 5 squared normals of tag 1
    om5 = _lib.rff_table("matern52", d, [1.4, 1.0, 0.1], F, seed=seed)[0]
    u = (pr.philox_normal(pr.rff_key(seed, pr.TAG_RADIAL), j, np.arange(5)[None, :]) ** 2).sum(axis=1)
    want = pr.philox_normal(pr.rff_key(seed, pr.TAG_DIRECTION), j, c) * np.sqrt(5.0 / u)[:, None] / 1.4
    assert np.abs(om5 - want).max() <= 1e-12 * np.abs(want).max()


def test_table_statuses():
    lib = _lib.load()
    th = np.array([1.0, 1.0, 0.1])
    ftot = C.c_int64(-1)

    def call(kid, p, F=16, d=2, theta=th):
        return lib.gphip_rff_table(kid, d, _lib._d(theta), p, F, 0, C.byref(ftot), None, None, None)
    assert call(_lib.kernel_id("se"), 3) == 0 and ftot.value == 16
    assert call(_lib.kernel_id("se"), 4) == 0                              # .. with the constant mean's entry
    assert call(_lib.kernel_id("se+rq+const"), 7) == 0 and ftot.value == 33
    assert call(_lib.kernel_id("se*rq"), 6) == 0 and ftot.value == 16
    assert call(100, 3) == 6 and call(_lib.kernel_id("null"), 1) == 6      # GPHIP_KERNEL_CUSTOM, the null kernel: GPHIP_ERR_UNSUPPORTED
    assert call(_lib.kernel_id("se"), 2) == 2 and call(_lib.kernel_id("se_ard"), 3) == 2      # a wrong p: GPHIP_ERR_DIM
    assert call(_lib.kernel_id("se"), 3, F=0) == 2
    assert call(77, 3) == 1                                                # an unknown id
    om, ph, amp = np.zeros((16, 2)), np.zeros(16), np.zeros(16)
    bad = np.array([0.0, 1.0, 0.1])
    assert lib.gphip_rff_table(_lib.kernel_id("se"), 2, _lib._d(bad), 3, 16, 0, C.byref(ftot), _lib._d(om), _lib._d(ph), _lib._d(amp)) == 1


def _small_problem(n=60, m=40, d=2, seed=2):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2.0, 2.0, size=(n, d))
    y = np.sin(X[:, 0]) + 0.5 * np.cos(2.0 * X[:, 1]) + 0.1 * rng.standard_normal(n)
    Xs = rng.uniform(-2.0, 2.0, size=(m, d))
    return X, y, Xs, np.array([0.9, 1.2, 1.1, 0.1, 0.2])              # se_ard, const mean


def test_reference_is_linear_gaussian_in_the_draw():
    X, y, Xs, th = _small_problem()
    om, ph, amp = _lib.rff_table("se_ard", 2, th, 256, seed=4)
    table = {"omega": om, "phase": ph, "amp": amp}
    mo = pr.moments("se_ard", th, X, y, Xs, table, "const")
    C_ = mo["cov"]
    assert np.max(np.abs(C_ - C_.T)) <= 1e-14 * np.max(np.abs(C_))
    assert np.linalg.eigvalsh(0.5 * (C_ + C_.T)).min() >= -1e-12 * np.max(np.diag(C_))
    rng = np.random.default_rng(9)
    w, eps = rng.standard_normal((5, 256)), 0.1 * rng.standard_normal((5, len(X)))
    f = pr.paths("se_ard", th, X, y, Xs, table, w, eps, "const", grad=False)["out"]
    lin = mo["mean"][None, :] + w @ mo["A"].T + eps @ mo["B"].T
    assert np.max(np.abs(f - lin)) <= 1e-12 * max(1.0, np.max(np.abs(f)))


def test_rff_error_of_the_posterior_covariance_is_recorded():
    X, y, Xs, th = _small_problem()
    exact = pr.exact_latent_cov("se_ard", th, X, Xs, "const")
    for F in (256, 16384):
        om, ph, amp = _lib.rff_table("se_ard", 2, th, F, seed=4)
        C_ = pr.moments("se_ard", th, X, y, Xs, {"omega": om, "phase": ph, "amp": amp}, "const")["cov"]
        err = np.max(np.abs(C_ - exact)) / np.max(np.diag(exact))
        print("RFF covariance error, F = %d: %.4f of max Sigma_ii" % (F, err))
        assert np.isfinite(err)
