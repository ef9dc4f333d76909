"""The one prediction pass of sparse objects as gphip_sparse_predict / gphip_sparse_predict_pw run it: one
slot, the resident fit.  The hand-over kernel against the copy + norm launch it replaced, several passes over the test points
(option "sparse_samples_chunk", which caps the one-theta call too), one test point, one full tile, and the phase times.  The cases
are those of tests/sparse_samples_cases.py and tests/sparse_pw_reference.py, whose numpy side tests/test_sparse_samples.py and
tests/test_sparse_pw.py pin on the CPU; all have M = 300 test points (three tiles, the last with 44 points), and m = 150 inducing
points (m_pad = 256: 106 pad columns that the hand-over copies and must not sum) except the seams case (m = 300, three tile columns).
Bars are those of tests/test_gpu_sparse.py: 1e-7 x max |y| for means, 1e-7 x max k(x, x) for variances."""
import functools

import numpy as np
import pytest

import sparse_batch_cases as cases
import sparse_pw_reference as pw
import sparse_reference as ref
import sparse_samples_cases as sc
from bayesianinference_amd import _lib, synthetic as syn

pytestmark = pytest.mark.gpu

TOL = 1e-7
SAMPLES_PHASES = ["ms_samples_v1", "ms_samples_handover", "ms_samples_v2", "ms_samples_reduce"]
SUBJECTS = ["se_ard", "nonstat", "seams", "pw"]


def _frozen(a):
    a = np.asarray(a)
    a.setflags(write=False)
    return a


class Subject:
    """One object and one theta: how to open and fit it, how to predict at the first k test points, and the numpy reference."""

    def __init__(self, label):
        self.label = label
        self.mt = self.nt = None
        if label == "pw":                       # (1333, 3, 150), constant mean in theta: CASES[0] of tests/sparse_pw_reference.py
            name, n, d, m, self.mean = pw.CASES[0]
            self.X, self.y = syn.make_dataset(n, d)
            self.kernel, self.th, self.jit = pw.kernel_of(name, d), pw.theta(name, d, self.mean), pw.JITTER
            self.Z = pw.inducing(self.X, m, None)
            self.Xs = sc.test_points(d)
            sn2, _ = ref.noise_and_mean(self.kernel, self.th, d, self.mean)
            self.mv, self.nu = pw.trend(self.X), pw.noise(self.X, sn2)
            # m(x*) a ramp in the INDEX of the test point (a slice that starts at the wrong offset is off by 0.01 x the offset),
            # nu(x*) different from index to index
            self.mt, self.nt = _frozen(0.2 + 0.01 * np.arange(sc.M)), _frozen(pw.noise(self.Xs, sn2))
        elif label == "seams":
            self.X, self.y, self.Z, self.mean, rows, self.Xs, self.seams_want = sc.seams_case()
            self.kernel, self.th, self.jit = "se_ard", rows[0], cases.JITTER
        else:
            self.kernel, self.X, self.y, self.Z, self.mean, rows, self.jit, _ = sc.case({"se_ard": "parity0", "nonstat": "nonstat"}[label])
            self.th = rows[0]
            self.Xs = sc.test_points(self.X.shape[1])
        self.ymax = float(np.abs(self.y).max())
        self.kmax = float(ref.kdiag(self.kernel, self.th, self.X, self.mean).max())

    def open(self):
        h = _lib.SparseHandle(self.X, self.y, self.Z, self.kernel, self.mean)
        info = h.fit_pw(self.th, self.jit, self.mv, self.nu) if self.label == "pw" else h.fit(self.th, self.jit)
        assert info == 0
        return h

    def predict(self, h, latent, k=sc.M):
        if self.label == "pw":
            return h.predict_pw(self.Xs[:k], latent, self.mt[:k], self.nt[:k])
        return h.predict(self.Xs[:k], latent=latent)

    @functools.lru_cache(maxsize=None)
    def want(self, latent):
        if self.label == "pw":
            mu, var = pw.predict_formulas(self.kernel, self.th, self.X, self.y, self.Z, self.jit, self.Xs, self.mv, self.nu, self.mt, self.nt,
                                          self.mean, latent)
        elif self.label == "seams" and not latent:
            mu, var = self.seams_want["mean"][0], self.seams_want["var"][0]
        elif self.label == "seams":                                 # (the case module keeps the noisy reference only)
            mu, var = ref.predict_formulas(self.kernel, self.th, self.X, self.y, self.Z, self.jit, self.Xs, self.mean, latent)
        else:
            w = sc.reference({"se_ard": "parity0", "nonstat": "nonstat"}[self.label], latent)
            mu, var = w["mean"][0], w["var"][0]
        return _frozen(mu), _frozen(var)

    def within_bars(self, got, latent, what, k=sc.M):
        wm, wv = self.want(latent)
        em, ev = np.abs(got[0] - wm[:k]).max() / self.ymax, np.abs(got[1] - wv[:k]).max() / self.kmax
        print(f"{self.label} latent={latent} {what}: mean {em:.2e} var {ev:.2e}")
        assert got[0].shape == (k,) and got[1].shape == (k,)
        assert em <= TOL and ev <= TOL, (self.label, latent, what)


@functools.lru_cache(maxsize=None)
def subject(label):
    return Subject(label)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- 1. both hand-over forms return the same bytes
@pytest.mark.parametrize("label", SUBJECTS)
def test_one_theta_both_handover_forms_same_bytes(label):
    s = subject(label)
    h = s.open()
    assert h.get_option("sparse_samples_handover") == 1
    for latent in (False, True):
        a = s.predict(h, latent)
        s.within_bars(a, latent, "hand-over kernel")
        assert _same(a, s.predict(h, latent))                       # a second call: the same bytes
        h.set_option("sparse_samples_handover", 0)
        b = s.predict(h, latent)
        s.within_bars(b, latent, "copy + norm launch")
        assert _same(b, s.predict(h, latent))
        h.set_option("sparse_samples_handover", 1)
        assert _same(a, b), (label, latent)
    h.close()


# ---- 2. several passes
@pytest.mark.parametrize("label", SUBJECTS)
def test_one_theta_in_several_passes(label):
    s = subject(label)
    h = s.open()
    for latent in (False, True):
        before = s.predict(h, latent)
        assert h.get_option("last_sparse_samples_chunk") == 384      # by the rule: all 300 points, three tiles
        h.set_option("sparse_samples_chunk", 128)                    # passes of 128, 128 and 44 points
        got = s.predict(h, latent)
        assert h.get_option("last_sparse_samples_chunk") == 128
        s.within_bars(got, latent, "in passes of 128")
        print(f"{label} latent={latent}: largest difference to the unchunked call: mean {np.abs(got[0] - before[0]).max():.2e} "
              f"var {np.abs(got[1] - before[1]).max():.2e}")
        h.set_option("sparse_samples_chunk", 100)                    # rounded up to 128
        assert _same(got, s.predict(h, latent)) and h.get_option("last_sparse_samples_chunk") == 128
        h.set_option("sparse_samples_chunk", 0)
        assert _same(before, s.predict(h, latent))                   # the default call's bytes are those of before
        assert h.get_option("last_sparse_samples_chunk") == 384
    h.close()


# ---- 3. one test point; one full tile without pad rows
@pytest.mark.parametrize("label", ["se_ard", "nonstat", "pw"])
def test_one_test_point_and_one_full_tile(label):
    s = subject(label)
    h = s.open()
    for k in (1, 128):
        for latent in (False, True):
            s.within_bars(s.predict(h, latent, k), latent, f"M = {k}", k)
        assert h.get_option("last_sparse_samples_chunk") == 128
    h.close()


# ---- 4. phases
def test_one_theta_prediction_fills_and_resets_the_phases():
    s = subject("se_ard")
    h = s.open()
    h.set_option("profile", 1)

    def read():
        return [h.get_option(k) for k in SAMPLES_PHASES]

    assert all(v == 0 for v in read())                               # nothing predicted yet
    h.set_option("sparse_samples_chunk", 128)
    s.predict(h, False)                                              # three passes
    first = read()
    print("three passes", dict(zip(SAMPLES_PHASES, first)))
    assert all(v > 0 for v in first)
    F, info = h.bound(s.th, s.jit)                                   # the bound resets its own phases, not these
    assert info == 0 and read() == first
    s.predict(h, False, 1)                                           # one pass of one point: each call resets its phases, so every
    second = read()                                                  # one is below the three passes' (it would be above if it added)
    print("one pass", dict(zip(SAMPLES_PHASES, second)))
    assert all(0 < b < a for a, b in zip(first, second))
    h.close()
