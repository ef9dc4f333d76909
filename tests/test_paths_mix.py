"""The mixture paths object (gphip_paths_create_samples / gphip_paths_rows / gphip_paths_get_table), the parts that need no GPU:
the three symbols, the Batched=True route of samplePathsFromGaussianProcess against a stub handle that records its one call, and
argument validation in front of the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import paths_mix_reference as pmr
import paths_reference as pr
from bayesianinference_amd import _lib, gaussian_process as gp

NEW = ("gphip_paths_create_samples", "gphip_paths_rows", "gphip_paths_get_table")


def test_symbols_are_declared_exported_signed_and_bound():
    lib = _lib.load()
    declared = _lib.declared_symbols()
    for name in NEW:
        assert name in declared and name in _lib._SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name][1] and getattr(lib, name).restype is C.c_int
    assert [len(_lib._SIGNATURES[n][1]) for n in NEW] == [9, 3, 5]
    with open(_lib.HEADER) as f:
        header = f.read()
    assert re.search(r"int gphip_paths_create_samples\(gphip_handle h, const double\* Thetas[^;]*?, int R, int p,\s*const int\* counts[^;]*?, "
                     r"const uint64_t\* seeds[^;]*?, int F,\s*gphip_paths_handle\* out, int\* info[^;]*?\);", header)
    assert re.search(r"int gphip_paths_rows\(gphip_paths_handle q, int\* R, int\* row_of_draw[^)]*\);", header)
    assert re.search(r"int gphip_paths_get_table\(gphip_paths_handle q, int r, double\* omega[^,]*, double\* phase, double\* amp[^)]*\);", header)
    assert callable(_lib.Handle.sample_paths_samples) and callable(_lib.Paths.rows)
    # the new code lives in its own files, behind gphip_paths.inc
    csrc = os.path.join(os.path.dirname(_lib.__file__), "csrc")
    with open(os.path.join(csrc, "gphip.hip")) as f:
        tail = f.read()
    assert tail.index('#include "gphip_paths.inc"') < tail.index('#include "gphip_paths_mix.inc"')
    with open(os.path.join(csrc, "gphip_paths_mix.inc")) as f:
        assert '#include "gp_paths_mix.h"' in f.read()
    # without a device: NULL arguments are refused before anything else
    q, info, one = C.c_void_p(), (C.c_int * 1)(), (C.c_int * 1)(1)
    th, sd = (C.c_double * 3)(1.0, 1.0, 0.1), (C.c_uint64 * 1)(0)
    assert lib.gphip_paths_create_samples(None, th, 1, 3, one, sd, 8, C.byref(q), info) == 1 and not q.value
    assert lib.gphip_paths_rows(None, None, None) == 1 and lib.gphip_paths_get_table(None, 0, None, None, None) == 1


def test_the_reference_stacks_the_rows_in_draw_order():
    """paths_mix_reference.mix against paths_reference.paths row by row (the module adds no mathematics), and rows_of"""
    name, d, mean = pr.CASES[5]                                   # se_ard*matern32+const, d = 3, constant mean
    c = pr.case_reference(name, d, mean)
    X, y, Xs = c["X"][:40], c["y"][:40], c["Xs"][:5]
    th = pmr.rows_of(name, d, c["theta"])
    assert th.shape == (3, len(c["theta"])) and np.array_equal(th[0], c["theta"])
    idx = pmr.ell_index(name, d)
    other = [i for i in range(th.shape[1]) if i not in idx]
    assert np.allclose(th[1, idx], 0.8 * c["theta"][idx]) and np.allclose(th[2, idx], 1.25 * c["theta"][idx])
    assert np.array_equal(th[1, other], c["theta"][other]) and np.array_equal(th[2, other], c["theta"][other])
    counts, seeds, F = (2, 0, 3), (11, 12, 13), 16
    tables, ws, es = [], [], []
    for r in range(3):
        om, ph, amp = _lib.rff_table(name, d, th[r], F, seeds[r])
        tables.append({"omega": om, "phase": ph, "amp": amp})
        sn = abs(th[r][-2])
        ws.append(pr.philox_normal(seeds[r], np.arange(counts[r])[:, None], np.arange(len(ph))[None, :]))
        es.append(sn * pr.philox_normal(pr.rff_key(seeds[r], pr.TAG_EPS), np.arange(counts[r])[:, None], np.arange(len(X))[None, :]))
    w, eps = np.concatenate(ws), np.concatenate(es)
    assert np.array_equal(pmr.row_of_draw(counts), [0, 0, 2, 2, 2])
    got = pmr.mix(name, th, X, y, Xs, tables, w, eps, counts, mean)
    own = pmr.mix(name, th, X, y, np.broadcast_to(Xs, (5,) + Xs.shape), tables, w, eps, counts, mean, own=True)
    for r, sl in ((0, slice(0, 2)), (2, slice(2, 5))):
        one = pr.paths(name, th[r], X, y, Xs, tables[r], w[sl], eps[sl], mean)
        for k in ("v", "out", "dout"):
            assert np.array_equal(got[k][sl], one[k]), (r, k)
            assert np.abs(own[k][sl] - one[k]).max() <= 1e-12 * np.abs(one[k]).max(), (r, k)


class _StubPaths:
    S, d = 0, 1

    def close(self):
        pass


class _StubHandle:
    """records sample_paths_samples; the loop route's calls are counted to show that the batched route makes none"""
    d, kernel = 1, "se"

    def __init__(self):
        self.calls, self.fits = [], 0

    def fit(self, theta):
        self.fits += 1
        return 0

    def predict_draws(self, P, n, seed=0, latent=True):
        return np.zeros((n, len(P))), 0

    def sample_paths(self, *a):
        raise AssertionError("the loop route was taken")

    def sample_paths_samples(self, Thetas, counts, seeds, F=1024):
        self.calls.append((np.array(Thetas), list(counts), list(seeds), F))
        return _StubPaths()


def _stub_object(nsamples=7):
    rng = np.random.default_rng(4)
    X = np.linspace(0.0, 1.0, 12)[:, None]
    points = np.abs(rng.normal(1.0, 0.2, (nsamples, 3)))
    w = rng.random(nsamples)
    w[2] = 0.0                                                    # a sample that no draw picks
    stub = _StubHandle()
    obj = gp.inferenceObject({"Data": (X, np.sin(X)), "Samples": [{"Point": points[k], "CrudePosteriorWeight": w[k]} for k in range(nsamples)],
                              "GaussianProcessData": {"HIPHandle": stub, "ModelFunctions": {"NuggetFunction": None, "MeanFunction": None}}})
    return obj, stub, points


@pytest.mark.parametrize("n,seed", [(9, 0), (64, 3)])
def test_batched_route_makes_one_call_with_the_loop_routes_rows_counts_and_seeds(n, seed):
    obj, stub, points = _stub_object()
    f = gp.samplePathsFromGaussianProcess(obj, n, Features=48, seed=seed, Batched=True)
    assert len(stub.calls) == 1 and stub.fits == 0 and len(f._parts) == 1
    Th, counts, seeds, F = stub.calls[0]
    which = gp.gaussianProcessFunctionSamples(obj, np.linspace(0.0, 1.0, 3), n, seed=seed)["Sample"]
    used = np.unique(which)
    assert 2 not in used and len(used) >= 2
    assert np.array_equal(Th, points[used])                       # the distinct sampled thetas in ascending index
    assert counts == [int(c) for c in np.bincount(which)[used]] and sum(counts) == n and F == 48
    assert seeds == [int(np.random.SeedSequence([seed & (2**63 - 1), int(k)]).generate_state(1, np.uint64)[0]) for k in used]
    assert np.array_equal(f.sample, which)
    rows = f._parts[0][0]
    assert np.array_equal(rows, np.concatenate([np.flatnonzero(which == k) for k in used]))
    assert np.array_equal(np.sort(rows), np.arange(n))            # every draw once
    f.close()
    # the default stays the loop route
    with pytest.raises(AssertionError, match="loop route"):
        gp.samplePathsFromGaussianProcess(obj, n, Features=48, seed=seed)


def test_batched_is_ignored_in_the_direct_form_and_passed_on_by_thompson():
    import inspect
    assert inspect.signature(gp.samplePathsFromGaussianProcess).parameters["Batched"].default is False
    assert inspect.signature(gp.thompsonSampleFromGaussianProcess).parameters["Batched"].default is False
    assert gp.samplePathsFromGaussianProcess((np.zeros((3, 1)), np.zeros((3, 1))), 0, "se", [1.0, 1.0, 0.1], Batched=True) is None


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called: " + name)


def test_wrong_shapes_raise_before_the_library_is_touched():
    h = _lib.Handle.__new__(_lib.Handle)
    h._lib, h._h, h.N, h.d, h.p = _NoLibrary(), None, 10, 2, 4
    good = np.ones((3, 4))
    for Th, counts, seeds, F in ((np.ones((3, 5)), [1, 1, 1], [0, 1, 2], 8), (np.ones((0, 4)), [], [], 8), (np.ones((2, 3, 4)), [1, 1], [0, 1], 8),
                                 (good, [1, 1], [0, 1, 2], 8), (good, [1, 1, 1], [0, 1], 8), (good, [1, -1, 1], [0, 1, 2], 8),
                                 (good, [0, 0, 0], [0, 1, 2], 8), (good, [1, 1, 1], [0, 1, 2], 0)):
        with pytest.raises(ValueError):
            h.sample_paths_samples(Th, counts, seeds, F)
