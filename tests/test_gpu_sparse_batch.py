"""The batched sparse bound on the device (gphip_sparse_bound_batch) and the native sampler on a sparse object
(gphip_sparse_nested_sampling), against the numpy reference of tests/sparse_reference.py and against the one-theta entry point.
The numpy side of every case (conditioning, agreement of the reference's two routes, the row that must fail) is checked on the
CPU by tests/test_sparse_batch.py.  Bars: 1e-8 relative for F and each part against the reference (tests/test_gpu_sparse.py),
1e-12 relative between the batched and the one-theta evaluation of the same theta (the bar of that file's chunk / strip test)."""
import math

import numpy as np
import pytest

import sparse_batch_cases as cases
import sparse_reference as ref
from bayesianinference_amd import _lib, gaussian_process as gp, nested_sampling as ns, synthetic as syn

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return abs(a - b) / abs(b)


def _check_rows(h, kernel, rows, X, y, Z, jit, mean, label, tol=1e-8, tol_one=1e-12):
    F, info, parts = h.bound_batch(rows, jit, parts=True)
    assert F.shape == (len(rows),) and parts.shape == (len(rows), 5)
    for s, th in enumerate(rows):
        want = ref.bound_formulas(kernel, th, X, y, Z, jit, mean)
        one, info1 = h.bound(th, jit)
        eF = _rel(F[s], want["F"])
        eP = max(_rel(a, b) for a, b in zip(parts[s], want["parts"]))
        e1 = _rel(F[s], one)
        print(f"{label} row {s}: F {F[s]:.8f} reference {want['F']:.8f} rel {eF:.2e} parts {eP:.2e} one-theta {e1:.2e}")
        assert info[s] == 0 and info1 == 0
        assert eF <= tol and eP <= tol
        assert e1 <= tol_one
    return F, parts


@pytest.mark.parametrize("name,n,d,m,mean,B", cases.PARITY)
def test_parity_with_the_reference_and_the_one_theta_call(name, n, d, m, mean, B):
    X, y, Z, kernel, rows = cases.parity_case(name, n, d, m, mean, B)
    h = _lib.SparseHandle(X, y, Z, kernel, mean)
    _check_rows(h, kernel, rows, X, y, Z, cases.JITTER, mean, f"{name} N={n} m={m}")
    assert h.get_option("last_sparse_slots") == B                   # one group
    h.close()


def test_default_jitter_is_applied_per_row():
    X, y = syn.make_dataset(1333, 3)
    Z = cases.inducing(X, 150)
    rows = np.array([np.concatenate([np.linspace(0.8, 1.3, 3), [sf, 0.15, 0.2]]) for sf in (0.5, 1.1, 2.0)])
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const")
    F, info = h.bound_batch(rows, -1.0)
    for s, th in enumerate(rows):
        one, info1 = h.bound(th, -1.0)
        jit = h.get_option("last_jitter")
        print(f"sf {th[3]}: batch {F[s]:.10f} one-theta {one:.10f} rel {_rel(F[s], one):.2e} jitter {jit:.3e}")
        assert jit == pytest.approx(1e-10 * th[3] ** 2, rel=1e-12)
        assert info[s] == 0 and info1 == 0 and _rel(F[s], one) <= 1e-12
    h.bound_batch(rows, -1.0)
    assert h.get_option("last_jitter") == pytest.approx(1e-10 * 2.0 ** 2, rel=1e-12)      # the last row's
    h.close()


def test_failures_stay_in_their_row():
    X, y, Z, rows = cases.failure_case()
    h = _lib.SparseHandle(X, y, Z, "se_ard", "zero")
    single = [h.bound(th, 0.0) for th in rows]
    assert [i for _, i in single] == [0, _lib.INFO_NAN, 0, _lib.INFO_NOT_SPD, 0]
    assert h.fit(rows[0], 0.0) == 0
    h.predict(X[:5])
    F, info, parts = h.bound_batch(rows, 0.0, parts=True)
    print("info", info, "F", F)
    assert list(info) == [i for _, i in single]
    for s in (1, 3):
        assert np.isnan(F[s]) and np.all(np.isnan(parts[s]))
    for s in (0, 2, 4):
        want = ref.bound_formulas("se_ard", rows[s], X, y, Z, 0.0, "zero")
        eP = max(_rel(a, b) for a, b in zip(parts[s], want["parts"]))
        print(f"row {s}: rel {_rel(F[s], want['F']):.2e} parts {eP:.2e}")
        assert _rel(F[s], want["F"]) <= 1e-8 and eP <= 1e-8
    with pytest.raises(_lib.GphipError) as e:                    # the batch dropped the fit
        h.predict(X[:5])
    assert e.value.status == 4
    one, info1 = h.bound(rows[2], 0.0)
    assert info1 == 0 and _rel(one, ref.bound_formulas("se_ard", rows[2], X, y, Z, 0.0, "zero")["F"]) <= 1e-8
    h.close()


def test_determinism_and_layout_independence():
    import torch
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    X, y, Z, kernel, rows = cases.parity_case(*cases.DETERMINISM)
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const")
    jit = cases.JITTER
    F0, i0, p0 = h.bound_batch(rows, jit, parts=True)
    F1, i1, p1 = h.bound_batch(rows, jit, parts=True)
    assert np.all(i0 == 0) and np.array_equal(F0, F1) and np.array_equal(p0, p1)         # the same bytes
    assert h.get_option("last_sparse_slots") == 5
    want = cases.expected_nsplit(384, 1536, 5, ncu)
    print("CUs", ncu, "strips", h.get_option("last_sparse_nsplit"), "rule", want)
    assert h.get_option("last_sparse_nsplit") == want
    perm = np.array([3, 0, 4, 1, 2])
    Fp, ip, pp = h.bound_batch(rows[perm], jit, parts=True)
    assert np.array_equal(Fp, F0[perm]) and np.array_equal(pp, p0[perm])
    for key, val in (("sparse_batch_slots", 2), ("sparse_chunk", 512), ("sparse_split", 4)):
        for k in ("sparse_batch_slots", "sparse_chunk", "sparse_split"):
            h.set_option(k, 0)
        h.set_option(key, val)
        if key == "sparse_batch_slots":
            h.bound_batch(rows[:4], jit)
            assert h.get_option("last_sparse_slots") == 2            # two groups of two rows
        Fa, ia, pa = h.bound_batch(rows, jit, parts=True)
        Fb, ib, pb = h.bound_batch(rows, jit, parts=True)
        assert np.all(ia == 0) and np.array_equal(Fa, Fb) and np.array_equal(pa, pb), key
        err = max(_rel(a, b) for a, b in zip(Fa, F0))
        print(key, val, "max rel to the default", f"{err:.2e}", "slots", h.get_option("last_sparse_slots"), "chunk",
              h.get_option("last_sparse_chunk"), "strips", h.get_option("last_sparse_nsplit"))
        assert err <= 1e-12, key
        if key == "sparse_batch_slots":
            assert h.get_option("last_sparse_slots") == 1            # three groups: 2, 2 and 1 row
        else:
            assert h.get_option("last_sparse_slots") == 5
        if key == "sparse_chunk":
            assert h.get_option("last_sparse_chunk") == 512          # three chunks of the 1500 data points
        if key == "sparse_split":
            assert h.get_option("last_sparse_nsplit") == 4
    h.close()


# fp32 objects against the fp64 reference at N = 2000, d = 3, m = 300, sn = 0.15, sf = 1.1, default fp32 jitter (1e-4 k(x, x)).
# Measured: F 1.99e-5 relative, parts at most 5.07e-6, means 5.49e-5 max |y|, variances 3.99e-6 sf^2;
# the bars are 4 x those, the rule section 8b used for leave-one-out.  (Copied from tests/test_gpu_sparse.py: the same
# quantities on the same case; its first row is that file's theta.)
FP32_BARS = {"F": 4 * 1.99e-5, "parts": 4 * 5.07e-6}


def test_fp32_object_against_the_fp64_reference():
    X, y = syn.make_dataset(2000, 3)
    Z = cases.inducing(X, 300)
    base = cases.base_theta("se_ard", 3, "const")
    rows = np.array([base, base * np.array([1.05, 0.96, 1.03, 1.0, 1.1, 0.5]), base * np.array([0.95, 1.04, 0.97, 1.0, 1.2, 1.5])])
    h = _lib.SparseHandle(X, y, Z, "se_ard", "const", dtype=32)
    F, info, parts = h.bound_batch(rows, -1.0, parts=True)
    jit = 1e-4 * cases.SF ** 2                                   # every row has sf = SF
    assert h.get_option("last_jitter") == pytest.approx(jit, rel=1e-12)
    h.close()
    for s, th in enumerate(rows):
        want = ref.bound_formulas("se_ard", th, X, y, Z, jit, "const")
        eF, eP = _rel(F[s], want["F"]), max(_rel(a, b) for a, b in zip(parts[s], want["parts"]))
        print(f"fp32 row {s}: F {eF:.2e} parts {eP:.2e}")
        assert info[s] == 0 and eF <= FP32_BARS["F"] and eP <= FP32_BARS["parts"]


def test_status_contract():
    X, y = syn.make_dataset(300, 2)
    h = _lib.SparseHandle(X, y, cases.inducing(X, 40), "se_ard", "zero")
    th = np.array([[0.9, 1.1, 1.0, 0.12], [1.0, 1.0, 1.1, 0.2]])
    with pytest.raises(_lib.GphipError) as e:
        h.bound_batch(th[:, :-1], 1e-6)
    assert e.value.status == 2
    with pytest.raises(_lib.GphipError) as e:
        h.bound_batch(th, float("nan"))
    assert e.value.status == 1
    F, info = h.bound_batch(np.zeros((0, 4)), 1e-6)
    assert F.shape == (0,) and info.shape == (0,)
    F, info, parts = h.bound_batch(np.zeros((0, 4)), 1e-6, parts=True)
    assert parts.shape == (0, 5)
    F, info = h.bound_batch(th, 1e-6)
    assert np.all(info == 0) and np.all(np.isfinite(F))
    h.close()


SAMPLER_VARIABLES, SAMPLER_JITTER = cases.SAMPLER_VARIABLES, cases.SAMPLER_JITTER
_sampler_case = cases.sampler_case               # N = 400, d = 1, m = 32; why its noise is 0.4: see there


def test_native_sampler_on_a_sparse_object_matches_grid_integration():
    """The log evidence against the 24^3 midpoint grid, every grid value from bound_batch, to 4 se + 0.25 (the bar of
    test_native_sampler_on_a_gp_matches_grid_integration_and_the_python_driver).  tests/test_sparse_batch.py shows in numpy that
    this grid has converged for the case's data (24^3 and 36^3 agree to 0.002).  The device's grid value is held to that numpy
    value here as well, to 2e-8 relative (1e-8 for each of the two against the reference's bound), so the grid is a reference
    in its own right and not the code under test twice."""
    X, y, Z, box = _sampler_case()
    h = _lib.SparseHandle(X, y, Z, "se")
    _, grid = cases.sampler_grid(cases.SAMPLER_GRID)
    vals = np.empty(len(grid))
    for s0 in range(0, len(grid), 1152):
        v, info = h.bound_batch(grid[s0:s0 + 1152], SAMPLER_JITTER)
        vals[s0:s0 + 1152] = np.where(info == 0, v, -np.inf)
    want = ns.log_sum_exp(vals) - math.log(len(grid))
    host = cases.sampler_grid_bound(X, y, Z, cases.SAMPLER_GRID, SAMPLER_JITTER).ravel()
    want_host = ns.log_sum_exp(host) - math.log(len(grid))
    print(f"grid log evidence: device {want:.8f} numpy {want_host:.8f}")
    assert abs(want - want_host) <= 2e-8 * abs(want_host)
    res = h.nested_sampling(box, SAMPLER_JITTER, pool=100, mc_steps=30, walkers=32, seed=11)
    h.close()
    out = ns.evidence_sampling(res, [v[0] for v in SAMPLER_VARIABLES], 100, np.random.default_rng(0))
    z, se = out["LogEvidence"]["Mean"], out["LogEvidence"]["StandardError"]
    print(f"log evidence {z:.4f} +- {se:.4f}, grid {want:.4f}, evaluations {res['LikelihoodEvaluations']}")
    assert abs(z - want) < 4 * se + 0.25, (z, se, want)


def test_native_sampler_on_a_sparse_object_repeats_and_counts_its_evaluations():
    X, y, Z, box = _sampler_case()
    h = _lib.SparseHandle(X, y, Z, "se")
    res = h.nested_sampling(box, SAMPLER_JITTER, pool=100, mc_steps=30, walkers=32, seed=11)
    again = h.nested_sampling(box, SAMPLER_JITTER, pool=100, mc_steps=30, walkers=32, seed=11)
    assert np.array_equal(again["Points"], res["Points"]) and np.array_equal(again["LogLikelihood"], res["LogLikelihood"])
    assert res["LikelihoodEvaluations"] >= 100 + 30 * 32
    assert res["TotalSamples"] > 100 and np.all(np.isfinite(res["LogLikelihood"]))
    # every sample's value is the bound at its point
    F, info = h.bound_batch(res["Points"][:64], SAMPLER_JITTER)
    assert np.all(info == 0) and np.max(np.abs(F - res["LogLikelihood"][:64]) / np.abs(F)) <= 1e-12
    with pytest.raises(_lib.GphipError):
        h.nested_sampling(np.array([[1.0, 1.0], [0.2, 3.0], [0.03, 0.6]]), SAMPLER_JITTER)             # lo == hi
    assert h.get_option("last_sparse_slots") > 1
    h.close()


def test_python_nested_sampling_on_a_sparse_object_batches_its_steps():
    X, y, Z, _ = _sampler_case()
    obj = gp.defineSparseGaussianProcess((X, y), "SE", Z, variables=SAMPLER_VARIABLES, Jitter=SAMPLER_JITTER)
    assert not obj.failed
    res = ns.nestedSampling(obj, SamplePoolSize=20, MaxIterations=30, MinIterations=10, Seed=3)
    assert not isinstance(res, str) and "Samples" in res
    hh = obj["SparseGaussianProcessData"]["HIPHandle"]
    assert hh.get_option("last_sparse_slots") > 1                # the Python driver really batched
    hh.close()
