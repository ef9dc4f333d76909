"""The abort word of the persistent kernels: a dependency wait that hits its spin limit sets it, and every later wait falls
through, so the results of that call are void.  Every route that waits on the word must turn a set word into GPHIP_ERR_HIP
that names the option switching the route off, and the handle must work on afterwards.  The test hook "debug_abort_word"
(it resolves under GPHIP_TEST_HOOKS=1, which tests/conftest.py sets) sets the word in front of the next launch of one kind:
1 dataflow Cholesky, 2 dataflow substitution / inverse, 3 single-vector substitution.  After the error the same call
without the hook gives bit-identical results to a fresh handle's (these routes are bit-repeatable)."""
import numpy as np
import pytest

from bayesianinference_amd import _lib, synthetic as syn

pytestmark = pytest.mark.gpu

ERR_HIP, ERR_STATE = 3, 4
D = 3
TH = syn.default_theta("se_ard", D)
XS = syn.make_test_points(100, D)
THS = TH[None, :] * (1.0 + 0.05 * np.arange(8))[:, None]

CALLS = {
    "grad": lambda h: h.loglik_grad(TH),
    "solve1": lambda h: (h.solve(np.random.default_rng(1).standard_normal(h.N)),),
    "solve8": lambda h: (h.solve(np.random.default_rng(8).standard_normal((h.N, 8))),),
    "predict": lambda h: h.predict(XS),
    "samples": lambda h: h.predict_samples(THS, XS),
    "loglik": lambda h: h.loglik(TH),
}


def _handle(n, opts, fit):
    X, y = syn.make_dataset(n, D)
    h = _lib.Handle(X, y, "se_ard")
    for k, v in opts.items():
        h.set_option(k, v)
    if fit:
        assert h.fit(TH) == 0
    return h


@pytest.mark.parametrize("n,kind,opts,fit,call,drops_fit,off", [
    (2600, 3, {"grad_potri": 0, "trsv": 1}, False, "grad", True, "trsv=0"),     # the gradient's alpha on the single-vector route
    (2048, 2, {"grad_potri": 1}, False, "grad", True, "grad_potri=2"),           # U = L^-T from the inverse launch
    (2600, 3, {}, True, "solve1", True, "trsv=0"),
    (2048, 2, {}, True, "solve8", True, "predict_df=0"),                         # forward + backward dataflow launches
    (2048, 2, {}, True, "predict", True, "predict_df=0"),
    (1024, 2, {}, False, "samples", False, "predict_df=0"),                      # one forward launch for all samples
    (2048, 1, {}, False, "loglik", False, "dataflow=0"),                         # fused single launch
])
def test_a_set_abort_word_fails_the_call_and_the_handle_works_on(n, kind, opts, fit, call, drops_fit, off):
    run = CALLS[call]
    h = _handle(n, opts, fit)
    h.set_option("debug_abort_word", kind)
    with pytest.raises(_lib.GphipError) as exc:
        run(h)
    assert exc.value.status == ERR_HIP and "timed out" in str(exc.value) and off in str(exc.value), exc.value
    assert h.get_option("debug_abort_word") == 0                                 # the hook fires once
    if drops_fit:
        for refused in ("solve1", "predict"):
            with pytest.raises(_lib.GphipError) as exc:
                CALLS[refused](h)
            assert exc.value.status == ERR_STATE, exc.value
        if fit:
            assert h.fit(TH) == 0
    got = run(h)
    ref = _handle(n, opts, fit)
    want = run(ref)
    h.close()
    ref.close()
    for a, b in zip(got, want):
        assert np.array_equal(np.asarray(a), np.asarray(b)), (call, a, b)
