"""The input dimensions every dispatch site of the device code is run at (tests/test_dim_dispatch.py on the host,
tests/test_gpu_dim_dispatch.py on the device).  Plain data: one record per site with

  "source"      where the dispatch lives,
  "thresholds"  what that site has in the sources today (tests/test_dim_dispatch.py reads the sources and compares),
  "edges"       the d after which another instantiation, window count or route takes over: every t here needs t and t + 1 in "d",
  "d"           the dimensions run, per kernel.

Rule for "d": t and t + 1 for every edge t, one interior value per interval, and for windowed routes one d that is an exact multiple
of the window and one that leaves a single-coordinate tail.  A new boundary in the sources means: update "thresholds" and "edges"
here and add the new boundary's d values.

A reference that cannot meet its own host check (tests/test_dim_dispatch.py) at some d is not used at that d and is listed under
"not_used"; there is none today.

theta(kernel, d, mean) is the hyper-parameter vector of every case.  The length scales are sqrt(d) x linspace(0.8, 1.3, d) (0.3
at d = 1): distinct, so that every length-scale derivative differs from its neighbours and a swapped or dropped coordinate shows,
and growing with sqrt(d), so that K stays far from diagonal on [-1, 1)^d (with length scales near 1 it is numerically diagonal from
d ~ 20 on and every comparison would pass on zeros)."""
import numpy as np

from oracle import gp_oracle as orc

SF, SN = 1.1, 0.15
SF2_TERM = 0.9                       # the second term's amplitude
ELL2_SCALE = 1.5                     # the second term's length scales against the first's
ALPHA, OFFSET, MU = 1.7, 0.3, 0.2

TWO_TERM = "se_ard*matern32_ard+const"
ONE_TERM = "rq_ard"

N_BUILD, M_CROSS = 150, 37           # builds, likelihoods, theta gradients (two 128-tiles, the last ragged)
N_XGRAD, M_XGRAD, M_INDUCING = 300, 130, 40
PATHS_SHAPE = {"n": 100, "S": 5, "F": 40, "points": 70}

_DIRECT = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16, 17, 24, 31, 32, 33]
_XG_ONE = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 48, 50]
_XG_TWO = [2, 4, 8, 9, 16, 17, 32, 33]
_PATHS = [1, 4, 5, 8, 9, 16, 17, 32, 33]

SITES = {
    "kbuild_direct": {
        "source": "gphip.hip launch_kbuild_kt",
        "thresholds": {"KB_CASE": [1, 2, 3, 4, 5, 6, 7, 8, 16], "KB_LDS_MAXD": 32},
        "edges": [1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 32],
        "d": {"se_ard": _DIRECT, "matern52_ard": _DIRECT},
    },
    "kbuild_mfma": {
        "source": "gphip.hip launch_kbuild_mfma_kt; stage_theta keeps d > KB_LDS_MAXD on the direct build (kbuild_direct runs 33)",
        "thresholds": {"KM_CASE": [1, 2, 3, 4], "KM_STEP": 4, "KB_LDS_MAXD": 32},
        "edges": [4, 8, 12, 16],
        "d": {"se_ard": [1, 4, 5, 8, 9, 12, 13, 16, 17, 32], "matern52_ard": [1, 4, 5, 8, 9, 12, 13, 16, 17, 32]},
    },
    "grad_reduce": {
        "source": "gphip.hip launch_grad_kt, launch_grad",
        "thresholds": {"GR_CASE": [1, 2, 3, 4, 5, 6, 7, 8, 16], "KB_LDS_MAXD": 32, "window": 32},
        "edges": [1, 2, 3, 4, 5, 6, 7, 8, 15, 16, 32],
        "d": {"se_ard": _DIRECT, "matern52_ard": _DIRECT},
    },
    "general_two_term": {
        "source": "gphip.hip launch_kbuild (kbuild_kernel<T, 0, 2>), launch_grad (grad_reduce_general_kernel)",
        "thresholds": {"KB_LDS_MAXD": 32, "window": 32},
        "edges": [32, 64],           # LDS | global memory; two windows of 32 | a third window of one coordinate
        "d": {TWO_TERM: [1, 5, 16, 17, 32, 33, 64, 65]},
    },
    "general_one_term": {
        "source": "as general_two_term, one term; with kbuild_mfma the matrix-pipe build of the family",
        "thresholds": {"KB_LDS_MAXD": 32},
        "edges": [],
        "d": {ONE_TERM: [9, 32]},
    },
    "grad_rows": {
        "source": "gphip.hip grad_rows: per-workgroup rows while 4 np 8 <= 8192 bytes, np = 2 d + 6, else atomics",
        "thresholds": {"staging_bytes": 8192},
        "edges": [125],
        "d": {"se_ard": [125, 126]},
    },
    "theta_packed": {
        "source": "gphip.hip eval_chunk: theta as kernel arguments while B (d + SLOTP) <= THETA_PACK",
        "thresholds": {"THETA_PACK": 320, "SLOTP": 16},
        "edges": [],                 # in (B, d): see "Bd"
        "Bd": [(8, 24), (8, 25), (1, 304), (1, 305)],
        "d": {"se_ard": [24, 25, 304, 305]},
    },
    "predict_xgrad_one_term": {
        "source": "gphip_xgrad.inc queue_xgrad",
        "thresholds": {"chain": [2, 4, 8, 16, "KB_LDS_MAXD"], "KB_LDS_MAXD": 32, "window": 16},
        "edges": [2, 4, 8, 16, 32],  # beyond 32: windows of 16 (48: three whole windows; 33: a tail of one coordinate)
        "d": {"se_ard": _XG_ONE},
    },
    "predict_xgrad_two_terms": {
        "source": "gphip_xgrad.inc queue_xgrad",
        "thresholds": {"chain": [2, 4, 8, 16, "KB_LDS_MAXD"], "KB_LDS_MAXD": 32, "window": 16},
        "edges": [2, 4, 8, 16, 32],  # beyond 16: windows of 16 (32: two whole windows; 17, 33: a tail of one coordinate)
        "d": {TWO_TERM: [2, 3, 4, 5, 8, 9, 16, 17, 32, 33]},
    },
    "sparse_zgrad_one_term": {
        "source": "gphip_sparse.inc sparse_queue_zgrad",
        "thresholds": {"chain": [2, 4, 8, 16, "KB_LDS_MAXD"], "KB_LDS_MAXD": 32, "window": 16},
        "edges": [2, 4, 8, 16, 32],
        "d": {"se_ard": _XG_ONE},
    },
    "sparse_zgrad_two_terms": {
        "source": "gphip_sparse.inc sparse_queue_zgrad",
        "thresholds": {"chain": [2, 4, 8, 16, "KB_LDS_MAXD"], "KB_LDS_MAXD": 32, "window": 16},
        "edges": [2, 4, 8, 16, 32],
        "d": {TWO_TERM: [2, 3, 4, 5, 8, 9, 16, 17, 32, 33]},
    },
    "paths": {
        "source": "gphip_paths.inc queue_paths_contract (gradient windows of PC_GW coordinates)",
        "thresholds": {"chain": [8, 16, "KB_LDS_MAXD"], "KB_LDS_MAXD": 32, "PC_GW": 4},
        "edges": [4, 8, 16, 32],     # 4 | 5: one gradient window | a second one of one coordinate
        "d": {"matern52_ard": _PATHS},
    },
    "paths_own": {
        "source": "gphip_paths.inc queue_paths_own",
        "thresholds": {"chain": [8, 16], "KB_LDS_MAXD": 32, "PO_GW": 8},
        "edges": [8, 16, 32],        # beyond 32: gradient windows of PO_GW (33: four windows and a tail of one coordinate)
        "d": {"matern52_ard": _PATHS},
    },
    "rtc": {
        "source": "rtc_dyn.h: the program specialised for the handle's d up to RTC_SPEC_MAXD",
        "thresholds": {"RTC_SPEC_MAXD": 32},
        "edges": [32],
        "d": {"se_ard_source_text": [9, 32, 33]},
    },
}

NOT_USED = {}                        # (site, kernel, d) -> why its reference is not used there


def lengthscales(d, scale=1.0):
    return np.array([0.3 * scale]) if d == 1 else scale * np.sqrt(d) * np.linspace(0.8, 1.3, d)


def theta(kernel, d, mean="zero"):
    """[term 1: l.., (alpha), sf] [term 2 ..] [c] sn [mu]  (the oracle's layout) for any kernel of the oracle's grammar"""
    if kernel == "se_ard_source_text":
        kernel = "se_ard"
    terms, _, offset = orc.parse_kernel(kernel)
    th = []
    for k, t in enumerate(terms):
        ell = lengthscales(d, ELL2_SCALE if k else 1.0)
        if orc.n_lengthscales(t, d) == 1:
            ell = ell[len(ell) // 2:len(ell) // 2 + 1]
        th += list(ell)
        if t.startswith("rq"):
            th.append(ALPHA)
        th.append(SF2_TERM if k else SF)
    if offset:
        th.append(OFFSET)
    th.append(SN)
    if mean == "const":
        th.append(MU)
    out = np.array(th, dtype=np.float64)
    assert len(out) == orc.n_params(kernel, d, mean)
    return out


def theta_rows(kernel, d, B, mean="zero"):
    """B rows: row s has every length scale of theta(..) times 1 + 0.07 s (the rule of tests/test_gpu_grad_batch.py)"""
    th = theta(kernel, d, mean)
    terms, _, _ = orc.parse_kernel(kernel)
    rows = np.tile(th, (B, 1))
    o = 0
    for t in terms:
        nl = orc.n_lengthscales(t, d)
        for s in range(B):
            rows[s, o:o + nl] *= 1.0 + 0.07 * s
        o += nl + (1 if t.startswith("rq") else 0) + 1
    return rows


MEAN = {"se_ard": "zero", "matern52_ard": "zero", ONE_TERM: "zero", TWO_TERM: "const", "se_ard_source_text": "zero"}
PATHS_MEAN = "const"
_cache = {}


def _frozen(dct):
    for v in dct.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return dct


def build_data(kernel, d):
    """{"X", "y", "Xs", "theta", "mean_kind"} of a build / likelihood / theta-gradient case: seeded, computed once, left unchanged"""
    key = ("build", kernel, d)
    if key not in _cache:
        from bayesianinference_amd import synthetic as syn
        X, y = syn.make_dataset(N_BUILD, d)
        _cache[key] = _frozen({"X": X, "y": y, "Xs": syn.make_test_points(M_CROSS, d), "theta": theta(kernel, d, MEAN[kernel]),
                               "mean_kind": MEAN[kernel]})
    return _cache[key]


def xgrad_data(kernel, d):
    """the inputs of an input-gradient case in the shapes of tests/predict_grad_reference.py: N = 300, M = 130, test point 7 on
    training point 11, m = 40 inducing points, jitter 1e-6 sf^2"""
    key = ("xgrad", kernel, d)
    if key not in _cache:
        import predict_grad_reference as pg
        from bayesianinference_amd import synthetic as syn
        X, y = syn.make_dataset(N_XGRAD, d)
        Xs = syn.make_test_points(M_XGRAD, d).copy()
        Xs[pg.COINCIDE[0]] = X[pg.COINCIDE[1]]
        _cache[key] = _frozen({"X": X, "y": y, "Xs": Xs, "theta": theta(kernel, d, MEAN[kernel]), "mean_kind": MEAN[kernel],
                               "kernel": kernel, "Z": pg.inducing_of(X, M_INDUCING), "jitter": pg.JREL * SF ** 2})
    return _cache[key]


def xgrad_reference(kernel, d):
    """xgrad_data + the numpy reference of gphip_predict_grad: "mean", "var", "dmean", "dvar" """
    key = ("xgrad_exact", kernel, d)
    if key not in _cache:
        import predict_grad_reference as pg
        c = dict(xgrad_data(kernel, d))
        c.update(pg.exact(kernel, c["theta"], c["X"], c["y"], c["Xs"], c["mean_kind"]))
        _cache[key] = _frozen(c)
    return _cache[key]


def sparse_reference(kernel, d):
    """xgrad_data + the numpy references of the sparse object: gphip_sparse_predict_grad ("mean", "var", "dmean", "dvar") and the
    bound's gradient in the inducing locations ("gradZ"; "gradZ_torch" and "route_difference" as sparse_zgrad_reference has them)"""
    key = ("sparse", kernel, d)
    if key not in _cache:
        import predict_grad_reference as pg
        import sparse_zgrad_reference as zg
        c = dict(xgrad_data(kernel, d))
        a = (kernel, c["theta"], c["X"], c["y"], c["Z"], c["jitter"])
        c.update(pg.sparse(*a, c["Xs"], c["mean_kind"]))
        c["gradZ"] = zg.analytic(*a, c["mean_kind"])
        c["gradZ_torch"] = zg.autograd(*a, c["mean_kind"])[2]
        c["route_difference"] = float(np.abs(c["gradZ"] - c["gradZ_torch"]).max() / np.abs(c["gradZ"]).max())
        _cache[key] = _frozen(c)
    return _cache[key]


def paths_data(kernel, d):
    """the inputs of a pathwise-draw case in the shapes of the existing d = 40 tests: n = 100, 70 points, 5 draws x 7 own points"""
    key = ("paths", kernel, d)
    if key not in _cache:
        from bayesianinference_amd import synthetic as syn
        X, y = syn.make_dataset(PATHS_SHAPE["n"], d)
        S = PATHS_SHAPE["S"]
        P = syn.make_test_points(S * 7, d).reshape(S, 7, d).copy()
        P[2, 3] = X[11]                                  # a pair on a training point
        _cache[key] = _frozen({"X": X, "y": y, "Xs": syn.make_test_points(PATHS_SHAPE["points"], d), "own": P,
                               "theta": theta(kernel, d, PATHS_MEAN), "mean_kind": PATHS_MEAN})
    return _cache[key]


def cases(site):
    """[(site, kernel, d)] of one site"""
    return [(site, k, d) for k, ds in SITES[site]["d"].items() for d in ds]


def case_id(case):
    return "%s-%s-d%d" % case
