"""The table of tests/dim_dispatch_cases.py against the sources and against itself, the part that needs no GPU.

1. Thresholds.  Every dispatch on the input dimension d is read from the sources (comments stripped, simple regular expressions,
   as tests/test_source_lint.py does) and compared with what the table records.  A failure here means: a boundary moved or a case
   was added or dropped -- update "thresholds" and "edges" of the site in tests/dim_dispatch_cases.py AND add the new boundary's d
   values (t and t + 1) to its "d", so that tests/test_gpu_dim_dispatch.py runs both sides of it.
2. Coverage.  Every site's d list holds t and t + 1 for every edge t it records.
3. Conditions on the inputs.  For every (site, kernel, d): the median off-diagonal correlation of the noise-free K is in
   [0.1, 0.9] and cond(K) <= 1e5 -- no comparison passes on a numerically diagonal or a numerically singular matrix.
4. The references against their own second route at every d of the table: the oracle's analytic theta-gradient against the
   autograd one of tests/loglik_grad_reference.py (1e-9 of max |gradient|; SE / Matern-5/2), predict_grad_reference.exact /
   .sparse against their autograd twins (1e-10, the bar of tests/test_predict_grad.py), the inducing-location gradient's two
   routes (the bar of tests/test_sparse_zgrad.py), the pathwise reference against its linear-Gaussian form (tests/test_paths.py)."""
import os
import re

import numpy as np
import pytest

import dim_dispatch_cases as dc
import loglik_grad_reference as lgr
import paths_reference as pr
import predict_grad_reference as pg
from bayesianinference_amd import _lib, build
from oracle import gp_oracle as orc
from test_predict_grad import ROUTE_BAR as XGRAD_ROUTE_BAR
from test_sparse_zgrad import ROUTE_BAR as ZGRAD_ROUTE_BAR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bayesianinference_amd", "csrc")
HINT = ("a dispatch threshold changed in the sources: update the site's \"thresholds\" and \"edges\" in tests/dim_dispatch_cases.py "
        "and add the new boundary's d values (t and t + 1) to its \"d\"")
THETA_GRAD_ROUTE_BAR = 1e-9


def _code(name):
    text = open(os.path.join(CSRC, name)).read()
    text = re.sub(r"//[^\n]*", "", text)
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _const(name, header):
    m = re.findall(r"constexpr int %s = (\d+);" % name, _code(header))
    assert len(m) == 1, (name, header, m)
    return int(m[0])


def _between(code, start, end):
    """the single stretch of code from `start` to the next `end`"""
    assert code.count(start) == 1, (start, code.count(start))
    a = code.index(start)
    return code[a:code.index(end, a)]


def _chain(region):
    return [int(t) if t.isdigit() else t for t in re.findall(r"\bd <= (\w+)", region)]


# ---- 1. thresholds ----
def test_constants_are_what_the_table_records():
    got = {"KB_LDS_MAXD": _const("KB_LDS_MAXD", "gp_kernels.h"), "THETA_PACK": _const("THETA_PACK", "gp_kernels.h"),
           "SLOTP": _const("SLOTP", "gp_kernels.h"), "RTC_SPEC_MAXD": _const("RTC_SPEC_MAXD", "rtc_dyn.h"),
           "PC_GW": _const("PC_GW", "gp_paths.h"), "PO_GW": _const("PO_GW", "gp_paths_own.h")}
    for site, rec in dc.SITES.items():
        for name, value in rec["thresholds"].items():
            if name in got:
                assert got[name] == value, (site, name, got[name], value, HINT)
    assert {n for rec in dc.SITES.values() for n in rec["thresholds"]} >= set(got), HINT


def test_case_lists_of_the_build_and_gradient_switches():
    code = _code("gphip.hip")
    for macro, site in (("KB_CASE", "kbuild_direct"), ("KM_CASE", "kbuild_mfma"), ("GR_CASE", "grad_reduce")):
        got = [int(v) for v in re.findall(r"\b%s\((\d+)\)" % macro, code)]
        assert got == dc.SITES[site]["thresholds"][macro], (macro, got, HINT)
    assert len(re.findall(r"switch \(\(d \+ 3\) / 4\)", code)) == 1, HINT
    assert dc.SITES["kbuild_mfma"]["thresholds"]["KM_STEP"] == 4
    # the generic instantiations: LDS tiles up to KB_LDS_MAXD dimensions, global memory beyond; the matrix-pipe build up to it
    assert len(re.findall(r"d > KB_LDS_MAXD \? (?:0|64) :", code)) == 5, HINT
    assert len(re.findall(r"h->d <= KB_LDS_MAXD && h->dCentre\.p", code)) == 1, HINT
    assert len(re.findall(r"if \(a\.d > KB_LDS_MAXD\) \{", code)) == 1, HINT


def test_window_steps_and_the_staging_area():
    hip, xg, sp = _code("gphip.hip"), _code("gphip_xgrad.inc"), _code("gphip_sparse.inc")
    steps = {"gphip.hip": re.findall(r"a\.d0 < (?:a\.)?d; a\.d0 \+= (\d+)", hip), "gphip_xgrad.inc": re.findall(r"a\.d0 < d; a\.d0 \+= (\d+)", xg),
             "gphip_sparse.inc": re.findall(r"a\.d0 < d; a\.d0 \+= (\d+)", sp)}
    assert steps == {"gphip.hip": [str(dc.SITES["grad_reduce"]["thresholds"]["window"])],
                     "gphip_xgrad.inc": [str(dc.SITES["predict_xgrad_one_term"]["thresholds"]["window"])],
                     "gphip_sparse.inc": [str(dc.SITES["sparse_zgrad_one_term"]["thresholds"]["window"])]}, (steps, HINT)
    assert dc.SITES["general_two_term"]["thresholds"]["window"] == dc.SITES["grad_reduce"]["thresholds"]["window"]
    assert re.findall(r"4 \* np \* 8 > (\d+)", hip) == [str(dc.SITES["grad_rows"]["thresholds"]["staging_bytes"])], HINT
    assert len(re.findall(r"\(size_t\)nb \* \(h->d \+ SLOTP\) <= \(size_t\)THETA_PACK", hip)) == 1, HINT
    # np = 2 d + 6 accumulators for SE-ARD: d length scales ... the edge of the table follows from the staging area
    t = dc.SITES["grad_rows"]["thresholds"]["staging_bytes"]
    assert dc.SITES["grad_rows"]["edges"] == [(t // 32 - 6) // 2]
    pack, slotp = dc.SITES["theta_packed"]["thresholds"]["THETA_PACK"], dc.SITES["theta_packed"]["thresholds"]["SLOTP"]
    sides = [B * (d + slotp) <= pack for B, d in dc.SITES["theta_packed"]["Bd"]]
    assert sides == [True, False, True, False], HINT
    for (B, d), (B2, d2) in zip(dc.SITES["theta_packed"]["Bd"][::2], dc.SITES["theta_packed"]["Bd"][1::2]):
        assert B == B2 and d2 == d + 1 and B * (d + slotp) == pack, HINT      # exactly at the edge and one past it


def test_chains_of_the_four_dispatch_macros():
    xg = _chain(_between(_code("gphip_xgrad.inc"), "#define XG_LAUNCH", "#undef XG_LAUNCH"))
    zgr = _chain(_between(_code("gphip_sparse.inc"), "#define ZG_LAUNCH", "#undef ZG_LAUNCH"))
    paths = _code("gphip_paths.inc")
    pc = _chain(_between(paths, "#define PATHS_DW", "#undef PATHS_DW"))
    po = _chain(_between(paths, "#define PATHS_OWN_DW", "#undef PATHS_OWN_DW"))
    for site in ("predict_xgrad_one_term", "predict_xgrad_two_terms"):
        assert xg == dc.SITES[site]["thresholds"]["chain"], (site, xg, HINT)
    for site in ("sparse_zgrad_one_term", "sparse_zgrad_two_terms"):
        assert zgr == dc.SITES[site]["thresholds"]["chain"], (site, zgr, HINT)
    assert pc == dc.SITES["paths"]["thresholds"]["chain"], (pc, HINT)
    assert po == dc.SITES["paths_own"]["thresholds"]["chain"], (po, HINT)
    assert len(re.findall(r"const bool glb = d > KB_LDS_MAXD;", paths)) == 1, HINT      # paths_own: `else if (!glb)` ends its chain
    # the 32-wide instantiation serves one term only; two terms beyond 16 dimensions take the windows
    assert len(re.findall(r"d <= KB_LDS_MAXD && nterm == 1", _code("gphip_xgrad.inc"))) == 1, HINT
    assert len(re.findall(r"d <= KB_LDS_MAXD && nterm == 1", _code("gphip_sparse.inc"))) == 1, HINT
    # the run-time compiled program: specialised for 1 <= d <= RTC_SPEC_MAXD
    assert len(re.findall(r"spec_d >= 1 && spec_d <= RTC_SPEC_MAXD", _code("rtc_dyn.h"))) == 1, HINT


# ---- 2. coverage ----
@pytest.mark.parametrize("site", list(dc.SITES))
def test_both_sides_of_every_edge_are_run(site):
    rec = dc.SITES[site]
    resolve = lambda t: rec["thresholds"][t] if isinstance(t, str) else t      # noqa: E731
    edges = set(rec["edges"])
    for name, value in rec["thresholds"].items():                 # every recorded threshold is an edge, unless the site says why not
        if name == "chain":
            assert {resolve(t) for t in value} <= edges, (site, name, HINT)
        elif name in ("KB_CASE", "GR_CASE"):                      # a specialised D: its own instantiation, both neighbours differ
            assert {t for c in value for t in (c - 1, c) if t >= 1} <= edges, (site, name, HINT)
        elif name == "KM_CASE":
            assert {4 * ks for ks in value} <= edges, (site, HINT)
        elif name in ("KB_LDS_MAXD", "RTC_SPEC_MAXD") and site not in ("kbuild_mfma", "general_one_term"):
            assert value in edges, (site, name, HINT)
    for kernel, ds in rec["d"].items():
        assert ds == sorted(set(ds)), (site, kernel)
        for t in edges:
            assert t in ds and t + 1 in ds, (site, kernel, t, HINT)
    if "window" in rec["thresholds"] and site not in ("grad_reduce",):
        w = rec["thresholds"]["window"]
        start = 16 if site.endswith("two_terms") else 32           # the windowed route begins beyond this many dimensions
        for kernel, ds in rec["d"].items():
            beyond = [d for d in ds if d > start]
            assert any(d % w == 0 for d in beyond) and any(d % w == 1 for d in beyond), (site, kernel, HINT)
    if site == "kbuild_mfma":                                     # its upper end: 32 runs here, 33 stays on the direct build
        assert all(rec["thresholds"]["KB_LDS_MAXD"] == ds[-1] for ds in rec["d"].values())
        assert rec["thresholds"]["KB_LDS_MAXD"] + 1 in dc.SITES["kbuild_direct"]["d"]["se_ard"]


# ---- 3. conditions on the inputs ----
def _n_of(site):
    if site.startswith(("predict_xgrad", "sparse_zgrad")):
        return dc.N_XGRAD
    return dc.PATHS_SHAPE["n"] if site.startswith("paths") else dc.N_BUILD


INPUTS = sorted({(k if k != "se_ard_source_text" else "se_ard", d, _n_of(site), dc.PATHS_MEAN if site.startswith("paths") else dc.MEAN[k])
                 for site in dc.SITES for (_, k, d) in dc.cases(site)})


@pytest.mark.parametrize("kernel,d,n,mean", INPUTS, ids=["%s-d%d-n%d" % c[:3] for c in INPUTS])
def test_inputs_are_neither_diagonal_nor_singular(kernel, d, n, mean):
    from bayesianinference_amd import synthetic as syn
    X, _ = syn.make_dataset(n, d)
    th = dc.theta(kernel, d, mean)
    K = orc.covariance_matrix(kernel, th, X, mean)
    Kf = K - dc.SN ** 2 * np.eye(n)                               # the noise-free part
    sd = np.sqrt(np.diag(Kf))
    corr = (Kf / np.outer(sd, sd))[~np.eye(n, dtype=bool)]
    med, cond = float(np.median(corr)), float(np.linalg.cond(K))
    print(f"{kernel} d={d} N={n}: median off-diagonal correlation {med:.3f}, cond(K) {cond:.3e}")
    assert 0.1 <= med <= 0.9 and cond <= 1e5


def test_theta_layout_and_rows():
    th = dc.theta(dc.TWO_TERM, 3, "const")
    terms, op, c, sn, mu = orc.split_general(dc.TWO_TERM, 3, th, "const")
    assert op == "*" and (c, sn, mu) == (dc.OFFSET, dc.SN, dc.MU) and terms[0][3] == dc.SF and terms[1][3] == dc.SF2_TERM
    np.testing.assert_allclose(terms[1][1], dc.ELL2_SCALE * terms[0][1], rtol=1e-15)
    assert len(set(np.round(np.concatenate([terms[0][1], terms[1][1]]), 12))) == 6        # distinct length scales
    assert dc.theta("se_ard", 1)[0] == 0.3 and dc.theta("rq_ard", 9)[9] == dc.ALPHA
    rows = dc.theta_rows(dc.TWO_TERM, 3, 3, "const")
    assert np.array_equal(rows[0], th) and np.allclose(rows[2, :3], 1.14 * th[:3]) and np.allclose(rows[2, 4:7], 1.14 * th[4:7])
    assert np.array_equal(rows[2, [3, 7, 8, 9, 10]], th[[3, 7, 8, 9, 10]])


# ---- 4. the references against their own second route ----
def _err(g, want):
    return float(np.abs(g - want).max() / np.abs(want).max())


THETA_GRAD = dc.cases("grad_reduce") + dc.cases("grad_rows") + dc.cases("rtc")


@pytest.mark.parametrize("case", THETA_GRAD, ids=[dc.case_id(c) for c in THETA_GRAD])
def test_theta_gradient_routes_agree(case):
    _, kernel, d = case
    name = "se_ard" if kernel == "se_ard_source_text" else kernel
    c = dc.build_data(kernel, d)
    want = orc.log_likelihood_grad(name, c["theta"], c["X"], c["y"], c["mean_kind"])
    ll, got = lgr.loglik_and_grad(name, c["theta"], c["X"], c["y"], c["mean_kind"])
    lo = orc.log_likelihood(name, c["theta"], c["X"], c["y"], c["mean_kind"])
    print(f"{name} d={d}: analytic oracle against autograd {_err(got, want):.3e} of max |gradient| {np.abs(want).max():.4g}")
    assert abs(ll - lo) <= 1e-12 * max(abs(lo), dc.N_BUILD)       # the torch restatement is the same likelihood
    assert _err(got, want) <= THETA_GRAD_ROUTE_BAR


GENERAL = dc.cases("general_two_term") + dc.cases("general_one_term")


@pytest.mark.parametrize("case", [GENERAL[0], GENERAL[1], GENERAL[-2]], ids=[dc.case_id(c) for c in (GENERAL[0], GENERAL[1], GENERAL[-2])])
def test_autograd_theta_gradient_of_composed_forms_against_difference_quotients(case):
    """a sanity check of the one route the composed forms have: the oracle's 4th-order difference quotient, at its own accuracy
    (2e-6, the bar tests/test_gpu_kernels.py holds the device to against it)"""
    _, kernel, d = case
    c = dc.build_data(kernel, d)
    want = orc.log_likelihood_grad(kernel, c["theta"], c["X"], c["y"], c["mean_kind"])
    ll, got = lgr.loglik_and_grad(kernel, c["theta"], c["X"], c["y"], c["mean_kind"])
    lo = orc.log_likelihood(kernel, c["theta"], c["X"], c["y"], c["mean_kind"])
    print(f"{kernel} d={d}: autograd against difference quotients {_err(got, want):.3e}")
    assert abs(ll - lo) <= 1e-12 * max(abs(lo), dc.N_BUILD)
    np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6 * np.abs(want).max())


@pytest.mark.parametrize("case", GENERAL, ids=[dc.case_id(c) for c in GENERAL])
def test_torch_restatement_of_composed_forms_is_the_oracles_likelihood(case):
    _, kernel, d = case
    c = dc.build_data(kernel, d)
    ll, got = lgr.loglik_and_grad(kernel, c["theta"], c["X"], c["y"], c["mean_kind"])
    lo = orc.log_likelihood(kernel, c["theta"], c["X"], c["y"], c["mean_kind"])
    assert abs(ll - lo) <= 1e-12 * max(abs(lo), dc.N_BUILD) and np.all(np.isfinite(got)) and len(got) == len(c["theta"])


XGRAD = dc.cases("predict_xgrad_one_term") + dc.cases("predict_xgrad_two_terms")


@pytest.mark.parametrize("case", XGRAD, ids=[dc.case_id(c) for c in XGRAD])
def test_predict_grad_routes_agree(case):
    _, kernel, d = case
    c = dc.xgrad_reference(kernel, d)
    ag = pg.exact_autograd(kernel, c["theta"], c["X"], c["y"], c["Xs"], c["mean_kind"])
    em, ev = _err(ag["dmean"], c["dmean"]), _err(ag["dvar"], c["dvar"])
    print(f"{kernel} d={d}: numpy against autograd, dmean {em:.3e} dvar {ev:.3e}")
    assert c["dmean"].shape == (dc.M_XGRAD, d) and np.all(np.isfinite(c["dmean"])) and np.all(np.isfinite(c["dvar"]))
    assert em <= XGRAD_ROUTE_BAR and ev <= XGRAD_ROUTE_BAR


SPARSE = dc.cases("sparse_zgrad_one_term") + dc.cases("sparse_zgrad_two_terms")


@pytest.mark.parametrize("case", SPARSE, ids=[dc.case_id(c) for c in SPARSE])
def test_sparse_routes_agree(case):
    _, kernel, d = case
    c = dc.sparse_reference(kernel, d)
    ag = pg.sparse_autograd(kernel, c["theta"], c["X"], c["y"], c["Z"], c["jitter"], c["Xs"], c["mean_kind"])
    em, ev = _err(ag["dmean"], c["dmean"]), _err(ag["dvar"], c["dvar"])
    print(f"sparse {kernel} d={d}: predict_grad numpy against autograd, dmean {em:.3e} dvar {ev:.3e}; dF/dZ routes differ by "
          f"{c['route_difference']:.3e} of max |dF/dZ| {np.abs(c['gradZ']).max():.4g}")
    assert em <= XGRAD_ROUTE_BAR and ev <= XGRAD_ROUTE_BAR
    assert c["gradZ"].shape == (dc.M_INDUCING, d) and c["route_difference"] <= ZGRAD_ROUTE_BAR


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


PATHS = dc.cases("paths")


@pytest.mark.parametrize("case", PATHS, ids=[dc.case_id(c) for c in PATHS])
def test_paths_reference_is_linear_gaussian_in_the_draw(case, lib):
    """the pin of tests/test_paths.py at every d of the table: the reference's draws are its exact moments' linear form, 1e-12"""
    _, kernel, d = case
    c = dc.paths_data(kernel, d)
    S, F = dc.PATHS_SHAPE["S"], dc.PATHS_SHAPE["F"]
    om, ph, amp = _lib.rff_table(kernel, d, c["theta"], F, seed=2)
    table = {"omega": om, "phase": ph, "amp": amp}
    mo = pr.moments(kernel, c["theta"], c["X"], c["y"], c["Xs"], table, c["mean_kind"])
    rng = np.random.default_rng(9)
    w, eps = rng.standard_normal((S, len(ph))), dc.SN * rng.standard_normal((S, len(c["X"])))
    f = pr.paths(kernel, c["theta"], c["X"], c["y"], c["Xs"], table, w, eps, c["mean_kind"], grad=False)["out"]
    lin = mo["mean"][None, :] + w @ mo["A"].T + eps @ mo["B"].T
    assert np.max(np.abs(f - lin)) <= 1e-12 * max(1.0, np.max(np.abs(f)))
