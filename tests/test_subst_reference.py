"""tests/subst_reference.py pinned before it judges a kernel; no GPU.

1. The long-double inverse and two-triangle solve against a 40-digit mpmath solve at n = 24.
2. Every distinct matrix of the case table (tests/subst_cases.py) through LAPACK (solve_triangular twice) and through both host
   emulations of this project's algorithm (128-block explicit inverses; the 64-block inverses cut out of them): omega_solve2,
   phi_solve and the mean / variance checks inside their bars, and the CAP: the forward bars themselves stay under 1e-9 of what
   they bound (fp32: u32 / u64 times that), so they cannot go slack through an ill-conditioned row.
3. Every check bites, with the smallest planted defect it sees stated where it is asserted.
4. The launch counts of the table against values derived by hand."""
import numpy as np
import pytest
from scipy.linalg import solve_triangular

import factor_cases as fc
import factor_reference as fr
import subst_cases as sc
import subst_reference as sr
from oracle import gp_oracle as orc

pytestmark = pytest.mark.skipif(not fr.HAVE_LD, reason=fr.SKIP_REASON)

INPUTS = sc.distinct_inputs()
IDS = ["%s-d%d-%s-n%d-sn%g-f%d" % (c["kernel"], c["d"], c["mean"], c["n"], c["sn"], c["dtype"]) for c in INPUTS]
_cache = {}


def narrow(a, dtype):
    return a if dtype == 64 else a.astype(np.float32).astype(np.float64)


def host(case, theta=None):
    """everything the host can know of a row: K as the handle's arithmetic holds it, the emulated factor and its inverses, z, four
    right-hand sides, 65 test points with k* and kappa, and the prepared factor of the checks"""
    key = (case["kernel"], case["d"], case["mean"], case["n"], case["sn"], case["dtype"], None if theta is None else tuple(theta))
    if key not in _cache:
        dt = case["dtype"]
        X, y, th = sc.inputs(case)
        th = th if theta is None else np.asarray(theta)
        K = narrow(orc.covariance_matrix(case["kernel"], th, X, case["mean"]), dt)
        L, Ws = sr.emulate(K, dt)
        L, Ws = L.astype(np.float64), [w.astype(np.float64) for w in Ws]
        r = fc.residual(case, y, th)
        z = fr.solve_like_device(L, Ws, r, dt).astype(np.float64)
        B = sr.round_rhs(sc.rhs(dict(case, count=4), y, th), dt)
        Xs = sc.test_points(dict(case, count=65), X)
        ks, kappa = orc.k_and_kappa(case["kernel"], th, X, Xs, case["mean"])
        _cache[key] = dict(K=K, L=L, Ws=Ws, r=r, z=z, B=B, ks=narrow(ks, dt), kappa=kappa, mu=sc.mu_of(case, th), F=sr.Factor(L, dt), th=th, X=X, y=y)
    return _cache[key]


def all_checks(F, z, X, B, ks, kappa, mu, mean, var, dt):
    c = sr.solve_checks(F, None, X, B, dt)
    p = sr.predict_checks(F, None, z, ks, kappa, mu, mean, var, dt)
    c["mean"], c["var"] = p["mean"], p["var"]
    return c


def test_long_double_solve_and_inverse_match_mpmath():
    mp = pytest.importorskip("mpmath")
    n = 24
    X, y = fc.dataset(n, 3)
    K = orc.covariance_matrix("se_ard", fc.theta("se_ard", 3, 0.15), X)
    L = np.linalg.cholesky(K)
    B = np.random.default_rng(3).standard_normal((n, 2))
    F = sr.Factor(L, 64)
    _, x = sr.exact_solve(F, B)
    wide = lambda v: mp.mpf(float(np.float64(v))) + mp.mpf(float(v - np.longdouble(np.float64(v))))      # noqa: E731
    with mp.workdps(40):
        Lm = mp.matrix(L.tolist())
        Lim = mp.inverse(Lm)
        xm = Lim.T * (Lim * mp.matrix(B.tolist()))
        e_inv = max(abs(wide(F.Li[i, j]) - Lim[i, j]) for i in range(n) for j in range(n)) / max(abs(Lim[i, i]) for i in range(n))
        e_x = max(abs(wide(x[i, c]) - xm[i, c]) for i in range(n) for c in range(2)) / max(abs(xm[i, c]) for i in range(n) for c in range(2))
    # forward error of a substitution in long double: n eps cond(L) relative to the norm (Higham 8.7 to first order); the two
    # triangles one after the other: cond(L)^2 = cond(K), twice
    bar = 2 * n * fr.EPS_LD * float(np.linalg.cond(K))
    print("n = 24 against mpmath (40 digits): Li %.2e, x* %.2e of the largest entry, bar %.2e" % (float(e_inv), float(e_x), bar))
    assert float(e_inv) <= bar and float(e_x) <= bar <= 1e-14
    assert np.all(np.triu(F.Li, 1) == 0)


def lapack_route(h, dt):
    T = np.float64 if dt == 64 else np.float32
    L = np.linalg.cholesky(h["K"].astype(T)).astype(T)
    z = solve_triangular(L, h["r"].astype(T), lower=True).astype(T)
    yv = solve_triangular(L, h["B"].astype(T), lower=True).astype(T)
    x = solve_triangular(L, yv, lower=True, trans="T").astype(T)
    v = solve_triangular(L, h["ks"].astype(T), lower=True).astype(T).astype(np.float64)
    z = z.astype(np.float64)
    return L.astype(np.float64), z, x.astype(np.float64), h["mu"] + z @ v, h["kappa"] - np.sum(v * v, axis=0)


def emulation_route(h, dt, tb):
    Ws = h["Ws"] if tb == sr.TB else sr.cut_w64(h["Ws"])
    _, x = sr.substitute_like_device(h["L"], Ws, h["B"], dt, tb=tb)
    mean, var = sr.predict_like_device(h["L"], Ws, h["z"], h["ks"], h["kappa"], h["mu"], dt, tb=tb)
    return h["L"], h["z"], x, mean, var


@pytest.mark.parametrize("case", INPUTS, ids=IDS)
def test_lapack_and_both_emulations_are_inside_every_bar_and_the_bars_are_capped(case):
    h, dt = host(case), case["dtype"]
    for name, route in (("LAPACK", lambda: lapack_route(h, dt)), ("emulation-128", lambda: emulation_route(h, dt, 128)),
                        ("emulation-64", lambda: emulation_route(h, dt, 64))):
        L, z, x, mean, var = route()
        F = h["F"] if L is h["L"] else sr.Factor(L, dt)
        checks = all_checks(F, z, x, h["B"], h["ks"], h["kappa"], h["mu"], mean, var, dt)
        print(sr.report("%s %s" % (IDS[INPUTS.index(case)], name), checks))
        assert sr.failed(checks) == [], (name, checks)
    s_var, s_mean = sr.slack(h["F"], None, h["z"], h["ks"], h["kappa"], h["mu"], dt)
    print("  rho %.2e; cap: var bar / kappa %.2e, mean bar / max(|m*|, |z|_inf) %.2e (cap %.1e)" % (h["F"].rho, s_var, s_mean, sr.slack_cap(dt)))
    assert s_var <= sr.slack_cap(dt) and s_mean <= sr.slack_cap(dt)


BITE = [c for c in INPUTS if (c["kernel"], c["n"]) in (("se_ard", 385), ("se_ard", 641), ("matern52_ard", 385))]


@pytest.mark.parametrize("case", BITE, ids=[IDS[INPUTS.index(c)] for c in BITE])
def test_every_check_bites(case):
    h, dt, n = host(case), case["dtype"], case["n"]
    F, L, Ws, z, B, ks, kappa, mu = (h[k] for k in ("F", "L", "Ws", "z", "B", "ks", "kappa", "mu"))
    T = np.float64 if dt == 64 else np.float32
    eps = 1e-11 if dt == 64 else 1e-3
    _, x = sr.substitute_like_device(L, Ws, B, dt)
    mean, var = sr.predict_like_device(L, Ws, z, ks, kappa, mu, dt)
    run = lambda x_=x, mean_=mean, var_=var: sr.failed(all_checks(F, z, x_, B, ks, kappa, mu, mean_, var_, dt))      # noqa: E731
    assert run() == []

    # (1) one entry of x-hat off by a relative 1e-11 (fp32 1e-3): the entry whose own term weighs most in its row's normaliser.
    # omega_solve2 sees it.  phi_solve sees it by right only where eps |x_k| exceeds e_x[k], the forward bound of a stable
    # substitution, which carries cond: there the defect size is taken from the bar (twice it), and stated.
    den = F.absL @ (F.absL.T @ np.abs(x))
    Kd = np.sum(F.absL ** 2, axis=1)                              # (L L^T)_kk
    share = Kd[:, None] * np.abs(x) / den
    k, c = np.unravel_index(np.argmax(share), share.shape)
    assert eps * share[k, c] > 2 * sr.bar_solve2(n, dt)           # (else the defect is below what ANY backward-error test can see)
    x1 = x.copy()
    x1[k, c] = T(x1[k, c] * (1 + eps))
    assert "omega2" in run(x1)
    yx, xx = sr.exact_solve(F, B)
    e_y = F.g * (F.M @ np.abs(yx).astype(np.float64)) / (1.0 - F.rho)
    e_x = (F.g * (F.absLi.T @ (F.absL.T @ np.abs(xx).astype(np.float64))) + F.absLi.T @ e_y) / (1.0 - F.rho)
    eps_phi = float(2.0 * e_x[k, c] / abs(x[k, c]))
    print("%s: entry (%d, %d): omega_solve2 sees a relative %.0e; phi_solve's bar there is a relative %.2e of the entry" % (case["id"], k, c, eps, eps_phi / 2))
    x1p = x.copy()
    x1p[k, c] = x1p[k, c] * (1 + max(eps_phi, 4 * sr.U[dt]))
    assert "phi" in run(x1p)
    if eps > eps_phi:
        assert "phi" in run(x1)
    else:                                                         # 1e-11 is inside the forward bar by right: omega_solve2 fails ALONE
        assert run(x1) == ["omega2"]

    # (2) one off-diagonal 128-tile contribution L(b, c) left out of the backward pass
    nt = sc.nt_of(n)
    for skip in ((nt - 1, 0), (2, 1)):
        _, x2 = sr.substitute_like_device(L, Ws, B, dt, skip=skip)
        assert run(x2) == ["omega2", "phi"], skip

    # (3) the W of a neighbouring block used for one block
    _, x3 = sr.substitute_like_device(L, Ws, B, dt, w_of={1: 2})
    assert run(x3) == ["omega2", "phi"]

    # (4) the stale-copy model: x-hat computed, correctly, from the factor of a DIFFERENT theta (sn and the length scales changed
    # as the device test changes them), judged against this one's; and the smallest such change of sn that is seen
    th2 = sc.stale_theta(case, h["th"])
    h2 = host(case, th2)
    _, x4 = sr.substitute_like_device(h2["L"], h2["Ws"], B, dt)
    mean4, var4 = sr.predict_like_device(h2["L"], h2["Ws"], h2["z"], h2["ks"], h2["kappa"], h2["mu"], dt)
    assert run(x4, mean4, var4) == ["mean", "omega2", "phi", "var"]
    th3 = h["th"].copy()
    i_sn = len(th3) - (2 if case["mean"] == "const" else 1)
    th3[i_sn] *= 1 + (1e-7 if dt == 64 else 1e-1)                 # sn off by 1e-7: K's diagonal by 2e-7 sn^2 = 4.5e-9
    h3 = host(case, th3)
    _, x5 = sr.substitute_like_device(h3["L"], h3["Ws"], B, dt)
    assert "omega2" in run(x5)

    # (5) one predicted variance with one 64-row strip of v left out of ||v||^2; (6) the nugget added twice; a variance off by
    # twice its own bar (the smallest defect the check can see, as a relative size of the variance it is stated)
    # (a strip whose share of ||v||^2 is under the variance bar is inside it by right -- the late strips of an fp32 row -- so the
    #  verdict is asked of every strip that is clearly on one side: over twice the bar, or under half of it)
    _, _, _, var_bar7 = sr.predict_bars(F, None, z, ks[:, 7], kappa[7:8], mu, dt)
    v7 = fr.solve_like_device(L, Ws, ks[:, 7], dt).astype(np.float64)
    seen = 0
    for strip in range((n + 63) // 64):
        share7 = float(np.sum(v7[64 * strip:64 * strip + 64] ** 2))
        _, var5 = sr.predict_like_device(L, Ws, z, ks, kappa, mu, dt, drop_strip=(7, strip))
        if share7 > 2 * var_bar7[0]:
            assert run(var_=var5) == ["var"], strip
            seen += 1
        elif share7 < 0.5 * var_bar7[0]:
            assert run(var_=var5) == [], strip
    assert seen >= (3 if dt == 64 else 1) and float(np.sum(v7[:64] ** 2)) > 2 * var_bar7[0]
    _, var6 = sr.predict_like_device(L, Ws, z, ks, kappa, mu, dt, nugget_twice=case["sn"] ** 2)
    assert run(var_=var6) == ["var"]
    _, _, var_star, var_bar = sr.predict_bars(F, None, z, ks, kappa, mu, dt)
    t = int(np.argmax(var_bar / np.abs(var_star).astype(np.float64)))
    print("%s: the variance check sees a relative %.2e at its least favourable point" % (case["id"], 2 * var_bar[t] / float(var_star[t])))
    var7 = var.copy()
    var7[t] += 2.0 * var_bar[t] + 4 * sr.U64 * abs(var7[t])
    assert run(var_=var7) == ["var"]

    # (7) a mean with mu omitted (rows with a constant mean); a mean off by twice its own bar
    if case["mean"] == "const":
        mean7, _ = sr.predict_like_device(L, Ws, z, ks, kappa, mu, dt, no_mu=True)
        assert run(mean_=mean7) == ["mean"]
    m_star, mean_bar, _, _ = sr.predict_bars(F, None, z, ks, kappa, mu, dt)
    mean8 = mean.copy()
    mean8[3] += 2.0 * mean_bar[3] + 4 * sr.U64 * abs(mean8[3])
    assert run(mean_=mean8) == ["mean"]


def test_launch_table_against_hand_derived_counts():
    by = {c["id"]: c for c in sc.ALL}
    # Nt = 6, four vectors: two single-vector launches, zero flops
    assert by["solve-n700-f64-default-r4"]["launches"] == (2, 0, 0) and by["solve-n700-f64-default-r4"]["trsm_flops"] == 0.0
    # five vectors, default: both halves ONE dataflow launch each, 2 x 128 x 768^2 flops
    assert by["solve-n641-f64-default-r5"]["launches"] == (2, 0, 0) and by["solve-n641-f64-default-r5"]["trsm_flops"] == 2 * 128 * 768.0 ** 2
    # multi-kernel, Nt = 6: 6 diagonal products; 5 forward updates + 6 backward diagonal products + 5 backward updates
    assert by["solve-n641-f64-nopdf-panel2-r129"]["launches"] == (6, 16, 0) and by["solve-n641-f64-nopdf-panel2-r129"]["trsm_flops"] is None
    assert by["solve-n700-f32-default-r5"]["route"] == ("mk",) and by["solve-n129-f32-default-r129"]["launches"] == (2, 4, 0)
    # 1030 vectors pad to 1152 > Npad = 768 rows: no dataflow launch even at default options
    assert by["solve-n641-f64-nopdf-r1030"]["route"] == ("mk",) and sc.wide_panel(by["solve-n641-f64-nopdf-r1030"])
    # the 2048 seam at N = 257 (Nt = 3, Npad = 384): 2048 rows > Npad -> mk (3, 2 + 5); 130 -> 256 rows <= 384 -> two dataflow launches
    assert by["solve-n257-f64-seam2048-r2178"]["route"] == ("mk", "df") and by["solve-n257-f64-seam2048-r2178"]["launches"] == (5, 7, 0)
    assert [r["route"] for r in sc.SOLVE_SWITCH[0]] == [("df",), ("mk",)]
    assert by["predict-n700-f64-default-m700"]["launches"] == (1, 0, 1) and by["predict-n700-f64-default-m700"]["trsm_flops"] == 768.0 ** 3
    assert by["predict-n129-f64-default-m300"]["launches"] == (2, 1, 1)
    assert by["predict-n641-f64-mkfit-panel4-m129"]["launches"] == (6, 5, 1)
    # the chunk seam at N = 129 (Nt = 2): 32768 points multi-kernel (2, 1), 130 points one dataflow launch; two epilogues
    assert sc.PREDICT_SEAM["route"] == ("mk", "df") and sc.PREDICT_SEAM["launches"] == (3, 1, 2)
    assert [sc.staging(r) for r in (5, 96, 97, 128, 129, 700)] == ["compact", "compact", "transposed", "transposed", "compact", "transposed"]
    assert sc.SOLVE_NONFINITE["route"] == ("df",) and sc.SOLVE_NONFINITE["launches"] == (2, 0, 0)
    for tag, (other, _) in sc.SAME_LAUNCHES_AS.items():
        rows_a = [c for c in sc.ALL if c["tag"] == tag]
        rows_b = {(c["call"], c["n"], c["count"]): c for c in sc.ALL if c["tag"] == other and c["dtype"] == 64}
        for a in rows_a:
            b = rows_b.get((a["call"], a["n"], a["count"]))
            if b is not None and (tag != "mkfit" or a["count"] <= 4):
                assert a["launches"] == b["launches"], (a["id"], b["id"])
