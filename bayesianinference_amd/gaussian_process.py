"""Host-side mirror of the reference's GP interface for the MI355X path.

The reference is Wolfram Language (no Wolfram kernel exists here or on the GPU box), so the host
side above the C ABI is Python, keeping the reference's names, argument meaning, association
keys and failure behaviour:

  inferenceObject                       BayesianUtilities.wl:107-138
  dataNormalForm                        BayesianUtilities.wl:203-221
  defineGaussianProcess                 BayesianGaussianProcess.wl:228-330  (BGP)
  defineInferenceProblem (GP subset)    BayesianStatistics.wl:164-308       (BS)
  predictFromGaussianProcess            BayesianGaussianProcess.wl:332-394

Differences forced by the closed kernel set (SURVEY.md §7 "Arbitrary WL kernels vs named
kernels"): `kernel` is a named spec ("SE", "SEARD", "Matern52", "Matern52ARD" or None for the
null kernel BGP:25).  The nugget and the mean function may be ANY functions of the point, as in
the reference (`nugget[points[[i]]]` BGP:37, `meanFunction /@ inputData` BGP:300): pass a callable
f(X[N, d], theta[p]) -> values[N] (vectorised over the points; the hyper-parameters it uses are
entries of theta) and the host evaluates it per theta and hands the values to the library
(gphip_*_pw); "Constant" / None keep the forms sigma_n^2 and mu / 0 read from theta.
`variables` must list the hyper-parameters in the C-ABI order (l.., sigma_f, sigma_n[, mu]).
All arithmetic runs in the HIP library; nothing here falls back to the CPU.
"""
from __future__ import annotations

import math
from collections.abc import Mapping

import numpy as np

from . import _lib

# BU:47 -- closed-source constant in the reference; the WL shim reads the real one at load time.
MACHINE_LOG_ZERO = -1.7976931348623157e308

_KERNEL_ALIASES = {
    "se": "se", "squaredexponential": "se", "se_iso": "se",
    "seard": "se_ard", "se_ard": "se_ard",
    "matern52": "matern52", "matern5/2": "matern52",
    "matern52ard": "matern52_ard", "matern52_ard": "matern52_ard",
    "null": "null", "none": "null",
    "matern32": "matern32", "matern3/2": "matern32", "matern32ard": "matern32_ard", "matern32_ard": "matern32_ard",
    "rq": "rq", "rationalquadratic": "rq", "rqard": "rq_ard", "rq_ard": "rq_ard",
}

# The WL expressions that define each named kernel for the *reference* defineGaussianProcess, so
# that "same inputs" is well defined.
WL_KERNEL_EXPRESSIONS = {
    "se": "Function[{p, q}, sf^2 Exp[-Total[(p - q)^2]/(2 l^2)]]",
    "se_ard": "Function[{p, q}, sf^2 Exp[-1/2 Total[((p - q)/{l1, ..., ld})^2]]]",
    "matern52": "Function[{p, q}, With[{s = Sqrt[Total[(p - q)^2]]/l}, sf^2 (1 + Sqrt[5] s + 5 s^2/3) Exp[-Sqrt[5] s]]]",
    "matern52_ard": "Function[{p, q}, With[{s = Sqrt[Total[((p - q)/{l1, ..., ld})^2]]}, sf^2 (1 + Sqrt[5] s + 5 s^2/3) Exp[-Sqrt[5] s]]]",
    "null": "Function[0]",
    "matern32": "Function[{p, q}, With[{s = Sqrt[Total[(p - q)^2]]/l}, sf^2 (1 + Sqrt[3] s) Exp[-Sqrt[3] s]]]",
    "matern32_ard": "Function[{p, q}, With[{s = Sqrt[Total[((p - q)/{l1, ..., ld})^2]]}, sf^2 (1 + Sqrt[3] s) Exp[-Sqrt[3] s]]]",
    "rq": "Function[{p, q}, sf^2 (1 + Total[(p - q)^2]/(2 alpha l^2))^-alpha]",
    "rq_ard": "Function[{p, q}, sf^2 (1 + Total[((p - q)/{l1, ..., ld})^2]/(2 alpha))^-alpha]",
}


def wl_kernel_expression(kname: str) -> str:
    """WL text of a named or composed kernel ('term [(+|*) term] [+const]'): what a user hands to the REFERENCE's
    defineGaussianProcess so that "same inputs" is defined (each term with its own l / alpha / sf symbols)."""
    if kname in WL_KERNEL_EXPRESSIONS:
        return WL_KERNEL_EXPRESSIONS[kname]
    key, offset = (kname[:-len("+const")], True) if kname.endswith("+const") else (kname, False)
    for op in ("+", "*"):
        if op in key:
            a, b = key.split(op, 1)
            body = f"({WL_KERNEL_EXPRESSIONS[a]})[p, q] {op} ({WL_KERNEL_EXPRESSIONS[b]})[p, q]"
            break
    else:
        body = f"({WL_KERNEL_EXPRESSIONS[key]})[p, q]"
    return "Function[{p, q}, " + ("c + " if offset else "") + body + "]"
WL_NUGGET_EXPRESSION = "Function[sn^2]"


class inferenceObject(Mapping):
    """Association wrapper (BU:107-138): obj[key], obj["Properties"], Normal -> .normal(),
    Append -> .append(), inferenceObject[$Failed] -> inferenceObject(None) with .failed."""

    def __init__(self, assoc):
        if isinstance(assoc, inferenceObject):          # BU:128 idempotent wrapping
            assoc = assoc._assoc
        self._assoc = None if assoc is None else dict(assoc)

    @property
    def failed(self) -> bool:                           # BU:126 FailureQ
        return self._assoc is None

    def normal(self) -> dict:                           # BU:121 Normal
        return dict(self._assoc or {})

    def append(self, extra: Mapping) -> "inferenceObject":   # BU:122-125 Append
        out = self.normal()
        out.update(extra)
        return inferenceObject(out)

    def __getitem__(self, key):
        if self._assoc is None:
            raise KeyError("inferenceObject[$Failed]")
        if key == "Properties":                         # BU:130
            return sorted(list(self._assoc) + ["Properties"])
        if isinstance(key, tuple):                      # obj["GaussianProcessData", "ModelFunctions"]
            cur = self._assoc
            for k in key:
                cur = cur[k]
            return cur
        return self._assoc[key]

    def __iter__(self):
        return iter(self._assoc or {})

    def __len__(self):
        return len(self._assoc or {})

    def __repr__(self):
        if self.failed:
            return "inferenceObject[$Failed]"
        return f"inferenceObject[<{len(self._assoc)} defined properties: {', '.join(list(self._assoc)[:4])}...>]"


def dataNormalForm(data):
    """BU:203-221: vector -> N x 1 matrix; (in, out) / {"Input","Output"} / [(x, y), ...] ->
    (X[N,d], Y[N,k]); None on malformed input ($Failed)."""
    try:
        if isinstance(data, Mapping) and "Input" in data:
            data = (data["Input"], data["Output"])
        if isinstance(data, tuple) and len(data) == 2:
            xin, xout = dataNormalForm(data[0]), dataNormalForm(data[1])
            if xin is None or xout is None or len(xin) != len(xout):
                return None
            return xin, xout
        if isinstance(data, list) and data and isinstance(data[0], tuple) and len(data[0]) == 2:
            return dataNormalForm(([p[0] for p in data], [p[1] for p in data]))   # {x -> y ..}
        arr = np.asarray(data, dtype=np.float64)
        if arr.ndim == 1:
            return arr[:, None]
        if arr.ndim == 2:
            return arr
    except (TypeError, ValueError):
        pass
    return None


def normalizeData(data_in, data_out=None):
    """BU:232-265: per-column standardisation (FeatureExtraction[.., "StandardizedVector"]: subtract the
    mean, divide by the sample standard deviation).  normalizeData(X) -> {"NormalizedData", "Function",
    "InverseFunction"}; normalizeData(X, Y) -> {"Input": {..}, "Output": {..}} (BU:239-242)."""
    if data_out is not None:
        return {"Input": normalizeData(data_in), "Output": normalizeData(data_out)}
    arr = dataNormalForm(data_in)
    if arr is None or isinstance(arr, tuple):
        return None
    mean = arr.mean(axis=0)
    sd = arr.std(axis=0, ddof=1) if len(arr) > 1 else np.ones(arr.shape[1])
    sd = np.where(sd > 0, sd, 1.0)

    def forward(x):
        return (dataNormalForm(x) - mean) / sd

    def inverse(z):
        return dataNormalForm(z) * sd + mean

    return {"NormalizedData": forward(arr), "Function": forward, "InverseFunction": inverse,
            "Mean": mean, "StandardDeviation": sd}


def normalizedDataQ(data) -> bool:
    """BU:267-286."""
    def test(a):
        return isinstance(a, Mapping) and {"NormalizedData", "Function", "InverseFunction"} <= set(a)
    return test(data) or (isinstance(data, Mapping) and set(data) == {"Input", "Output"}
                          and all(test(v) for v in data.values()))


def takePosteriorFraction(obj, frac: float):
    """BU:288-316: keep the heaviest samples until their cumulative CrudePosteriorWeight exceeds `frac`
    (frac = 1: all samples, sorted by decreasing weight)."""
    samples = sorted(obj["Samples"], key=lambda smp: -smp["CrudeLogPosteriorWeight"])
    if frac < 1:
        kept, count = [], 0.0
        for smp in samples:
            if count > frac:
                break
            kept.append(smp)
            count += smp["CrudePosteriorWeight"]
        samples = kept
    return inferenceObject(obj).append({"Samples": samples})


def _resolve_kernel(kernel):
    if kernel is None:
        return "null"
    if isinstance(kernel, _lib.CustomKernel):                     # ANY covariance function, as source text (gphip_create_custom)
        return kernel
    key = str(kernel).lower().replace(" ", "").replace("-", "")
    if key in _KERNEL_ALIASES:
        return _KERNEL_ALIASES[key]
    # composed forms: term [(+|*) term] [+const]  (include/gphip.h GPHIP_KERNEL_COMPOSE)
    body, offset = (key[:-len("+const")], "+const") if key.endswith("+const") else (key, "")
    for op in ("+", "*"):
        if op in body:
            a, b = body.split(op, 1)
            if a in _KERNEL_ALIASES and b in _KERNEL_ALIASES and "null" not in (_KERNEL_ALIASES[a], _KERNEL_ALIASES[b]):
                return _KERNEL_ALIASES[a] + op + _KERNEL_ALIASES[b] + offset
            break
    else:
        if body in _KERNEL_ALIASES and _KERNEL_ALIASES[body] != "null" and offset:
            return _KERNEL_ALIASES[body] + offset
    raise ValueError(f"kernel {kernel!r} is not a named kernel {sorted(set(_KERNEL_ALIASES.values()))} or a composed form "
                     "'term [(+|*) term] [+const]'; hand any other covariance function over as a _lib.CustomKernel (the source "
                     "text of its body, compiled at run time into the device kernel build)")


def _log_prior_function(prior, params):
    """'LogPriorPDFFunction' (BS:256-274): callable theta -> log pdf.  Accepts a callable, a list
    of scipy.stats frozen distributions (ProductDistribution), or "Uniform"/None over the box."""
    lo = np.array([p[1] for p in params], dtype=np.float64)
    hi = np.array([p[2] for p in params], dtype=np.float64)
    if callable(prior):
        return prior
    if prior is None or (isinstance(prior, str) and prior.lower() == "uniform"):
        logvol = float(np.sum(np.log(hi - lo)))

        def uniform_logpdf(theta):
            theta = np.asarray(theta, dtype=np.float64)
            return -logvol if np.all((theta >= lo) & (theta <= hi)) else MACHINE_LOG_ZERO
        return uniform_logpdf
    dists = list(prior)
    if len(dists) != len(params):
        raise ValueError("prior list length differs from the number of parameters")

    def product_logpdf(theta):
        theta = np.asarray(theta, dtype=np.float64)
        if not np.all((theta >= lo) & (theta <= hi)):
            return MACHINE_LOG_ZERO
        val = float(sum(d.logpdf(t) for d, t in zip(dists, theta)))
        return val if math.isfinite(val) else MACHINE_LOG_ZERO
    return product_logpdf


def random_domain_points(params, count=100, width=100.0, rng=None):
    """BU:366-372 randomDomainPointDistribution: Cauchy(0, width) truncated to the parameter box."""
    rng = rng or np.random.default_rng(0)
    lo = np.array([p[1] for p in params], dtype=np.float64)
    hi = np.array([p[2] for p in params], dtype=np.float64)
    u = rng.random((count, len(params)))
    clo = np.arctan(np.maximum(lo, -1e300) / width)
    chi = np.arctan(np.minimum(hi, 1e300) / width)
    return width * np.tan(clo + u * (chi - clo))


def _pointwise(fn, P, thetas):
    """values of a point-dependent nugget / mean function for every theta: [B, len(P)] (None stays None)"""
    if fn is None:
        return None
    rows = []
    for th in np.atleast_2d(thetas):
        v = np.asarray(fn(P, th), dtype=np.float64)
        rows.append(np.broadcast_to(v, (len(P),)) if v.ndim == 0 else v.reshape(len(P)))
    return np.ascontiguousarray(np.array(rows))


def make_log_likelihood(handle: "_lib.Handle", nugget_fn=None, mean_fn=None, X=None):
    """The drop-in closure for "LogLikelihoodFunction" (seam at BGP:249,293-294): theta -> machine
    real, total over the parameter box, $MachineLogZero on numerical failure (BGP:298-304), never an
    exception for bad theta values (BS:276-298).  nugget_fn / mean_fn: point-dependent nugget[x] / meanFunction[x]
    (callables f(X, theta) -> values[N], BGP:37, 300), evaluated here on the host for every theta."""
    pw = nugget_fn is not None or mean_fn is not None

    def log_likelihood(theta):
        theta = np.asarray(theta, dtype=np.float64)
        if theta.ndim == 2 or pw:                         # Listable use: B x p -> B (BGP:59)
            if pw:
                out, info = handle.loglik_batch_pw(theta, _pointwise(mean_fn, X, theta), _pointwise(nugget_fn, X, theta))
            else:
                out, info = handle.loglik_batch(theta)
            res = np.where((info == 0) & np.isfinite(out), np.clip(out, MACHINE_LOG_ZERO, -MACHINE_LOG_ZERO), MACHINE_LOG_ZERO)
            return res if theta.ndim == 2 else float(res[0])
        ll, info = handle.loglik(theta)
        if info != 0 or not math.isfinite(ll):
            return MACHINE_LOG_ZERO
        return min(max(ll, MACHINE_LOG_ZERO), -MACHINE_LOG_ZERO)     # Clip, BGP:183,190-197
    return log_likelihood


def defineGaussianProcess(data, kernel, nugget="Constant", meanFunction=None, variables=(),
                          variablePrior="Uniform", **rules) -> inferenceObject:
    """BGP:228-330.  data: (X, Y) with Y N x 1 (BGP:220-226); variables: [(name, min, max), ...] in
    the order (l.., sigma_f, sigma_n[, mu]); variablePrior: callable / list of scipy frozen
    distributions / "Uniform"; extra rules are forwarded into the object (`rest___Rule`, BGP:233,323)
    -- e.g. Device=0.  A caller-supplied LogLikelihoodFunction=callable is installed verbatim
    (BGP:293-294).  Returns inferenceObject(None) where the reference returns inferenceObject[$Failed]."""
    if normalizedDataQ(data) and isinstance(data, Mapping) and "Input" in data:      # BGP:214-218
        rules.setdefault("DataPreProcessors", {k: {"Function": v["Function"], "InverseFunction": v["InverseFunction"]}
                                               for k, v in data.items()})
        data = (data["Input"]["NormalizedData"], data["Output"]["NormalizedData"])
    norm = dataNormalForm(data)
    if norm is None or not isinstance(norm, tuple):
        return inferenceObject(None)                              # BGP:204-207 dataFormat
    X, Y = norm
    if Y.shape[1] != 1:                                           # BGP:220-226 outputDim
        return inferenceObject(None)
    if len(X) != len(Y):                                          # BGP:251-253
        return inferenceObject(None)
    if isinstance(nugget, str) and nugget.lower() != "constant":
        raise ValueError('nugget must be "Constant" (Function[sn^2]) or a callable f(X, theta) -> variances[N]')
    nugget_fn = nugget if callable(nugget) else None
    mean_fn = meanFunction if callable(meanFunction) else None
    kname = _resolve_kernel(kernel)
    mean = "zero" if (mean_fn is not None or meanFunction in (None, 0, "Zero", "zero")) else "const"
    if mean == "const" and str(meanFunction).lower() not in ("constant", "const"):
        raise ValueError("meanFunction must be None/0, 'Constant' or a callable f(X, theta) -> means[N]")
    params = [tuple(v) for v in variables]
    if not params or any(len(v) != 3 for v in params):            # paramSpecPattern, BS:19
        return inferenceObject(None)
    # Device = one ordinal; Devices = a list of ordinals -> ONE multi-device handle (the library shards a large
    # factorisation over them and deals batches / posterior samples / test points to them, include/gphip.h);
    # Precision = "Double" (fp64, the parity path) | "Single" (fp32 device arithmetic, BASELINE.json cfg 5)
    device = rules.pop("Devices", rules.pop("Device", None))
    precision = str(rules.pop("Precision", "Double")).lower()
    if precision not in ("double", "single"):
        raise ValueError('Precision must be "Double" or "Single"')
    handle = _lib.Handle(X, Y[:, 0], kname, mean, dtype=64 if precision == "double" else 32,
                         device=device)                           # raises loudly without the library / GPU
    if handle.p != len(params):
        handle.close()
        raise ValueError(f"kernel {kname!r} with mean {mean!r} on d={X.shape[1]} needs {handle.p} "
                         f"hyper-parameters (l.., sigma_f, sigma_n[, mu]); got {len(params)}")
    # Switch[logLikelihood, Automatic, .., _Function | _CompiledFunction, .., _, ..]  (BGP:272-307):
    #   callable      installed verbatim (BGP:293-294)
    #   "Automatic"   LogLikelihood[MultinormalDistribution[m, K], {y}], unevaluated -> $MachineLogZero (BGP:273-292):
    #                 the multivariate-normal log-pdf IS -1/2 (N log 2pi + log det K + r.K^-1 r), and "stays
    #                 unevaluated" = K not positive definite = info != 0 -- so on this path both branches are the
    #                 same device computation; the branch taken is recorded under "LikelihoodBranch"
    #   anything else the default closure (BGP:296-305)
    user_ll = rules.pop("LogLikelihoodFunction", None)
    branch = "UserFunction" if callable(user_ll) else ("Automatic" if isinstance(user_ll, str) and
                                                       user_ll.lower() == "automatic" else "Default")
    pointwise = nugget_fn is not None or mean_fn is not None
    loglik = user_ll if callable(user_ll) else make_log_likelihood(handle, nugget_fn, mean_fn, X)

    def log_likelihood_gradient(theta):
        """(value, gradient) -- extension for gradient-based MAP / Laplace routes (LA:177-238 uses
        NMaximize without gradients); sentinel and NaN gradient on numerical failure.  Defined for the constant nugget /
        mean forms only (the library cannot differentiate a host function of the point)."""
        if pointwise:
            return loglik(theta), np.full(len(params), np.nan)
        if np.ndim(theta) == 2:
            # B x p -> (values[B], gradients[B, p]) from ONE device call (gphip_loglik_grad_batch); a failing row gets the
            # substitution of the one-theta form
            vals, grads, infos = handle.loglik_grad_batch(theta)
            bad = infos != 0
            vals[bad] = MACHINE_LOG_ZERO
            grads[bad] = np.nan
            return vals, grads
        ll, grad, info = handle.loglik_grad(theta)
        return (ll, grad) if info == 0 else (MACHINE_LOG_ZERO, np.full(len(params), np.nan))

    log_likelihood_gradient.batched = not pointwise               # a 2-D theta is accepted (laplace.approximateEvidence asks)

    def log_pseudo_likelihood(theta):
        """The leave-one-out log pseudo-likelihood L_LOO(theta) (R&W GPML 5.4.2; gphip_loo): the alternative to the marginal
        likelihood for choosing hyper-parameters.  Sentinel on numerical failure, like the likelihood closure."""
        if pointwise:
            return MACHINE_LOG_ZERO                               # (the library has no point-dependent form of it)
        res = handle.loo(theta, mean=False, var=False, logp=False)
        if res["info"] != 0 or not math.isfinite(res["total"]):
            return MACHINE_LOG_ZERO
        return min(max(res["total"], MACHINE_LOG_ZERO), -MACHINE_LOG_ZERO)

    def log_pseudo_likelihood_gradient(theta):
        """(L_LOO, gradient) from ONE factorisation (gphip_loo_grad); sentinel and NaN gradient on numerical failure."""
        if pointwise:
            return MACHINE_LOG_ZERO, np.full(len(params), np.nan)
        total, grad, info = handle.loo_grad(theta)
        return (total, grad) if info == 0 and math.isfinite(total) else (MACHINE_LOG_ZERO, np.full(len(params), np.nan))

    def covariance_function(theta):                               # "CovarianceFunction", BGP:264-271
        K = handle.covariance(theta)                              # Listable: B x p -> B matrices (BGP:59)
        if nugget_fn is not None:                                 # nugget[points[[i]]] on the diagonal instead of sn^2
            th2 = np.atleast_2d(np.asarray(theta, dtype=np.float64))
            nug = _pointwise(nugget_fn, X, th2)
            Kb = K.reshape((len(th2),) + K.shape[-2:]).copy()
            for b in range(len(th2)):
                sn = th2[b, handle.p - (2 if mean == "const" else 1)]      # theta = (l.., sf, sn[, mu])
                Kb[b][np.diag_indices(len(X))] += nug[b] - sn * sn
            K = Kb.reshape(K.shape)
        if isinstance(kname, str) and kname == "null":            # covarianceMatrix[.., nullKernel, ..] = nugget /@ points:
            return np.diagonal(K, axis1=-2, axis2=-1).copy()      # the DIAGONAL as a vector (BGP:27)
        return K

    def inverse_covariance_function(theta):                       # "InverseCovarianceFunction", BGP:308
        if pointwise:
            nug, mt = _pointwise(nugget_fn, X, theta), _pointwise(mean_fn, X, theta)
            info = handle.fit_pw(theta, mt, nug)
        else:
            info = handle.fit(theta)
        if info != 0:
            return MACHINE_LOG_ZERO                               # Throw[$MachineLogZero, "MatInv"]
        return {"Inverse": handle.solve, "LogDet": handle.logdet()}

    return defineInferenceProblem({
        "Data": (X, Y),
        "PriorDistribution": variablePrior,
        "Parameters": params,
        "KernelName": kname, "MeanName": mean, "LikelihoodBranch": branch,
        "GaussianProcessData": {
            "ModelFunctions": {
                "KernelFunction": ((kname.name, kname.body) if isinstance(kname, _lib.CustomKernel)
                                   else (kname, wl_kernel_expression(kname))),
                "NuggetFunction": nugget_fn if nugget_fn is not None else WL_NUGGET_EXPRESSION,
                "MeanFunction": mean_fn if mean_fn is not None else mean,
                "CovarianceFunction": covariance_function,
                "InverseCovarianceFunction": inverse_covariance_function,
            },
            "HIPHandle": handle,
        },
        **rules,
        "LogLikelihoodGradientFunction": log_likelihood_gradient,
        "LogPseudoLikelihoodFunction": log_pseudo_likelihood,
        "LogPseudoLikelihoodGradientFunction": log_pseudo_likelihood_gradient,
        "LogLikelihoodFunction": loglik,
    })


def defineInferenceProblem(assoc: Mapping) -> inferenceObject:
    """The subset of BS:164-308 a GP object goes through: parameter normal form, ParameterSymbols
    (BS:222), LogPriorPDFFunction (BS:256-274) and the 100-random-theta smoke test of both closures
    (BS:276-298) -- a closure that returns anything but finite reals fails the definition."""
    assoc = dict(assoc)
    params = assoc.get("Parameters")
    if not params or "LogLikelihoodFunction" not in assoc:
        return inferenceObject(None)
    assoc["ParameterSymbols"] = [p[0] for p in params]
    if "LogPriorPDFFunction" not in assoc:
        assoc["LogPriorPDFFunction"] = _log_prior_function(assoc.get("PriorDistribution"), params)
    pts = random_domain_points(params, 100)
    prior_vals = np.array([assoc["LogPriorPDFFunction"](t) for t in pts], dtype=np.float64)
    if not np.all(np.isfinite(prior_vals)):
        return inferenceObject(None)
    ll = assoc["LogLikelihoodFunction"]
    try:
        vals = np.asarray(ll(pts), dtype=np.float64)             # one batched sweep (B x p -> B)
        if vals.shape != (len(pts),):
            raise ValueError
    except (TypeError, ValueError):
        vals = np.array([ll(t) for t in pts], dtype=np.float64)
    if not np.all(np.isfinite(vals)):
        return inferenceObject(None)
    return inferenceObject(assoc)


def predictFromGaussianProcess(obj_or_examples, pts, kernel=None, theta=None, meanFunction=None):
    """BGP:332-394.  Two forms:
      predictFromGaussianProcess(obj, pts)            obj has "GaussianProcessData" and "Samples"
          (BGP:343-376): one Normal per posterior sample, mixed with the CrudePosteriorWeights.
          pts may be an int > 1: regular grid over the data bounds (BGP:332-341).
      predictFromGaussianProcess((X, Y), pts, kernel, theta[, meanFunction])
          direct form with the hyper-parameters baked in (BGP:378-394); duplicates in pts are
          removed first (DeleteDuplicates, BGP:380).
    Returns a dict with "Points" [M,d], "Weights" [S], "Mean" [S,M], "StandardDeviation" [S,M]:
    the content of Association[x* -> MixtureDistribution[weights, {NormalDistribution[mu, sigma]..}]]
    (for the direct form S = 1).  The variance includes the test-point nugget (BGP:113)."""
    if isinstance(obj_or_examples, inferenceObject):
        obj = obj_or_examples
        if obj.failed or "GaussianProcessData" not in obj or "Samples" not in obj:
            return None
        X = obj["Data"][0]
        if isinstance(pts, (int, np.integer)):
            if pts <= 1 or X.shape[1] != 1:
                return None
            pts = np.linspace(X.min(), X.max(), int(pts))         # CoordinateBoundsArray, BGP:336-339
        P = dataNormalForm(pts)
        if P is None or isinstance(P, tuple):
            return None
        handle = obj["GaussianProcessData"]["HIPHandle"]
        samples = obj["Samples"]
        points = np.array([s["Point"] for s in samples], dtype=np.float64)
        weights = np.array([s["CrudePosteriorWeight"] for s in samples], dtype=np.float64)
        mf = obj["GaussianProcessData"]["ModelFunctions"]
        nugget_fn = mf["NuggetFunction"] if callable(mf["NuggetFunction"]) else None
        mean_fn = mf["MeanFunction"] if callable(mf["MeanFunction"]) else None
        return _predict_samples(handle, points, weights, P, nugget_fn, mean_fn, X)
    norm = dataNormalForm(obj_or_examples)
    P = dataNormalForm(pts)
    if norm is None or not isinstance(norm, tuple) or P is None or norm[1].shape[1] != 1:
        return None                                               # Return[$Failed], BGP:383-390
    _, first = np.unique(P, axis=0, return_index=True)
    P = P[np.sort(first)]
    mean = "zero" if meanFunction in (None, 0, "Zero", "zero") else "const"
    handle = _lib.Handle(norm[0], norm[1][:, 0], _resolve_kernel(kernel), mean)
    try:
        return _predict_samples(handle, np.atleast_2d(np.asarray(theta, dtype=np.float64)), np.ones(1), P)
    finally:
        handle.close()


def predictiveDistribution(obj, inputs=None, estimate=None):
    """BS:1373-1416 for GP objects.  The reference's predictiveDistribution needs a "GeneratingDistribution"
    (BS:1381-1387), which a GP object does not carry; BASELINE.json's north_star names predictiveDistribution as the
    prediction API, so for objects with "GaussianProcessData" it forwards to predictFromGaussianProcess.
    estimate = "MaximumLikelihood" / "MAP" first reduces "Samples" to the single best sample (BS:1389-1416:
    TakeLargestBy LogLikelihood resp. LogLikelihood + LogPriorPDF).  Returns None ($Failed) for an unsampled object
    (BS:1375-1380) or a missing `inputs`."""
    if not isinstance(obj, inferenceObject) or obj.failed or "Samples" not in obj:
        return None                                               # predictiveDistribution::unsampled
    if "GaussianProcessData" not in obj or inputs is None:
        return None                                               # predictiveDistribution::MissGenDist
    if estimate is not None:
        key = {"maximumlikelihood": lambda smp: smp["LogLikelihood"],
               "map": lambda smp: smp["LogLikelihood"] + smp.get("LogPriorPDF", 0.0)}.get(str(estimate).lower())
        if key is None:
            raise ValueError('estimate must be None, "MaximumLikelihood" or "MAP"')
        obj = obj.append({"Samples": [max(obj["Samples"], key=key)]})
    return predictFromGaussianProcess(obj, inputs)


def _predict_samples(handle, points, weights, P, nugget_fn=None, mean_fn=None, X=None):
    """One batched pass over all samples (gphip_predict_samples); singular samples -> NaN rows.  Point-dependent
    nugget / mean functions are evaluated per sample at the training AND the test points (BGP:113, 408)."""
    if nugget_fn is not None or mean_fn is not None:
        mean, var, info = handle.predict_samples_pw(points, P, _pointwise(mean_fn, X, points), _pointwise(nugget_fn, X, points),
                                                    _pointwise(mean_fn, P, points), _pointwise(nugget_fn, P, points))
    else:
        mean, var, info = handle.predict_samples(points, P)
    bad = info != 0
    mean[bad], var[bad] = np.nan, np.nan
    with np.errstate(invalid="ignore"):
        sd = np.sqrt(var)                                          # Sqrt, BGP:414
    return {"Points": P, "Weights": weights, "Mean": mean, "StandardDeviation": sd}


def _direct_handle(examples, kernel, theta, meanFunction):
    """(handle fitted at theta, X) for the direct forms below; None when the data are not GP data or theta does not factor."""
    norm = dataNormalForm(examples)
    if norm is None or not isinstance(norm, tuple) or norm[1].shape[1] != 1:
        return None
    mean = "zero" if meanFunction in (None, 0, "Zero", "zero") else "const"
    handle = _lib.Handle(norm[0], norm[1][:, 0], _resolve_kernel(kernel), mean)
    if handle.fit(np.asarray(theta, dtype=np.float64).ravel()) != 0:
        handle.close()
        return None
    return handle


def predictJointFromGaussianProcess(examples, pts, kernel, theta, meanFunction=None):
    """Joint form of the direct predictFromGaussianProcess((X, Y), pts, kernel, theta[, meanFunction]): duplicates in pts are
    removed first (as BGP:380), then {"Points" [M,d], "Mean" [M], "Covariance" [M,M]} -- the MultinormalDistribution of noisy
    observations at the points, whose diagonal is the per-point variance of predictFromGaussianProcess.  None on bad data or a
    theta whose covariance matrix does not factor."""
    P = dataNormalForm(pts)
    if P is None or isinstance(P, tuple):
        return None
    _, first = np.unique(P, axis=0, return_index=True)
    P = P[np.sort(first)]
    handle = _direct_handle(examples, kernel, theta, meanFunction)
    if handle is None:
        return None
    try:
        mean, cov = handle.predict_cov(P, latent=False)
    finally:
        handle.close()
    return {"Points": P, "Mean": mean, "Covariance": cov}


def predictGradientFromGaussianProcess(obj_or_examples, pts, kernel=None, theta=None, meanFunction=None):
    """How the prediction changes when the test point moves (gphip_predict_grad; no reference counterpart).  The two forms of
    predictFromGaussianProcess:
      predictGradientFromGaussianProcess((X, Y), pts, kernel, theta[, meanFunction])      duplicates in pts are removed first;
          {"Points" [M,d], "Mean" [M], "StandardDeviation" [M], "MeanGradient" [M,d], "VarianceGradient" [M,d]}
      predictGradientFromGaussianProcess(obj, pts)     obj has "GaussianProcessData" and "Samples": the same arrays per
          posterior sample ([S,M] / [S,M,d]) with "Weights" [S], from a host loop of fit + predict_grad over the samples
          (samples whose covariance matrix does not factor give NaN rows).
    Values are in the handle's units, as predictFromGaussianProcess returns them; the variance is that of a noisy observation
    (its gradient is that of the latent variance).  None on bad data, a theta that does not factor, and for objects with a
    callable nugget or mean function (dm/dx of a host function is unknown)."""
    if isinstance(obj_or_examples, inferenceObject):
        obj = obj_or_examples
        if obj.failed or "GaussianProcessData" not in obj or "Samples" not in obj:
            return None
        mf = obj["GaussianProcessData"]["ModelFunctions"]
        if callable(mf["NuggetFunction"]) or callable(mf["MeanFunction"]):
            return None
        P = dataNormalForm(pts)
        if P is None or isinstance(P, tuple):
            return None
        handle = obj["GaussianProcessData"]["HIPHandle"]
        points = np.array([s["Point"] for s in obj["Samples"]], dtype=np.float64)
        weights = np.array([s["CrudePosteriorWeight"] for s in obj["Samples"]], dtype=np.float64)
        return _predict_grad_samples(handle.fit, handle.predict_grad, points, weights, P)
    P = dataNormalForm(pts)
    if P is None or isinstance(P, tuple):
        return None
    _, first = np.unique(P, axis=0, return_index=True)
    P = P[np.sort(first)]
    handle = _direct_handle(obj_or_examples, kernel, theta, meanFunction)
    if handle is None:
        return None
    try:
        mean, var, dmean, dvar = handle.predict_grad(P)
    finally:
        handle.close()
    with np.errstate(invalid="ignore"):
        return {"Points": P, "Mean": mean, "StandardDeviation": np.sqrt(var), "MeanGradient": dmean, "VarianceGradient": dvar}


def _predict_grad_samples(fit, predict_grad, points, weights, P):
    """the per-sample arrays of the two predictGradient functions: fit(theta) -> info, predict_grad(P) -> the four arrays"""
    S, (M, d) = len(points), P.shape
    mean, var = np.full((S, M), np.nan), np.full((S, M), np.nan)
    dmean, dvar = np.full((S, M, d), np.nan), np.full((S, M, d), np.nan)
    for s, th in enumerate(points):
        if fit(th) == 0:
            mean[s], var[s], dmean[s], dvar[s] = predict_grad(P)
    with np.errstate(invalid="ignore"):
        return {"Points": P, "Weights": weights, "Mean": mean, "StandardDeviation": np.sqrt(var), "MeanGradient": dmean,
                "VarianceGradient": dvar}


def predictiveLogDensity(examples, heldout, kernel, theta, meanFunction=None):
    """log N(ys | mean, Covariance) of held-out data heldout = (Xs, ys) under the GP of (X, Y) at theta: the joint predictive
    log density (the correlations between the held-out points included).  None on bad data or a failed factorisation."""
    P = dataNormalForm(heldout[0])
    if P is None or isinstance(P, tuple):
        return None
    ys = np.asarray(heldout[1], dtype=np.float64).ravel()
    if ys.shape != (len(P),):
        return None
    handle = _direct_handle(examples, kernel, theta, meanFunction)
    if handle is None:
        return None
    try:
        value, info = handle.predict_logpdf(P, ys)
    finally:
        handle.close()
    return value if info == 0 else None


def extendGaussianProcess(handle, new_examples):
    """The observe step of a sequential design loop (gphip_extend; no reference counterpart): new_examples = (X_new, y_new) in
    any form dataNormalForm takes, one output column, into the fit resident in `handle` (a _lib.Handle after fit) without
    refactoring it.  Returns a new _lib.Handle on all the points with the fit of the same theta resident -- predict,
    predict_grad, solve, extend again, .. work on it as after fit; `handle` itself is untouched and both are closed on their own --
    or None on bad data, non-finite outputs and new points whose predictive covariance does not factor (duplicates at a tiny
    noise level)."""
    norm = dataNormalForm(new_examples)
    if norm is None or not isinstance(norm, tuple) or norm[1].shape[1] != 1 or norm[0].shape[1] != handle.d or len(norm[0]) < 1:
        return None
    new, _, info = handle.extend(norm[0], norm[1][:, 0])
    return new if info == 0 else None


def gaussianProcessFunctionSamples(obj, pts, n: int, seed: int = 0, latent: bool = True):
    """n draws of the function values at pts from the posterior MIXTURE of a sampled GP object: each draw picks a theta from
    "Samples" by CrudePosteriorWeight (numpy generator seeded by `seed`), then the values come from the joint predictive
    distribution of that theta (one fit and one gphip_predict_draws per distinct theta).  latent = True: draws of f;
    False: of noisy observations.  Returns {"Points" [M,d], "Sample" [n] (index into "Samples"), "Values" [n,M]}; rows of a
    theta that does not factor are NaN.  None for an unsampled object and for objects with a point-dependent nugget or
    mean function (not supported by the joint path).  pts may be an int > 1 as for predictFromGaussianProcess.
    A sampled sparse object (defineSparseGaussianProcess) is taken as well: the same draw-to-sample assignment and per-theta
    seeds, one fit(theta, obj["Jitter"]) and one gphip_sparse_predict_draws per distinct theta."""
    if not isinstance(obj, inferenceObject) or obj.failed or "Samples" not in obj:
        return None
    sparse = "SparseGaussianProcessData" in obj
    if not sparse:
        if "GaussianProcessData" not in obj:
            return None
        mf = obj["GaussianProcessData"]["ModelFunctions"]
        if callable(mf["NuggetFunction"]) or callable(mf["MeanFunction"]):
            return None
    X = obj["Data"][0]
    if isinstance(pts, (int, np.integer)):
        if pts <= 1 or X.shape[1] != 1:
            return None
        pts = np.linspace(X.min(), X.max(), int(pts))
    P = dataNormalForm(pts)
    if P is None or isinstance(P, tuple) or int(n) < 1:
        return None
    handle = obj["SparseGaussianProcessData" if sparse else "GaussianProcessData"]["HIPHandle"]
    samples = obj["Samples"]
    points = np.array([s["Point"] for s in samples], dtype=np.float64)
    w = np.array([s["CrudePosteriorWeight"] for s in samples], dtype=np.float64)
    which = np.random.default_rng(seed).choice(len(samples), size=int(n), p=w / w.sum())
    values = np.full((int(n), len(P)), np.nan)
    for k in np.unique(which):
        rows = np.flatnonzero(which == k)
        if (handle.fit(points[k], obj["Jitter"]) if sparse else handle.fit(points[k])) != 0:
            continue
        key = int(np.random.SeedSequence([int(seed) & (2**63 - 1), int(k)]).generate_state(1, np.uint64)[0])
        out, info = handle.predict_draws(P, len(rows), seed=key, latent=latent)
        if info == 0:
            values[rows] = out
    return {"Points": P, "Sample": which, "Values": values}


class posteriorFunctionSamples:
    """What samplePathsFromGaussianProcess returns: n coherent draws of the latent posterior function.  f(pts) -> [n, M];
    f.gradient(pts) -> [n, M, d]; f.own(pts[n, M, d]) -> [n, M] and f.own_gradient(..) -> [n, M, d]: every draw at its own points;
    f.maximize(bounds) -> every draw's maximiser over a box; f.sample [n] = the index into "Samples" each draw belongs to (zeros
    in the direct form).
    Rows of a theta that does not factor are NaN.  close() (or the with block) releases the device objects."""

    def __init__(self, parts, n, d, inverse, scale, owned=None):
        self._parts, self.n, self.d = parts, int(n), int(d)             # parts: [(rows, _lib.Paths)]
        self._inverse, self._scale, self._owned = inverse, scale, owned
        self.sample = np.zeros(self.n, dtype=np.int64)

    def _points(self, pts):
        P = dataNormalForm(pts)
        if P is None or isinstance(P, tuple) or P.shape[1] != self.d:
            raise ValueError("pts must be M points of dimension %d" % self.d)
        return P

    def __call__(self, pts):
        P = self._points(pts)
        out = np.full((self.n, len(P)), np.nan)
        for rows, paths in self._parts:
            out[rows] = paths.eval(P)
        return out if self._inverse is None else np.asarray(self._inverse(out), dtype=np.float64).reshape(out.shape)

    def gradient(self, pts):
        P = self._points(pts)
        out = np.full((self.n, len(P), self.d), np.nan)
        for rows, paths in self._parts:
            out[rows] = paths.eval(P, grad=True)[1]
        return out * self._scale

    def _own(self, pts, grad):
        """(f [n, M], df/dx [n, M, d] or None) of every draw at its own points, in the normalised output units: one eval_own call
        per paths object on the rows of its draws; NaN rows for a theta that did not factor"""
        P = np.asarray(pts, dtype=np.float64)
        if P.ndim != 3 or P.shape[0] != self.n or P.shape[1] < 1 or P.shape[2] != self.d:
            raise ValueError("pts must have shape [%d, M, %d] with M >= 1" % (self.n, self.d))
        out = np.full(P.shape[:2], np.nan)
        dout = np.full(P.shape, np.nan) if grad else None
        for rows, paths in self._parts:
            res = paths.eval_own(P[rows], grad=grad)
            if grad:
                out[rows], dout[rows] = res
            else:
                out[rows] = res
        return out, dout

    def own(self, pts):
        """f_s(pts[s, t]) -> [n, M]: every draw at its own M points, pts[n, M, d] (gphip_paths_eval_own); units as __call__"""
        out = self._own(pts, False)[0]
        return out if self._inverse is None else np.asarray(self._inverse(out), dtype=np.float64).reshape(out.shape)

    def own_gradient(self, pts):
        """df_s/dx at pts[s, t] -> [n, M, d], scaled as gradient"""
        return self._own(pts, True)[1] * self._scale

    def maximize(self, bounds, candidates: int = 1024, starts: int = 4, iterations: int = 50, seed: int = 0):
        """argmax of every draw over the box bounds [d, 2] (rows (lo, hi)): {"x" [n, d], "f" [n]} in data units; NaN for the draws
        of a theta that did not factor.  `candidates` uniform points of numpy.random.default_rng(seed) are evaluated for all
        draws in one shared call, the `starts` best of every draw are ascended in lock step (_ascend_batched: every iteration is
        one eval_own call with gradients per paths object), and the best of a draw's starts is returned.  The work is done in
        the normalised output units; under a decreasing output map the draws are minimised there."""
        box = np.asarray(bounds, dtype=np.float64).reshape(-1, 2)
        if box.shape[0] != self.d or not np.all(box[:, 1] >= box[:, 0]) or int(candidates) < 1 or int(starts) < 1 or int(iterations) < 1:
            raise ValueError("bounds must be %d rows (lo, hi) with hi >= lo; candidates, starts and iterations at least 1" % self.d)
        lo, hi = box[:, 0], box[:, 1]
        sign = -1.0 if self._scale < 0 else 1.0
        cand = lo + (hi - lo) * np.random.default_rng(seed).random((int(candidates), self.d))
        vals = self(cand)                                                # data units: the map is monotone, the best are the best
        vals = np.where(np.isnan(vals), -np.inf, vals)
        best = np.argsort(-vals, axis=1, kind="stable")[:, :min(int(starts), len(cand))]

        def fg(X):
            f, g = self._own(X, True)
            return sign * f, sign * g

        X, f = _ascend_batched(fg, cand[best], lo, hi, int(iterations))
        f = np.where(np.isnan(f), -np.inf, f)
        k = np.argmax(f, axis=1)
        rows = np.arange(self.n)
        x, fz = X[rows, k], sign * f[rows, k]
        dead = ~np.isfinite(fz)
        x[dead], fz[dead] = np.nan, np.nan
        return {"x": x, "f": fz if self._inverse is None else np.asarray(self._inverse(fz), dtype=np.float64).reshape(fz.shape)}

    def close(self):
        for _, paths in self._parts:
            paths.close()
        self._parts = []
        if self._owned is not None:
            self._owned.close()
            self._owned = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def samplePathsFromGaussianProcess(obj_or_examples, n: int, kernel=None, theta=None, meanFunction=None, Features: int = 1024, seed: int = 0,
                                   Batched: bool = False):
    """n pathwise draws of the latent posterior function (gphip_paths_create; no reference counterpart) that can be evaluated at
    any points, and differentiated, after they have been drawn: Thompson sampling, optimum-location sampling.  Two forms, as
    predictFromGaussianProcess:
      samplePathsFromGaussianProcess(obj, n)                         a sampled GP object: every draw picks a theta from "Samples" by
          CrudePosteriorWeight (numpy generator seeded by `seed`, the assignment of gaussianProcessFunctionSamples), one fit and
          one paths object per distinct theta used;
      samplePathsFromGaussianProcess((X, Y), n, kernel, theta[, meanFunction])   the direct form.
    Features: random Fourier features per kernel term (the prior is approximated with error O(1 / sqrt(Features))).  Values come
    back in the units of the data ("DataPreProcessors" undone), gradients scaled accordingly.
    Batched=True on a sampled object: the same draw-to-sample assignment and per-theta keys, but the distinct thetas (ascending
    sample index) go with their counts and keys into ONE Handle.sample_paths_samples call (gphip_paths_create_samples: the
    thetas factored together, no fit per theta), and the result has a single part: every evaluation, and every iteration of
    maximize, is one device call.  Draw i is the same function as draw i of Batched=False, to rounding; the draws of a theta
    that does not factor are NaN; the handle is left without a fit.  Ignored in the direct form.
    On a GP object the paths objects live on the object's own "HIPHandle": until the result's close() (or the end of its `with`
    block) that handle cannot be closed (Handle.close raises GphipError, status 4), and it is left fitted at the last theta
    used here, not at the theta it held before the call.  The direct form owns a handle of its own and closes it with the result.
    Returns a posteriorFunctionSamples, or None for bad arguments, an unsampled object, point-dependent nugget / mean functions
    and a run-time compiled kernel."""
    if int(n) < 1 or int(Features) < 1:
        return None
    if isinstance(obj_or_examples, inferenceObject):
        obj = obj_or_examples
        if obj.failed or "GaussianProcessData" not in obj or "Samples" not in obj:
            return None
        mf = obj["GaussianProcessData"]["ModelFunctions"]
        if callable(mf["NuggetFunction"]) or callable(mf["MeanFunction"]):
            return None
        handle = obj["GaussianProcessData"]["HIPHandle"]
        if isinstance(handle.kernel, _lib.CustomKernel):
            return None
        samples = obj["Samples"]
        points = np.array([s["Point"] for s in samples], dtype=np.float64)
        w = np.array([s["CrudePosteriorWeight"] for s in samples], dtype=np.float64)
        which = np.random.default_rng(seed).choice(len(samples), size=int(n), p=w / w.sum())
        used = np.unique(which)                                          # the distinct thetas, ascending sample index
        keys = [int(np.random.SeedSequence([int(seed) & (2**63 - 1), int(k)]).generate_state(1, np.uint64)[0]) for k in used]
        rows = [np.flatnonzero(which == k) for k in used]
        parts = []
        if Batched:                                                      # one mixture object; its draws are ordered theta by theta
            paths = handle.sample_paths_samples(points[used], [len(r) for r in rows], keys, int(Features))
            if paths is not None:
                parts.append((np.concatenate(rows), paths))
        else:
            for k, key, r in zip(used, keys, rows):
                if handle.fit(points[k]) != 0:
                    continue
                paths = handle.sample_paths(len(r), int(Features), key)
                if paths is not None:
                    parts.append((r, paths))
        inverse, scale = _output_scale(obj)
        res = posteriorFunctionSamples(parts, n, handle.d, inverse, scale)
        res.sample = which
        return res
    norm = dataNormalForm(obj_or_examples)
    if norm is None or not isinstance(norm, tuple) or norm[1].shape[1] != 1 or theta is None:
        return None
    k = _resolve_kernel(kernel)
    if isinstance(k, _lib.CustomKernel):
        return None
    mean = "zero" if meanFunction in (None, 0, "Zero", "zero") else "const"
    handle = _lib.Handle(norm[0], norm[1][:, 0], k, mean)
    paths = handle.sample_paths(int(n), int(Features), int(seed)) if handle.fit(np.asarray(theta, dtype=np.float64).ravel()) == 0 else None
    if paths is None:
        handle.close()
        return None
    return posteriorFunctionSamples([(np.arange(int(n)), paths)], n, handle.d, None, 1.0, owned=handle)


def _ascend_batched(fg, X0, lo, hi, iterations, trace=None):
    """Projected gradient ascent of n x R independent (function, point) pairs in lock step; pure numpy.  fg(X[n, R, d]) ->
    (f[n, R], g[n, R, d]) is called exactly once per iteration, on all pairs.  One step length per pair: a trial
    clip(x + step g) that lowers its pair's value is rejected and the pair's step is halved; an accepted trial sets the next
    step by the Barzilai-Borwein quotient |s . s / s . y| of the pair (s, y = the change of the point and of the gradient;
    doubled where the quotient does not exist).  The first iteration evaluates the projected start; the first step moves a
    tenth of the widest side of the box along the largest gradient component.  No pair's value ever decreases.  A pair whose
    values are NaN stays at its start.  Returns (X[n, R, d], f[n, R]); trace: a list that receives a copy of f per iteration."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    X = np.clip(np.asarray(X0, dtype=np.float64), lo, hi)
    f = g = step = None
    for it in range(int(iterations)):
        if it == 0:
            f, g = fg(X)
            f, g = np.array(f, dtype=np.float64), np.array(g, dtype=np.float64)
            gmax = np.abs(g).max(axis=2)
            width = float(np.max(hi - lo))
            step = np.where(gmax > 0, 0.1 * (width if width > 0 else 1.0) / np.where(gmax > 0, gmax, 1.0), 1.0)
        else:
            Xt = np.clip(X + step[:, :, None] * g, lo, hi)
            ft, gt = fg(Xt)
            ok = ft >= f                                                 # (NaN: rejected)
            s, y = Xt - X, gt - g
            ss, sy = np.einsum("nrc,nrc->nr", s, s), np.einsum("nrc,nrc->nr", s, y)
            with np.errstate(divide="ignore", invalid="ignore"):
                bb = np.abs(ss / sy)
            grown = np.where(np.isfinite(bb) & (bb > 0), bb, np.where(ss > 0, 2.0 * step, step))     # (a pair held by the box keeps its step)
            step = np.clip(np.where(ok, grown, 0.5 * step), 1e-300, 1e100)
            X = np.where(ok[:, :, None], Xt, X)
            g = np.where(ok[:, :, None], gt, g)
            f = np.where(ok, ft, f)
        if trace is not None:
            trace.append(f.copy())
    return X, f


def thompsonSampleFromGaussianProcess(obj_or_examples, n: int, bounds, kernel=None, theta=None, meanFunction=None, Features: int = 1024,
                                      seed: int = 0, Batched: bool = False, **maximize_options):
    """Thompson sampling in one call: n pathwise draws of the latent posterior function (samplePathsFromGaussianProcess, both
    forms) and the maximiser of each over the box `bounds` (posteriorFunctionSamples.maximize(bounds, seed=seed,
    **maximize_options)); the draws are released before it returns.  {"x" [n, d], "f" [n], "sample" [n]} in data units, or None
    wherever samplePathsFromGaussianProcess returns None.  Batched=True on a sampled object: one mixture paths object over all
    thetas used (samplePathsFromGaussianProcess), so one creation call and one evaluation call per ascent step."""
    draws = samplePathsFromGaussianProcess(obj_or_examples, n, kernel, theta, meanFunction, Features, seed, Batched=Batched)
    if draws is None:
        return None
    with draws:
        best = draws.maximize(bounds, seed=seed, **maximize_options)
        return {"x": best["x"], "f": best["f"], "sample": np.array(draws.sample)}


def _output_scale(obj):
    """(inverse, scale) of the "Output" pre-processor of an object defined on normalizeData(..) data: y = inverse(z), and the
    factor by which it stretches a standard deviation; (None, 1.0) for an object on raw data."""
    pre = obj.get("DataPreProcessors") if hasattr(obj, "get") else None
    if not pre or "Output" not in pre:
        return None, 1.0
    inv = pre["Output"]["InverseFunction"]
    return inv, float(np.ravel(inv(np.array([1.0])))[0] - np.ravel(inv(np.array([0.0])))[0])


def leaveOneOutFromGaussianProcess(obj, theta=None):
    """Leave-one-out cross-validation of the training data of a HIP-backed GP object (R&W GPML 5.4.2; one factorisation per
    theta, gphip_loo): how well the model predicts each point from all the others.  Returns, in the units of the data
    ("DataPreProcessors" undone):
        "Mean" [N], "StandardDeviation" [N]   of the leave-one-out predictive distribution of each training output
        "LogDensity" [N]                      log p(y_i | X, y_-i)
        "LogPseudoLikelihood"                 their sum
        "StandardizedResiduals" [N]           (y_i - Mean_i) / StandardDeviation_i
    theta given: that hyper-parameter vector.  theta=None on a sampled object: the posterior mixture over its "Samples" -- per
    point, LogDensity = log of the CrudePosteriorWeight-weighted mean of exp(log p_i) over the samples, Mean / StandardDeviation
    the moments of the mixture of the per-sample normals (one gphip_loo per distinct theta; samples that do not factor carry no
    weight).  None for a failed object, an object with point-dependent nugget / mean functions, a theta that does not factor,
    or theta=None without "Samples"."""
    if not isinstance(obj, inferenceObject) or obj.failed or "GaussianProcessData" not in obj:
        return None
    mf = obj["GaussianProcessData"]["ModelFunctions"]
    if callable(mf["NuggetFunction"]) or callable(mf["MeanFunction"]):
        return None
    handle = obj["GaussianProcessData"]["HIPHandle"]
    y = np.asarray(obj["Data"][1], dtype=np.float64)[:, 0]
    if theta is not None:
        res = handle.loo(np.asarray(theta, dtype=np.float64).ravel())
        if res["info"] != 0:
            return None
        mean, var, logp = res["mean"], res["var"], res["logp"]
    else:
        if "Samples" not in obj:
            return None
        samples = obj["Samples"]
        points = np.array([s["Point"] for s in samples], dtype=np.float64)
        w = np.array([s["CrudePosteriorWeight"] for s in samples], dtype=np.float64)
        uniq, which = np.unique(points, axis=0, return_inverse=True)
        which = np.ravel(which)
        wu = np.array([w[which == k].sum() for k in range(len(uniq))])
        rows = [handle.loo(t) for t in uniq]
        ok = np.array([r["info"] == 0 for r in rows])
        if not ok.any() or wu[ok].sum() <= 0:
            return None
        wu = wu[ok] / wu[ok].sum()
        mus = np.array([r["mean"] for r, good in zip(rows, ok) if good])
        vs = np.array([r["var"] for r, good in zip(rows, ok) if good])
        lps = np.array([r["logp"] for r, good in zip(rows, ok) if good])
        top = lps.max(axis=0)
        logp = top + np.log((wu[:, None] * np.exp(lps - top)).sum(axis=0))
        mean = (wu[:, None] * mus).sum(axis=0)
        var = (wu[:, None] * (vs + mus * mus)).sum(axis=0) - mean * mean
    sd = np.sqrt(var)
    resid = (y - mean) / sd
    inv, scale = _output_scale(obj)
    if inv is not None:
        mean, sd, logp = np.ravel(inv(mean)), sd * abs(scale), logp - math.log(abs(scale))
    return {"Mean": mean, "StandardDeviation": sd, "LogDensity": logp, "LogPseudoLikelihood": float(np.sum(logp)),
            "StandardizedResiduals": resid}


def mixture_moments(pred: Mapping):
    """Mean and variance of the per-point MixtureDistribution (what regressionPlot1D draws, BV:310-374)."""
    w = np.asarray(pred["Weights"], dtype=np.float64)
    w = w / w.sum()
    mu, sd = pred["Mean"], pred["StandardDeviation"]
    m = w @ mu
    return m, w @ (sd ** 2 + mu ** 2) - m ** 2


def mixture_percentiles(pred: Mapping, levels: Sequence[float] = (0.95, 0.5, 0.05)):
    """InverseCDF of every per-point MixtureDistribution at `levels` -- the curves regressionPlot1D draws
    by default ("DistributionPercentiles" -> {0.95, 0.5, 0.05}, BV:303-308, 351-352).  Returns an array
    len(levels) x M.  The mixture CDF is monotone, so a bracketed bisection + Newton polish per point
    is exact to the last bits; everything is vectorised over the M test points."""
    from scipy.special import ndtr
    levels = np.asarray(levels, dtype=np.float64)
    if levels.ndim != 1 or levels.size == 0 or levels.min() <= 0.0 or levels.max() >= 1.0:
        raise ValueError("levels must lie strictly between 0 and 1 (BV:351)")
    w = np.asarray(pred["Weights"], dtype=np.float64)
    w = w / w.sum()
    mu = np.asarray(pred["Mean"], dtype=np.float64)
    sd = np.asarray(pred["StandardDeviation"], dtype=np.float64)
    keep = w > 0.0
    w, mu, sd = w[keep], mu[keep], sd[keep]

    def cdf(x):                                            # x: (M,) -> (M,)
        return np.einsum("s,sm->m", w, ndtr((x[None, :] - mu) / sd))

    def pdf(x):
        z = (x[None, :] - mu) / sd
        return np.einsum("s,sm->m", w, np.exp(-0.5 * z * z) / (sd * np.sqrt(2.0 * np.pi)))

    out = np.empty((levels.size, mu.shape[1]))
    span = 9.0 * sd                                       # every component's mass to ~1e-19 lies inside
    for k, q in enumerate(levels):
        lo, hi = (mu - span).min(axis=0), (mu + span).max(axis=0)
        for _ in range(60):                               # bisection: brackets shrink by 2^-60
            mid = 0.5 * (lo + hi)
            below = cdf(mid) < q
            lo = np.where(below, mid, lo)
            hi = np.where(below, hi, mid)
        x = 0.5 * (lo + hi)
        for _ in range(2):                                # Newton polish inside the bracket
            step = (cdf(x) - q) / np.maximum(pdf(x), 1e-300)
            x = np.clip(x - step, lo, hi)
        out[k] = x
    return out


def mixture_plot_moments(pred: Mapping):
    """The "Moments" option of regressionPlot1D (BV:340-349): per point the three curves
    {mean + sd + m3^(1/3), mean, mean - sd + m3^(1/3)} with m3 the third central moment of the mixture
    and the real cube root (Surd)."""
    w = np.asarray(pred["Weights"], dtype=np.float64)
    w = w / w.sum()
    mu = np.asarray(pred["Mean"], dtype=np.float64)
    sd = np.asarray(pred["StandardDeviation"], dtype=np.float64)
    m = w @ mu
    var = w @ (sd ** 2 + mu ** 2) - m ** 2
    dm = mu - m
    m3 = w @ (dm ** 3 + 3.0 * dm * sd ** 2)               # third central moment of a normal mixture
    s = np.sqrt(np.maximum(var, 0.0))
    skew = np.cbrt(m3)
    return np.stack([m + s + skew, m, m - s + skew])


# ---------------------------------------------------------------------------------------------
# persistence: an inferenceObject is a plain Association the user may
# Put/Export (BU:125); the device state (X, y resident; L, z after a fit) is rebuildable from it.
# ---------------------------------------------------------------------------------------------
def save_gaussian_process(obj, path: str, theta=None):
    """Writes data, kernel/mean names, parameter specs, samples (if any) and an optional fitted theta."""
    X, Y = obj["Data"]
    kern = obj["KernelName"]
    custom = isinstance(kern, _lib.CustomKernel)
    payload = {"X": X, "Y": Y, "kernel": "custom:" + kern.name if custom else kern, "mean": obj["MeanName"],
               "param_names": np.array([p[0] for p in obj["Parameters"]]),
               "param_lo": np.array([p[1] for p in obj["Parameters"]], dtype=np.float64),
               "param_hi": np.array([p[2] for p in obj["Parameters"]], dtype=np.float64)}
    if custom:                                                    # the function travels as its source text
        payload["kernel_body"] = kern.body
        payload["kernel_nparams"] = kern.nparams
    if "Samples" in obj:
        payload["sample_points"] = np.array([smp["Point"] for smp in obj["Samples"]], dtype=np.float64)
        payload["sample_logw"] = np.array([smp["CrudeLogPosteriorWeight"] for smp in obj["Samples"]])
    if theta is not None:
        payload["theta_fit"] = np.asarray(theta, dtype=np.float64)
    np.savez_compressed(path, **payload)


def load_gaussian_process(path: str, variablePrior="Uniform", trust_kernel_source: bool = False, **rules):
    """Rebuilds the object (new device handle, data uploaded again); if a fitted theta was saved the
    handle is re-fitted so predict/solve work immediately.  Returns (object, theta_fit or None).
    A checkpoint of a run-time compiled covariance function carries that function's C++ SOURCE TEXT, which loading
    compiles and runs on the device: such a file is executable content, not data.  It is refused unless the caller says
    the file comes from a trusted source (trust_kernel_source=True)."""
    z = np.load(path, allow_pickle=False)
    if "kernel_body" in z and not trust_kernel_source:
        raise ValueError(f"{path} carries the source text of a covariance function (kernel_body): loading compiles and runs it. "
                         "Pass trust_kernel_source=True if the file comes from a trusted source.")
    params = [(str(n), float(a), float(b)) for n, a, b in zip(z["param_names"], z["param_lo"], z["param_hi"])]
    kernel = None if str(z["kernel"]) == "null" else str(z["kernel"])
    if "kernel_body" in z:
        kernel = _lib.CustomKernel(str(z["kernel_body"]), int(z["kernel_nparams"]), name=str(z["kernel"])[len("custom:"):])
    mean = "Constant" if str(z["mean"]) == "const" else None
    obj = defineGaussianProcess((z["X"], z["Y"]), kernel, "Constant", mean, params, variablePrior, **rules)
    if obj.failed:
        return obj, None
    extra = {}
    if "sample_points" in z:
        logw = z["sample_logw"]
        extra["Samples"] = [{"Point": pt, "CrudeLogPosteriorWeight": float(lw), "CrudePosteriorWeight": float(np.exp(lw))}
                            for pt, lw in zip(z["sample_points"], logw)]
    theta = z["theta_fit"] if "theta_fit" in z else None
    if theta is not None:
        obj["GaussianProcessData"]["HIPHandle"].fit(theta)
    return (obj.append(extra) if extra else obj), theta


# ---------------------------------------------------------------------------------------------
# Sparse inducing-point GP (Titsias 2009; include/gphip.h gphip_sparse_*): for data sizes the exact path cannot hold
# ---------------------------------------------------------------------------------------------
def selectInducingPoints(X, m: int, seed: int = 0):
    """m distinct rows of X, chosen by the counter-based generator of synthetic.py: a partial Fisher-Yates shuffle of the row
    indices whose k-th swap partner comes from uniform k of stream STREAM_X at `seed`.  Deterministic; nothing cleverer: this
    is the START of optimizeInducingPoints, which moves the locations along the gradient of the bound."""
    from . import synthetic
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    n, m = len(X), int(m)
    if m < 1 or m > n:
        raise ValueError(f"m must be in 1 .. N = {n}")
    idx = np.arange(n)
    u = synthetic.uniform(synthetic.STREAM_X, 0, m, synthetic.SEED + 1000003 * (int(seed) + 1))
    for k in range(m):
        j = k + min(int(u[k] * (n - k)), n - k - 1)
        idx[k], idx[j] = idx[j], idx[k]
    return X[idx[:m]].copy()


def make_sparse_log_likelihood(handle: "_lib.SparseHandle", jitter: float = -1.0, nugget_fn=None, mean_fn=None, X=None):
    """The closure for "LogLikelihoodFunction" of a sparse object: theta -> F(theta), the collapsed lower bound on the log
    marginal likelihood; $MachineLogZero on numerical failure (info != 0), B x p -> B for a batch, like make_log_likelihood.
    A batch is ONE device call (SparseHandle.bound_batch), so every Metropolis step of nestedSampling is one call.
    nugget_fn / mean_fn: point-dependent nugget[x] / meanFunction[x] (callables f(X, theta) -> values[N], as
    make_log_likelihood takes them), evaluated here on the host for every theta; a 1-D or 2-D theta then is one
    SparseHandle.bound_batch_pw call."""
    pw = nugget_fn is not None or mean_fn is not None

    def one(theta):
        val, info = handle.bound(theta, jitter)
        if info != 0 or not math.isfinite(val):
            return MACHINE_LOG_ZERO
        return min(max(val, MACHINE_LOG_ZERO), -MACHINE_LOG_ZERO)

    def log_likelihood(theta):
        theta = np.asarray(theta, dtype=np.float64)
        if theta.ndim == 2 or pw:
            if theta.ndim == 2 and theta.shape[0] == 0:
                return np.zeros(0, dtype=np.float64)
            if pw:
                val, info = handle.bound_batch_pw(theta, jitter, _pointwise(mean_fn, X, theta), _pointwise(nugget_fn, X, theta))
            else:
                val, info = handle.bound_batch(theta, jitter)
            val = np.asarray(val, dtype=np.float64)
            bad = (np.asarray(info) != 0) | ~np.isfinite(val)
            res = np.where(bad, MACHINE_LOG_ZERO, np.clip(np.where(bad, 0.0, val), MACHINE_LOG_ZERO, -MACHINE_LOG_ZERO))
            return res if theta.ndim == 2 else float(res[0])
        return one(theta)
    return log_likelihood


def defineSparseGaussianProcess(data, kernel, inducing, nugget="Constant", meanFunction=None, variables=(),
                                variablePrior="Uniform", **rules) -> inferenceObject:
    """defineGaussianProcess for a sparse inducing-point GP: `inducing` = an int m (-> selectInducingPoints(X, m)) or an array
    [m, d]; the other arguments, parameter specs, priors and pre-processors are defineGaussianProcess's: nugget = "Constant" or
    a callable f(X, theta) -> variances[N], meanFunction = None / 0, "Constant" or a callable f(X, theta) -> means[N] (the
    handle then has the zero mean).  Extra rules: Jitter (default -1: the library's), Device, Precision, Seed (of the inducing-point choice).
    "LogLikelihoodFunction" of the returned object is the collapsed bound F(theta) <= log p(y | X, theta), so nestedSampling,
    laplace.selectHyperparameters(Criterion="MarginalLikelihood") and approximateEvidence run on it unchanged.
    "LogLikelihoodGradientFunction" returns (F, dF/dtheta) from the device's analytic gradient (gphip_sparse_bound_grad: one
    evaluation plus one more pass over the data, the jitter held fixed); rule Gradient="Differences" keeps the difference
    quotient instead: central differences of F with the step eps^(1/3) max(|theta_k|, 1e-2), 2p + 1 evaluations of the bound.
    With a callable nugget or mean it is always the difference quotient (the library cannot differentiate a host function of
    the point).  Also carries "InducingPoints" and "Jitter"; no leave-one-out keys."""
    if normalizedDataQ(data) and isinstance(data, Mapping) and "Input" in data:
        rules.setdefault("DataPreProcessors", {k: {"Function": v["Function"], "InverseFunction": v["InverseFunction"]}
                                               for k, v in data.items()})
        data = (data["Input"]["NormalizedData"], data["Output"]["NormalizedData"])
    norm = dataNormalForm(data)
    if norm is None or not isinstance(norm, tuple):
        return inferenceObject(None)
    X, Y = norm
    if Y.shape[1] != 1 or len(X) != len(Y):
        return inferenceObject(None)
    if isinstance(nugget, str) and nugget.lower() != "constant":
        raise ValueError('nugget must be "Constant" (Function[sn^2]) or a callable f(X, theta) -> variances[N]')
    if not (isinstance(nugget, str) or callable(nugget)):
        raise ValueError('nugget must be "Constant" (Function[sn^2]) or a callable f(X, theta) -> variances[N]')
    nugget_fn = nugget if callable(nugget) else None
    mean_fn = meanFunction if callable(meanFunction) else None
    pointwise = nugget_fn is not None or mean_fn is not None
    kname = _resolve_kernel(kernel)
    if isinstance(kname, str) and kname == "null":
        raise ValueError("a sparse GP needs a covariance function (the null kernel has nothing to approximate)")
    mean = "zero" if (mean_fn is not None or meanFunction in (None, 0, "Zero", "zero")) else "const"
    if mean == "const" and str(meanFunction).lower() not in ("constant", "const"):
        raise ValueError("meanFunction must be None/0, 'Constant' or a callable f(X, theta) -> means[N]")
    params = [tuple(v) for v in variables]
    if not params or any(len(v) != 3 for v in params):
        return inferenceObject(None)
    device = rules.pop("Device", None)
    precision = str(rules.pop("Precision", "Double")).lower()
    if precision not in ("double", "single"):
        raise ValueError('Precision must be "Double" or "Single"')
    jitter = float(rules.pop("Jitter", -1.0))
    seed = int(rules.pop("Seed", 0))
    gradient = str(rules.pop("Gradient", "Analytic")).lower()
    if gradient not in ("analytic", "differences"):
        raise ValueError('Gradient must be "Analytic" or "Differences"')
    if isinstance(inducing, (int, np.integer)):
        Z = selectInducingPoints(X, int(inducing), seed)
    else:
        Z = np.atleast_2d(np.asarray(inducing, dtype=np.float64))
        if Z.ndim != 2 or Z.shape[1] != X.shape[1] or len(Z) < 1:
            return inferenceObject(None)
    # the number of hyper-parameters is host logic (the kernel grammar / the CustomKernel, + sigma_n [+ mu]): a wrong count is
    # refused before any device is touched
    need = _lib.num_params(kname, X.shape[1], mean)
    if need != len(params):
        raise ValueError(f"kernel {kname!r} with mean {mean!r} on d={X.shape[1]} needs {need} "
                         f"hyper-parameters (l.., sigma_f, sigma_n[, mu]); got {len(params)}")
    handle = _lib.SparseHandle(X, Y[:, 0], Z, kname, mean, dtype=64 if precision == "double" else 32,
                               device=device)                     # raises loudly without the library / GPU
    loglik = make_sparse_log_likelihood(handle, jitter, nugget_fn, mean_fn, X)

    def log_likelihood_gradient(theta):
        """(F, dF/dtheta) from the device (gphip_sparse_bound_grad; F is the value "LogLikelihoodFunction" returns); sentinel and
        NaN gradient on numerical failure, like the exact object's."""
        theta = np.asarray(theta, dtype=np.float64).ravel()
        val, grad, info = handle.bound_grad(theta, jitter)
        if info != 0 or not math.isfinite(val):
            return MACHINE_LOG_ZERO, np.full(len(theta), np.nan)
        return min(max(val, MACHINE_LOG_ZERO), -MACHINE_LOG_ZERO), grad

    def log_likelihood_gradient_differences(theta):
        """(F, dF/dtheta) by central differences of the bound: a difference quotient, 2p + 1 bound evaluations, step
        eps^(1/3) max(|theta_k|, 1e-2).  Sentinel and NaN gradient on numerical failure."""
        theta = np.asarray(theta, dtype=np.float64).ravel()
        val = loglik(theta)
        grad = np.full(len(theta), np.nan)
        if val <= MACHINE_LOG_ZERO:
            return MACHINE_LOG_ZERO, grad
        for k in range(len(theta)):
            step = np.finfo(np.float64).eps ** (1.0 / 3.0) * max(abs(theta[k]), 1e-2)
            tp, tm = theta.copy(), theta.copy()
            tp[k] += step
            tm[k] -= step
            fp, fm = loglik(tp), loglik(tm)
            if fp <= MACHINE_LOG_ZERO or fm <= MACHINE_LOG_ZERO:
                return MACHINE_LOG_ZERO, np.full(len(theta), np.nan)
            grad[k] = (fp - fm) / (tp[k] - tm[k])
        return val, grad

    return defineInferenceProblem({
        "Data": (X, Y),
        "PriorDistribution": variablePrior,
        "Parameters": params,
        "KernelName": kname, "MeanName": mean, "LikelihoodBranch": "SparseBound",
        "InducingPoints": Z, "Jitter": jitter,
        "SparseGaussianProcessData": {
            "ModelFunctions": {
                "KernelFunction": ((kname.name, kname.body) if isinstance(kname, _lib.CustomKernel)
                                   else (kname, wl_kernel_expression(kname))),
                "NuggetFunction": nugget_fn if nugget_fn is not None else WL_NUGGET_EXPRESSION,
                "MeanFunction": mean_fn if mean_fn is not None else mean,
            },
            "HIPHandle": handle,
        },
        **rules,
        "LogLikelihoodGradientFunction": (log_likelihood_gradient if gradient == "analytic" and not pointwise
                                          else log_likelihood_gradient_differences),
        "LogLikelihoodFunction": loglik,
    })


def optimizeInducingPoints(obj, theta, Joint: bool = False, MaxIterations: int = 200, Tolerance=None):
    """Maximises the bound F of a sparse object over its inducing locations Z by L-BFGS-B with the device's gradient
    (gphip_sparse_bound_grad_inducing): over Z alone at the given theta, or (Joint=True) over (theta, Z) with theta inside the
    object's parameter box and Z unbounded.  Every evaluation is one set_inducing and one bound_grad_inducing; a failed one
    (info != 0) is the 1e300 wall of laplace.selectHyperparameters.  The jitter is the object's "Jitter"; when that is the
    default rule it is frozen at the value of the starting evaluation ("last_jitter"), so that the objective and the gradient
    describe one function.  Tolerance: L-BFGS-B stops when the largest component of the projected gradient is at most this
    (None: scipy's defaults).
    Returns a new inferenceObject: "InducingPoints" replaced, the handle (shared with `obj`) left at the best Z found, and
    "InducingOptimisation": {"Start": F0, "Maximum": F1, "Theta", "Iterations", "Evaluations", "Message"}; never a Z whose F is
    below the start's.  ValueError for a run-time compiled kernel; None for an object that is not a sparse GP object or whose
    starting evaluation fails."""
    from scipy.optimize import minimize
    if not isinstance(obj, inferenceObject) or obj.failed or "SparseGaussianProcessData" not in obj:
        return None
    if isinstance(obj["KernelName"], _lib.CustomKernel):
        raise ValueError("a run-time compiled kernel has no gradient in the inducing locations")
    handle = obj["SparseGaussianProcessData"]["HIPHandle"]
    theta0 = np.asarray(theta, dtype=np.float64).ravel()
    Z0 = np.array(obj["InducingPoints"], dtype=np.float64)
    m, d = Z0.shape
    p = len(theta0)
    handle.set_inducing(Z0)
    F0, _, _, info = handle.bound_grad_inducing(theta0, obj["Jitter"], with_theta=False)
    if info != 0 or not math.isfinite(F0):
        return None
    jitter = float(obj["Jitter"]) if obj["Jitter"] >= 0.0 else handle.get_option("last_jitter")
    if jitter != obj["Jitter"]:
        F0 = handle.bound(theta0, jitter)[0]
    best = {"F": F0, "theta": theta0.copy(), "Z": Z0.copy()}
    count = [0]

    def neg(x):
        th = np.clip(x[:p], lo, hi) if Joint else theta0
        Z = x[p if Joint else 0:].reshape(m, d)
        count[0] += 1
        handle.set_inducing(Z)
        F, g, gz, info = handle.bound_grad_inducing(th, jitter, with_theta=Joint)
        if info != 0 or not math.isfinite(F) or not np.all(np.isfinite(gz)) or (Joint and not np.all(np.isfinite(g))):
            return 1e300, np.zeros_like(x)                    # the sentinel: a wall, never an exception
        if F > best["F"]:
            best.update(F=F, theta=np.array(th, dtype=np.float64), Z=Z.copy())
        return -F, -(np.concatenate([g, gz.ravel()]) if Joint else gz.ravel())

    options = {"maxiter": int(MaxIterations)}
    if Tolerance is not None:
        options.update(gtol=float(Tolerance), ftol=0.0)
    if Joint:
        lo = np.array([v[1] for v in obj["Parameters"]], dtype=np.float64)
        hi = np.array([v[2] for v in obj["Parameters"]], dtype=np.float64)
        x0 = np.concatenate([np.clip(theta0, lo, hi), Z0.ravel()])
        bounds = list(zip(lo, hi)) + [(None, None)] * (m * d)
    else:
        lo = hi = None
        x0, bounds = Z0.ravel(), None
    res = minimize(neg, x0, jac=True, method="L-BFGS-B", bounds=bounds, options=options)
    handle.set_inducing(best["Z"])                            # the handle is left at the best Z found (its fit is dropped)
    msg = res.message.decode() if isinstance(res.message, bytes) else str(res.message)
    return obj.append({"InducingPoints": best["Z"],
                       "InducingOptimisation": {"Start": F0, "Maximum": best["F"], "Theta": best["theta"], "Iterations": int(res.nit),
                                                "Evaluations": count[0], "Message": msg}})


def _sparse_pointwise_functions(obj):
    """(nugget_fn, mean_fn) of a sparse object: its callables, None where the object has the constant form"""
    mf = obj["SparseGaussianProcessData"]["ModelFunctions"]
    return (mf["NuggetFunction"] if callable(mf["NuggetFunction"]) else None,
            mf["MeanFunction"] if callable(mf["MeanFunction"]) else None)


def predictFromSparseGaussianProcess(obj, pts, theta=None):
    """Prediction from a sparse object: for one theta, or (theta=None) the posterior mixture of a sampled object -- one Normal
    per posterior sample, mixed with the CrudePosteriorWeights.  Returns the dict of predictFromGaussianProcess: "Points" [M,d],
    "Weights" [S], "Mean" [S,M], "StandardDeviation" [S,M] (S = 1 for one theta); the variance includes the noise sn^2.  Samples
    whose fit fails give NaN rows.  The mixture is ONE device call over all samples (SparseHandle.predict_samples), which leaves no
    fit resident; the theta= form is fit + predict and leaves its fit resident.  None where the object is not a sparse GP object
    (or unsampled without a theta)."""
    if not isinstance(obj, inferenceObject) or obj.failed or "SparseGaussianProcessData" not in obj:
        return None
    X = obj["Data"][0]
    if isinstance(pts, (int, np.integer)):
        if pts <= 1 or X.shape[1] != 1:
            return None
        pts = np.linspace(X.min(), X.max(), int(pts))
    P = dataNormalForm(pts)
    if P is None or isinstance(P, tuple):
        return None
    handle = obj["SparseGaussianProcessData"]["HIPHandle"]
    nugget_fn, mean_fn = _sparse_pointwise_functions(obj)
    pw = nugget_fn is not None or mean_fn is not None
    if theta is not None:
        points, weights = np.atleast_2d(np.asarray(theta, dtype=np.float64)), np.ones(1)
        mean = np.full((len(points), len(P)), np.nan)
        var = np.full((len(points), len(P)), np.nan)
        for s, th in enumerate(points):
            if pw:                                                # the functions at the training and at the test points
                if handle.fit_pw(th, obj["Jitter"], _pointwise(mean_fn, X, th), _pointwise(nugget_fn, X, th)) == 0:
                    mean[s], var[s] = handle.predict_pw(P, False, _pointwise(mean_fn, P, th), _pointwise(nugget_fn, P, th))
            elif handle.fit(th, obj["Jitter"]) == 0:
                mean[s], var[s] = handle.predict(P)
    elif "Samples" in obj:
        points = np.array([s["Point"] for s in obj["Samples"]], dtype=np.float64)
        weights = np.array([s["CrudePosteriorWeight"] for s in obj["Samples"]], dtype=np.float64)
        if pw:
            mean, var, info = handle.predict_samples_pw(points, P, obj["Jitter"], False, _pointwise(mean_fn, X, points),
                                                        _pointwise(nugget_fn, X, points), _pointwise(mean_fn, P, points),
                                                        _pointwise(nugget_fn, P, points))
        else:
            mean, var, info = handle.predict_samples(points, P, obj["Jitter"])
        mean[info != 0] = np.nan
        var[info != 0] = np.nan
    else:
        return None
    with np.errstate(invalid="ignore"):
        sd = np.sqrt(var)
    return {"Points": P, "Weights": weights, "Mean": mean, "StandardDeviation": sd}


def predictJointFromSparseGaussianProcess(obj, pts, theta):
    """Joint form of predictFromSparseGaussianProcess(obj, pts, theta) for one theta: duplicates in pts are removed first (as
    predictJointFromGaussianProcess does), then {"Points" [M,d], "Mean" [M], "Covariance" [M,M]} -- the MultinormalDistribution
    of noisy observations at the points under the sparse posterior, whose diagonal is the per-point variance of
    predictFromSparseGaussianProcess.  None where the object is not a sparse GP object, on bad points or a theta whose fit fails."""
    if not isinstance(obj, inferenceObject) or obj.failed or "SparseGaussianProcessData" not in obj:
        return None
    P = dataNormalForm(pts)
    if P is None or isinstance(P, tuple):
        return None
    if any(f is not None for f in _sparse_pointwise_functions(obj)):
        raise ValueError("no joint prediction from a sparse GP object with a point-dependent nugget or mean function")
    _, first = np.unique(P, axis=0, return_index=True)
    P = P[np.sort(first)]
    handle = obj["SparseGaussianProcessData"]["HIPHandle"]
    if handle.fit(np.asarray(theta, dtype=np.float64).ravel(), obj["Jitter"]) != 0:
        return None
    mean, cov = handle.predict_cov(P, latent=False)
    return {"Points": P, "Mean": mean, "Covariance": cov}


def predictGradientFromSparseGaussianProcess(obj, pts, theta=None):
    """predictGradientFromGaussianProcess for a sparse object (gphip_sparse_predict_grad): for one theta the direct form's dict,
    or (theta=None) the per-sample arrays of a sampled object with "Weights", from a host loop of fit + predict_grad.  None
    where the object is not a sparse GP object (or unsampled without a theta), on bad points, a theta whose fit fails, and for
    objects with a callable nugget or mean function."""
    if not isinstance(obj, inferenceObject) or obj.failed or "SparseGaussianProcessData" not in obj:
        return None
    if any(f is not None for f in _sparse_pointwise_functions(obj)):
        return None
    P = dataNormalForm(pts)
    if P is None or isinstance(P, tuple):
        return None
    handle = obj["SparseGaussianProcessData"]["HIPHandle"]
    fit = lambda th: handle.fit(np.asarray(th, dtype=np.float64).ravel(), obj["Jitter"])       # noqa: E731
    if theta is not None:
        out = _predict_grad_samples(fit, handle.predict_grad, np.atleast_2d(np.asarray(theta, dtype=np.float64))[:1], np.ones(1), P)
        if not np.all(np.isfinite(out["Mean"][0])):
            return None
        return {"Points": P, "Mean": out["Mean"][0], "StandardDeviation": out["StandardDeviation"][0],
                "MeanGradient": out["MeanGradient"][0], "VarianceGradient": out["VarianceGradient"][0]}
    if "Samples" not in obj:
        return None
    points = np.array([s["Point"] for s in obj["Samples"]], dtype=np.float64)
    weights = np.array([s["CrudePosteriorWeight"] for s in obj["Samples"]], dtype=np.float64)
    return _predict_grad_samples(fit, handle.predict_grad, points, weights, P)


def sparsePredictiveLogDensity(obj, heldout, theta):
    """log N(ys | mean, Covariance) of held-out data heldout = (Xs, ys) under the sparse posterior of obj at theta: the joint
    predictive log density (the correlations between the held-out points included).  None where the object is not a sparse GP
    object, on bad data or a failed fit / factorisation."""
    if not isinstance(obj, inferenceObject) or obj.failed or "SparseGaussianProcessData" not in obj:
        return None
    P = dataNormalForm(heldout[0])
    if P is None or isinstance(P, tuple):
        return None
    ys = np.asarray(heldout[1], dtype=np.float64).ravel()
    if ys.shape != (len(P),):
        return None
    if any(f is not None for f in _sparse_pointwise_functions(obj)):
        raise ValueError("no joint predictive density from a sparse GP object with a point-dependent nugget or mean function")
    handle = obj["SparseGaussianProcessData"]["HIPHandle"]
    if handle.fit(np.asarray(theta, dtype=np.float64).ravel(), obj["Jitter"]) != 0:
        return None
    value, info = handle.predict_logpdf(P, ys)
    return value if info == 0 else None


def samplePathsFromSparseGaussianProcess(obj, n: int, theta=None, Features: int = 1024, seed: int = 0):
    """samplePathsFromGaussianProcess for a sparse object (gphip_sparse_paths_create): n pathwise draws of the latent posterior
    function under the collapsed bound's optimal q(u), which can be evaluated and differentiated after they have been drawn, at
    a cost per point that does not depend on the number of data points.  Two forms:
      samplePathsFromSparseGaussianProcess(obj, n, theta)   one fit at theta and one paths object of n draws under `seed`;
      samplePathsFromSparseGaussianProcess(obj, n)          a sampled object: every draw picks a theta from "Samples" by
          CrudePosteriorWeight with the assignment and the per-theta keys of samplePathsFromGaussianProcess, one fit and one
          paths object per distinct theta used.
    Every fit uses obj["Jitter"].  The paths objects live on the object's own "HIPHandle": until the result's close() (or the end
    of its `with` block) that handle cannot be closed or given another number of inducing points, and it is left fitted at the
    last theta used here.  Returns a posteriorFunctionSamples (values in the units of the data, gradients scaled accordingly),
    or None for a non-sparse or failed object, an unsampled object without theta, bad arguments, point-dependent nugget / mean
    functions and a run-time compiled kernel."""
    if not isinstance(obj, inferenceObject) or obj.failed or "SparseGaussianProcessData" not in obj:
        return None
    if int(n) < 1 or int(Features) < 1:
        return None
    if any(f is not None for f in _sparse_pointwise_functions(obj)):
        return None
    handle = obj["SparseGaussianProcessData"]["HIPHandle"]
    if isinstance(handle.kernel, _lib.CustomKernel):
        return None
    inverse, scale = _output_scale(obj)
    if theta is not None:
        if handle.fit(np.asarray(theta, dtype=np.float64).ravel(), obj["Jitter"]) != 0:
            return None
        paths = handle.sample_paths(int(n), int(Features), int(seed))
        if paths is None:
            return None
        return posteriorFunctionSamples([(np.arange(int(n)), paths)], n, handle.d, inverse, scale)
    if "Samples" not in obj:
        return None
    samples = obj["Samples"]
    points = np.array([s["Point"] for s in samples], dtype=np.float64)
    w = np.array([s["CrudePosteriorWeight"] for s in samples], dtype=np.float64)
    which = np.random.default_rng(seed).choice(len(samples), size=int(n), p=w / w.sum())
    parts = []
    for k in np.unique(which):
        rows = np.flatnonzero(which == k)
        if handle.fit(points[k], obj["Jitter"]) != 0:
            continue
        key = int(np.random.SeedSequence([int(seed) & (2**63 - 1), int(k)]).generate_state(1, np.uint64)[0])
        paths = handle.sample_paths(len(rows), int(Features), key)
        if paths is not None:
            parts.append((rows, paths))
    res = posteriorFunctionSamples(parts, n, handle.d, inverse, scale)
    res.sample = which
    return res


def thompsonSampleFromSparseGaussianProcess(obj, n: int, bounds, theta=None, Features: int = 1024, seed: int = 0, **maximize_options):
    """thompsonSampleFromGaussianProcess for a sparse object: n pathwise draws (samplePathsFromSparseGaussianProcess, both forms)
    and the maximiser of each over the box `bounds` (posteriorFunctionSamples.maximize(bounds, seed=seed, **maximize_options));
    the draws are released before it returns.  {"x" [n, d], "f" [n], "sample" [n]} in data units, or None wherever
    samplePathsFromSparseGaussianProcess returns None."""
    draws = samplePathsFromSparseGaussianProcess(obj, n, theta, Features, seed)
    if draws is None:
        return None
    with draws:
        best = draws.maximize(bounds, seed=seed, **maximize_options)
        return {"x": best["x"], "f": best["f"], "sample": np.array(draws.sample)}
