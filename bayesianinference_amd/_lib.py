"""ctypes binding of the C ABI in include/gphip.h (the drop-in boundary).

The library is the product: there is no CPU fallback.  If `libgphip.so` is missing or no gfx950
device is visible, every compute entry point raises `GphipError` loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "lib", "libgphip.so")
if os.environ.get("GPHIP_LIB"):        # developer A/B runs: another BUILD of the same HIP library (scripts/ab_build.py)
    LIB_PATH = os.environ["GPHIP_LIB"]
HEADER = os.path.join(os.path.dirname(PKG), "include", "gphip.h")

OK = 0
INFO_OK, INFO_NOT_SPD, INFO_NAN = 0, 1, 2
KERNEL_IDS = {"se": 0, "se_ard": 1, "matern52": 2, "matern52_ard": 3, "null": 4, "matern32": 5, "matern32_ard": 6,
              "rq": 7, "rq_ard": 8}
_OPS = {"+": 1, "*": 2}


def kernel_id(name: str) -> int:
    """Named kernel or a composed form -> the integer of include/gphip.h.  Grammar (spaces ignored):
        term [(+|*) term] [+const]      term in se, se_ard, matern52, matern52_ard, matern32, matern32_ard, rq, rq_ard
    e.g. "se+const" (the reference's own example, BGP:16), "se_ard+matern32", "rq*se_ard+const".  theta layout:
    [term 1: l.., (alpha), sf] [term 2: l.., (alpha), sf] [c] sn [mu]."""
    key = name.replace(" ", "").lower()
    if key in KERNEL_IDS:
        return KERNEL_IDS[key]
    offset = 0
    if key.endswith("+const"):
        key, offset = key[:-len("+const")], 1
    for sym, op in _OPS.items():
        if sym in key:
            a, b = key.split(sym, 1)
            break
    else:
        a, b, op = key, None, 0
    if a not in KERNEL_IDS or a == "null" or (b is not None and (b not in KERNEL_IDS or b == "null")):
        raise GphipError(1, f"unknown kernel {name!r}")
    return KERNEL_IDS[a] | ((KERNEL_IDS[b] if b else 0) << 8) | (op << 16) | (offset << 20) | (1 << 24)

MEAN_IDS = {"zero": 0, "const": 1}
PROFILE_CLASSES = ("kbuild", "potrf", "trsm", "gemm_panel", "syrk_trailing", "eval_total", "predict_epilogue")
COMM_ID_BYTES = 128

_STATUS = {1: "bad argument", 2: "dimension mismatch", 3: "HIP runtime failure",
           4: "handle not fitted", 5: "no gfx950 device", 6: "unsupported"}


class GphipError(RuntimeError):
    def __init__(self, status: int, msg: str = ""):
        self.status = status
        super().__init__(f"gphip status {status} ({_STATUS.get(status, '?')}): {msg}")


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_h = C.c_void_p

_SIGNATURES = {
    "gphip_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                               _ip, C.c_int, C.POINTER(_h)]),
    "gphip_create_custom": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                      C.POINTER(_h)]),
    "gphip_create_custom_devices": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_char_p, C.c_int, C.c_int, C.c_int, _ip, C.c_int,
                                              C.POINTER(_h)]),
    "gphip_create_custom_rank": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_void_p, C.POINTER(_h)]),
    "gphip_create_error": (C.c_char_p, []),
    "gphip_custom_compile": (C.c_int, [C.c_char_p, C.c_int, C.c_char_p, C.c_int, _ip]),
    "gphip_custom_compile_d": (C.c_int, [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, _ip]),
    "gphip_kernel_parse": (C.c_int, [C.c_char_p, C.c_int64, _ip]),
    "gphip_cform_to_body": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int64]),
    "gphip_tab_prior_sample": (C.c_int, [_dp, _dp, C.c_int, C.c_int64, C.c_int, C.c_uint64, _dp]),
    "gphip_comm_unique_id": (C.c_int, [C.c_void_p]),
    "gphip_create_rank": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(_h)]),
    "gphip_comm_info": (C.c_int, [_h, _ip, _ip, C.POINTER(C.c_char_p)]),
    "gphip_destroy": (C.c_int, [_h]),
    "gphip_num_params": (C.c_int, [_h, _ip]),
    "gphip_loglik": (C.c_int, [_h, _dp, C.c_int, _dp, _ip]),
    "gphip_loglik_batch": (C.c_int, [_h, _dp, C.c_int, C.c_int, _dp, _ip]),
    "gphip_loglik_parts": (C.c_int, [_h, _dp, C.c_int, _dp, _dp, _ip]),
    "gphip_loglik_grad": (C.c_int, [_h, _dp, C.c_int, _dp, _dp, _ip]),
    "gphip_loglik_grad_batch": (C.c_int, [_h, _dp, C.c_int, C.c_int, _dp, _dp, _ip]),
    "gphip_loo": (C.c_int, [_h, _dp, C.c_int, _dp, _dp, _dp, _dp, _ip]),
    "gphip_loo_grad": (C.c_int, [_h, _dp, C.c_int, _dp, _dp, _ip]),
    "gphip_fit": (C.c_int, [_h, _dp, C.c_int, _ip]),
    "gphip_predict": (C.c_int, [_h, C.c_void_p, C.c_int64, _dp, _dp]),
    "gphip_predict_samples": (C.c_int, [_h, _dp, C.c_int, C.c_int, C.c_void_p, C.c_int64, _dp, _dp, _ip]),
    "gphip_predict_cov": (C.c_int, [_h, C.c_void_p, C.c_int64, C.c_int, _dp, _dp]),
    "gphip_predict_draws": (C.c_int, [_h, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_uint64, _dp, C.c_double, _dp, _ip]),
    "gphip_predict_logpdf": (C.c_int, [_h, C.c_void_p, C.c_int64, _dp, _dp, _ip]),
    "gphip_extend": (C.c_int, [_h, C.c_void_p, _dp, C.c_int64, C.POINTER(_h), _dp, _ip]),
    "gphip_predict_grad": (C.c_int, [_h, C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp]),
    "gphip_rff_table": (C.c_int, [C.c_int, C.c_int64, _dp, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_int64), _dp, _dp, _dp]),
    "gphip_paths_create": (C.c_int, [_h, C.c_int, C.c_int, C.c_uint64, C.POINTER(_h), _ip]),
    "gphip_paths_eval": (C.c_int, [_h, C.c_void_p, C.c_int64, _dp, _dp]),
    "gphip_paths_eval_own": (C.c_int, [_h, C.c_void_p, C.c_int64, _dp, _dp]),
    "gphip_paths_shape": (C.c_int, [_h, _ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "gphip_paths_get": (C.c_int, [_h, _dp, _dp, _dp, _dp, _dp]),
    "gphip_paths_destroy": (C.c_int, [_h]),
    "gphip_paths_create_samples": (C.c_int, [_h, _dp, C.c_int, C.c_int, _ip, C.POINTER(C.c_uint64), C.c_int, C.POINTER(_h), _ip]),
    "gphip_paths_rows": (C.c_int, [_h, _ip, _ip]),
    "gphip_paths_get_table": (C.c_int, [_h, C.c_int, _dp, _dp, _dp]),
    "gphip_loglik_batch_pw": (C.c_int, [_h, _dp, C.c_int, C.c_int, _dp, _dp, _dp, _ip]),
    "gphip_fit_pw": (C.c_int, [_h, _dp, C.c_int, _dp, _dp, _ip]),
    "gphip_predict_pw": (C.c_int, [_h, C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp]),
    "gphip_predict_samples_pw": (C.c_int, [_h, _dp, C.c_int, C.c_int, _dp, _dp, C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp, _ip]),
    "gphip_covariance": (C.c_int, [_h, _dp, C.c_int, _dp]),
    "gphip_covariance_batch": (C.c_int, [_h, _dp, C.c_int, C.c_int, _dp]),
    "gphip_cross_covariance": (C.c_int, [_h, _dp, C.c_int, C.c_void_p, C.c_int64, _dp, _dp]),
    "gphip_solve": (C.c_int, [_h, _dp, C.c_int64, _dp]),
    "gphip_logdet": (C.c_int, [_h, _dp]),
    "gphip_set_option": (C.c_int, [_h, C.c_char_p, C.c_double]),
    "gphip_get_option": (C.c_int, [_h, C.c_char_p, C.POINTER(C.c_double)]),
    "gphip_get_profile": (C.c_int, [_h, C.c_int, _dp, _dp, _dp, _dp]),
    "gphip_reset_profile": (C.c_int, [_h]),
    "gphip_sync": (C.c_int, [_h]),
    "gphip_ns_default_options": (C.c_int, [C.c_void_p]),
    "gphip_nested_sampling": (C.c_int, [_h, _dp, _ip, C.c_void_p, C.c_void_p, C.c_void_p, _dp, C.c_int64, _dp, _dp, _dp, _dp,
                                        C.POINTER(C.c_int64), _dp, C.POINTER(C.c_int64)]),
    "gphip_ns_crude_weights": (C.c_int, [_dp, _dp, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), _dp, _dp, _dp]),
    "gphip_factor_bytes": (C.c_int, [_h, C.c_int, _dp]),
    "gphip_factor_get": (C.c_int, [_h, _dp, _dp, _dp]),
    "gphip_set_streams": (C.c_int, [_h, C.c_void_p, C.c_void_p]),
    "gphip_dist_num_panels": (C.c_int, [_h, _ip]),
    "gphip_dist_panel_shape": (C.c_int, [_h, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "gphip_dist_begin": (C.c_int, [_h, _dp, C.c_int, C.c_int, C.c_int]),
    "gphip_dist_factor_panel": (C.c_int, [_h, C.c_int, C.c_void_p]),
    "gphip_dist_update": (C.c_int, [_h, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "gphip_dist_end": (C.c_int, [_h, _dp, _dp, _ip]),
    "gphip_sparse_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.POINTER(_h)]),
    "gphip_sparse_create_custom": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_char_p, C.c_int,
                                             C.c_int, C.c_int, C.c_int, C.POINTER(_h)]),
    "gphip_sparse_destroy": (C.c_int, [_h]),
    "gphip_sparse_set_inducing": (C.c_int, [_h, C.c_void_p, C.c_int64]),
    "gphip_sparse_num_params": (C.c_int, [_h, _ip]),
    "gphip_sparse_bound": (C.c_int, [_h, _dp, C.c_int, C.c_double, _dp, _dp, _ip]),
    "gphip_sparse_bound_batch": (C.c_int, [_h, _dp, C.c_int, C.c_int, C.c_double, _dp, _dp, _ip]),
    "gphip_sparse_nested_sampling": (C.c_int, [_h, C.c_double, _dp, _ip, C.c_void_p, C.c_void_p, C.c_void_p, _dp, C.c_int64, _dp, _dp, _dp,
                                               _dp, C.POINTER(C.c_int64), _dp, C.POINTER(C.c_int64)]),
    "gphip_sparse_bound_grad": (C.c_int, [_h, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _ip]),
    "gphip_sparse_bound_grad_inducing": (C.c_int, [_h, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _ip]),
    "gphip_sparse_fit": (C.c_int, [_h, _dp, C.c_int, C.c_double, _ip]),
    "gphip_sparse_predict": (C.c_int, [_h, C.c_void_p, C.c_int64, C.c_int, _dp, _dp]),
    "gphip_sparse_predict_grad": (C.c_int, [_h, C.c_void_p, C.c_int64, _dp, _dp, _dp, _dp]),
    "gphip_sparse_predict_samples": (C.c_int, [_h, _dp, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_int64, C.c_int, _dp, _dp, _dp, _ip]),
    "gphip_sparse_bound_pw": (C.c_int, [_h, _dp, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _ip]),
    "gphip_sparse_bound_batch_pw": (C.c_int, [_h, _dp, C.c_int, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _ip]),
    "gphip_sparse_fit_pw": (C.c_int, [_h, _dp, C.c_int, C.c_double, _dp, _dp, _ip]),
    "gphip_sparse_predict_pw": (C.c_int, [_h, C.c_void_p, C.c_int64, C.c_int, _dp, _dp, _dp, _dp]),
    "gphip_sparse_predict_samples_pw": (C.c_int, [_h, _dp, C.c_int, C.c_int, C.c_double, _dp, _dp, C.c_void_p, C.c_int64, C.c_int, _dp, _dp,
                                                  _dp, _dp, _dp, _ip]),
    "gphip_sparse_predict_cov": (C.c_int, [_h, C.c_void_p, C.c_int64, C.c_int, _dp, _dp]),
    "gphip_sparse_predict_draws": (C.c_int, [_h, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_uint64, _dp, C.c_double, _dp, _ip]),
    "gphip_sparse_predict_logpdf": (C.c_int, [_h, C.c_void_p, C.c_int64, _dp, _dp, _ip]),
    "gphip_sparse_set_option": (C.c_int, [_h, C.c_char_p, C.c_double]),
    "gphip_sparse_get_option": (C.c_int, [_h, C.c_char_p, C.POINTER(C.c_double)]),
    "gphip_sparse_last_error": (C.c_char_p, [_h]),
    "gphip_sparse_paths_create": (C.c_int, [_h, C.c_int, C.c_int, C.c_uint64, C.POINTER(_h), _ip]),
    "gphip_sparse_paths_get": (C.c_int, [_h, _dp, _dp]),
    "gphip_last_error": (C.c_char_p, [_h]),
    "gphip_version": (C.c_char_p, []),
    "gphip_device_count": (C.c_int, [_ip]),
}

_lib = None


def declared_symbols() -> list[str]:
    """Every function name include/gphip.h declares (used by the symbol-export test)."""
    with open(HEADER) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gphip_[a-z_]+)\s*\(", text)))


def load():
    """dlopen the in-tree library (built by `python -m bayesianinference_amd.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GphipError(3, f"{LIB_PATH} is missing -- run `python -m bayesianinference_amd.build` "
                            "(hipcc, gfx950).  There is no CPU fallback.")
    # PyTorch-ROCm wheels bundle their own libamdhip64/libhsa-runtime64.  A process must end up with
    # ONE HIP runtime, or torch later reports "No HIP GPUs are available" and torch streams cannot be
    # handed to this library (dist_cholesky.py).  Importing torch first makes the dynamic loader
    # resolve libgphip's libamdhip64.so.7 dependency to the copy torch already mapped.
    if os.environ.get("GPHIP_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        if os.environ.get("GPHIP_LIB") and not hasattr(lib, name):
            continue                                   # developer A/B against an OLDER build of the library
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def device_count() -> int:
    n = C.c_int(0)
    load().gphip_device_count(C.byref(n))
    return n.value


def comm_unique_id() -> bytes:
    """RCCL unique id (rank 0 creates it, the host distributes it to every rank: gphip_create_rank)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load().gphip_comm_unique_id(buf)
    if rc != OK:
        raise GphipError(rc, "gphip_comm_unique_id: no RCCL could be bound (set GPHIP_RCCL_PATH)")
    return buf.raw


def _d(a: np.ndarray):
    return a.ctypes.data_as(_dp)


class NsOptions(C.Structure):
    """gphip_ns_options (include/gphip.h)"""
    _fields_ = [("pool", C.c_int), ("max_iterations", C.c_int), ("min_iterations", C.c_int), ("mc_steps", C.c_int),
                ("walkers", C.c_int), ("termination_fraction", C.c_double), ("min_accept", C.c_double),
                ("max_accept", C.c_double), ("seed", C.c_uint64)]


LOGPRIOR_FN = C.CFUNCTYPE(C.c_double, _dp, C.c_int, C.c_void_p)


def ns_crude_weights(points, loglik, pool: int):
    """gphip_ns_crude_weights: (order, logX, crude log weights, log evidence) -- calculateWeightsCrude, BS:818-835."""
    pts = np.ascontiguousarray(np.atleast_2d(np.asarray(points, dtype=np.float64)))
    ll = np.ascontiguousarray(np.asarray(loglik, dtype=np.float64))
    m, p = pts.shape
    order = np.zeros(m, dtype=np.int64)
    logx, logw, z = np.zeros(m), np.zeros(m), C.c_double(0.0)
    rc = load().gphip_ns_crude_weights(_d(pts), _d(ll), m, p, int(pool), order.ctypes.data_as(C.POINTER(C.c_int64)), _d(logx),
                                       _d(logw), C.byref(z))
    if rc != OK:
        raise GphipError(rc, "gphip_ns_crude_weights")
    return order, logx, logw, z.value


def num_params(kernel, d: int, mean: str) -> int:
    """Length of theta for a kernel (a name of the grammar or a CustomKernel) on d dimensions with the mean "zero" / "const":
    the kernel's parameters, sigma_n and, for the constant mean, mu.  Host logic (gphip_kernel_parse): no device is touched."""
    if isinstance(kernel, CustomKernel):
        count = kernel.nparams
    else:
        spec = (C.c_int * 8)()
        if load().gphip_kernel_parse(str(kernel).encode(), int(d), spec) != OK:
            raise GphipError(1, f"{kernel!r} is not a kernel of the library")
        count = spec[7]                                # the 0-based position of sigma_n
    return count + 1 + (1 if mean == "const" else 0)


class CustomKernel:
    """ANY covariance function k(x, x'; p) for the device (the reference takes any `kernel @@ points[[{i,j}]]`, BGP:29-33):
    `body` = C++ statements in X(k), Y(k) (coordinates of the two points), P(k) (hyper-parameters), D (dimension), T (the
    arithmetic type) that `return` the covariance without the nugget -- see gphip_create_custom in include/gphip.h;
    theta of such a handle = [p_0 .. p_{nparams-1}, sn (, mu)].  `fn(A, B, p)` (optional) = the same function in numpy on
    broadcastable point arrays [.., d] -- what the CPU oracle evaluates in the tests."""

    def __init__(self, body: str, nparams: int, fn=None, name: str = "custom"):
        self.body, self.nparams, self.fn, self.name = str(body), int(nparams), fn, name

    def __repr__(self):
        return f"CustomKernel({self.name!r}, nparams={self.nparams})"


def rff_table(kernel, d: int, theta, F: int, seed: int = 0):
    """gphip_rff_table (host only): (omega[Ftot, d], phase[Ftot], amp[Ftot]) of a named kernel (a name or an id) at theta."""
    lib = load()
    kid = kernel if isinstance(kernel, int) else kernel_id(kernel)
    th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
    ftot = C.c_int64(0)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    rc = lib.gphip_rff_table(kid, int(d), _d(th), th.size, int(F), seed, C.byref(ftot), None, None, None)
    if rc != OK:
        raise GphipError(rc, "gphip_rff_table: no feature table for this kernel, theta or F")
    omega, phase, amp = np.zeros((ftot.value, int(d))), np.zeros(ftot.value), np.zeros(ftot.value)
    rc = lib.gphip_rff_table(kid, int(d), _d(th), th.size, int(F), seed, C.byref(ftot), _d(omega), _d(phase), _d(amp))
    if rc != OK:
        raise GphipError(rc, "gphip_rff_table: no feature table for this kernel, theta or F")
    return omega, phase, amp


class Paths:
    """Owns one gphip_paths_handle (Handle.sample_paths, SparseHandle.sample_paths): S coherent draws of the latent posterior
    function.  Keeps its parent handle alive; close() it (or leave the with block) before the parent is closed.  On a sparse
    parent N reads m, the contraction points are Z and the error text comes from the sparse object."""

    def __init__(self, parent, h):
        self._parent, self._lib, self._q = parent, parent._lib, h
        self._sparse = isinstance(parent, SparseHandle)
        S, ftot, n, d = C.c_int(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._lib.gphip_paths_shape(self._q, C.byref(S), C.byref(ftot), C.byref(n), C.byref(d))
        self.S, self.Ftot, self.N, self.d = S.value, ftot.value, n.value, d.value

    def _check(self, rc: int):
        if rc != OK:
            last = self._lib.gphip_sparse_last_error if getattr(self, "_sparse", False) else self._lib.gphip_last_error
            raise GphipError(rc, (last(self._parent._h) or b"").decode())

    def eval(self, Xs, grad: bool = False):
        """f_s(Xs): out[S, M]; grad=True: (out, dout[S, M, d]) with dout[s, t, c] = df_s/dx_tc.  out is the same bytes either way."""
        Xs = self._parent._test_points(Xs)
        M = Xs.shape[0]
        out = np.zeros((self.S, M))
        dout = np.zeros((self.S, M, self.d)) if grad else None
        self._check(self._lib.gphip_paths_eval(self._q, Xs.ctypes.data, M, _d(out), _d(dout) if grad else None))
        return (out, dout) if grad else out

    def eval_own(self, Xs, grad: bool = False):
        """gphip_paths_eval_own: every draw at its own points.  Xs[S, M, d] -> out[S, M] with out[s, t] = f_s(Xs[s, t]); grad=True:
        (out, dout[S, M, d]).  out is the same bytes either way.  A wrong shape raises ValueError before any library call."""
        Xs = np.ascontiguousarray(np.asarray(Xs, dtype=np.float64))
        if Xs.ndim != 3 or Xs.shape[0] != self.S or Xs.shape[1] < 1 or Xs.shape[2] != self.d:
            raise ValueError("Xs must have shape [%d, M, %d] with M >= 1, got %s" % (self.S, self.d, list(Xs.shape)))
        M = Xs.shape[1]
        out = np.zeros((self.S, M))
        dout = np.zeros((self.S, M, self.d)) if grad else None
        self._check(self._lib.gphip_paths_eval_own(self._q, Xs.ctypes.data, M, _d(out), _d(dout) if grad else None))
        return (out, dout) if grad else out

    def rows(self):
        """gphip_paths_rows: (R, row_of_draw [S]) -- the hyper-parameter rows of the object and the row each draw belongs to; an
        ordinary object has R = 1."""
        R, row_of = C.c_int(0), np.zeros(self.S, dtype=np.int32)
        self._check(self._lib.gphip_paths_rows(self._q, C.byref(R), row_of.ctypes.data_as(_ip)))
        return R.value, row_of

    def table(self, r=None):
        """{"omega" [Ftot, d], "phase" [Ftot], "w" [S, Ftot], "eps" [S, N], "v" [S, N]}: what the draws were made from.  A sparse
        parent: N = m, "eps" = sqrt(jitter) zeta, and the unit normals "xi" [S, m] and "zeta" [S, m] as well.
        r given: row r's {"omega", "phase", "amp" [Ftot]} (gphip_paths_get_table).  r=None on a mixture object (Handle.
        sample_paths_samples): "w", "eps" and "v" only -- the tables are per row."""
        if r is not None:
            t = {"omega": np.zeros((self.Ftot, self.d)), "phase": np.zeros(self.Ftot), "amp": np.zeros(self.Ftot)}
            self._check(self._lib.gphip_paths_get_table(self._q, int(r), _d(t["omega"]), _d(t["phase"]), _d(t["amp"])))
            return t
        t = {"omega": np.zeros((self.Ftot, self.d)), "phase": np.zeros(self.Ftot), "w": np.zeros((self.S, self.Ftot)),
             "eps": np.zeros((self.S, self.N)), "v": np.zeros((self.S, self.N))}
        if getattr(self, "info", None) is not None:                  # a mixture object: Handle.sample_paths_samples sets .info [R]
            del t["omega"], t["phase"]
            self._check(self._lib.gphip_paths_get(self._q, None, None, _d(t["w"]), _d(t["eps"]), _d(t["v"])))
            return t
        self._check(self._lib.gphip_paths_get(self._q, _d(t["omega"]), _d(t["phase"]), _d(t["w"]), _d(t["eps"]), _d(t["v"])))
        if getattr(self, "_sparse", False):
            t["xi"], t["zeta"] = np.zeros((self.S, self.N)), np.zeros((self.S, self.N))
            self._check(self._lib.gphip_sparse_paths_get(self._q, _d(t["xi"]), _d(t["zeta"])))
        return t

    def close(self):
        if getattr(self, "_q", None):
            self._lib.gphip_paths_destroy(self._q)
            self._q = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Handle:
    """Owns one gphip_handle: training data resident on the device (gphip_create .. gphip_destroy)."""

    def __init__(self, X, y, kernel="se_ard", mean: str = "zero", dtype: int = 64, device=None,
                 rank=None, world=None, comm_id: bytes | None = None):
        """device: None (current device), one ordinal, or a LIST of ordinals = one multi-device handle in this
        process (a repeated ordinal = virtual ranks sharing a GPU).  rank/world/comm_id: this process is one
        rank of a multi-process job (gphip_create_rank; comm_id from comm_unique_id() of rank 0).
        kernel: a name of the grammar of kernel_id(), or a CustomKernel (ANY covariance function, given as the source text of
        its body: compiled at run time into the library's kernel build, gphip_create_custom)."""
        lib = load()
        if isinstance(kernel, CustomKernel):
            self._init_custom(lib, X, y, kernel, mean, dtype, device, rank, world, comm_id)
            return
        X = np.ascontiguousarray(np.atleast_2d(np.asarray(X, dtype=np.float64)))
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).ravel())
        if X.shape[0] != y.shape[0]:
            raise GphipError(2, "Input and output data are not of same length")     # BGP:251-253
        if mean not in MEAN_IDS:
            raise GphipError(1, f"unknown mean {mean!r}")
        kid = kernel_id(kernel)
        self.N, self.d = X.shape
        self.kernel, self.mean, self.dtype = kernel, mean, int(dtype)
        self._lib = lib
        self._h = _h()
        devs, nd = (None, 0)
        if device is not None:
            lst = [int(v) for v in device] if isinstance(device, (list, tuple)) else [int(device)]
            devs, nd = (C.c_int * len(lst))(*lst), len(lst)
        if comm_id is not None:
            if rank is None or world is None or len(comm_id) != COMM_ID_BYTES:
                raise GphipError(1, "rank, world and a 128-byte comm_id go together")
            rc = lib.gphip_create_rank(X.ctypes.data, y.ctypes.data, self.N, self.d, kid, MEAN_IDS[mean],
                                       dtype, -1 if device is None else int(devs[0]), int(rank), int(world),
                                       C.c_char_p(comm_id), C.byref(self._h))
        else:
            rc = lib.gphip_create(X.ctypes.data, y.ctypes.data, self.N, self.d, kid,
                                  MEAN_IDS[mean], dtype, devs, nd, C.byref(self._h))
        if rc != OK:
            self._h = None
            why = {5: "no gfx950 GPU visible, or a device ordinal that does not exist",
                   6: "unsupported combination (null kernel on a multi-device handle, d > 32, dtype other than 64 / 32, or no "
                      "RCCL could be bound for a multi-process handle: set GPHIP_RCCL_PATH)",
                   1: "bad argument (unknown kernel / mean id, rank outside the world)",
                   2: "bad shape (N < 1 or d < 1)"}.get(rc, "is a gfx950 GPU visible?")
            raise GphipError(rc, "gphip_create failed: " + why)
        p = C.c_int(0)
        lib.gphip_num_params(self._h, C.byref(p))
        self.p = p.value

    def _init_custom(self, lib, X, y, kernel, mean, dtype, device, rank=None, world=None, comm_id=None):
        X = np.ascontiguousarray(np.atleast_2d(np.asarray(X, dtype=np.float64)))
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).ravel())
        if X.shape[0] != y.shape[0]:
            raise GphipError(2, "Input and output data are not of same length")     # BGP:251-253
        if mean not in MEAN_IDS:
            raise GphipError(1, f"unknown mean {mean!r}")
        self.N, self.d = X.shape
        self.kernel, self.mean, self.dtype = kernel, mean, int(dtype)
        self._lib = lib
        self._h = _h()
        lst = [] if device is None else ([int(v) for v in device] if isinstance(device, (list, tuple)) else [int(device)])
        devs = (C.c_int * max(len(lst), 1))(*lst) if lst else None
        if comm_id is not None:
            if rank is None or world is None or len(comm_id) != COMM_ID_BYTES:
                raise GphipError(1, "rank, world and a 128-byte comm_id go together")
            rc = lib.gphip_create_custom_rank(X.ctypes.data, y.ctypes.data, self.N, self.d, kernel.body.encode(), int(kernel.nparams),
                                              MEAN_IDS[mean], dtype, lst[0] if lst else -1, int(rank), int(world),
                                              C.c_char_p(comm_id), C.byref(self._h))
        else:
            rc = lib.gphip_create_custom_devices(X.ctypes.data, y.ctypes.data, self.N, self.d, kernel.body.encode(), int(kernel.nparams),
                                                 MEAN_IDS[mean], dtype, devs, len(lst), C.byref(self._h))
        if rc != OK:
            self._h = None
            raise GphipError(rc, "gphip_create_custom failed: " + (lib.gphip_create_error() or b"").decode())
        p = C.c_int(0)
        lib.gphip_num_params(self._h, C.byref(p))
        self.p = p.value

    # -- helpers -------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != OK:
            raise GphipError(rc, (self._lib.gphip_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            if self._lib.gphip_destroy(self._h) == 4:        # live Paths objects: nothing was destroyed, the handle stays open
                raise GphipError(4, (self._lib.gphip_last_error(self._h) or b"").decode())
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name: str, value: float):
        self._check(self._lib.gphip_set_option(self._h, name.encode(), float(value)))

    def get_option(self, name: str) -> float:
        v = C.c_double()
        self._check(self._lib.gphip_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    # -- hot path ------------------------------------------------------------------------
    def loglik(self, theta):
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        out, info = C.c_double(0.0), C.c_int(0)
        self._check(self._lib.gphip_loglik(self._h, _d(th), th.size, C.byref(out), C.byref(info)))
        return out.value, info.value

    def loglik_parts(self, theta):
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        out, info = C.c_double(0.0), C.c_int(0)
        parts = np.zeros(2)
        self._check(self._lib.gphip_loglik_parts(self._h, _d(th), th.size, C.byref(out), _d(parts),
                                                 C.byref(info)))
        return out.value, parts[0], parts[1], info.value

    def loglik_batch(self, Theta):
        Th = np.ascontiguousarray(np.atleast_2d(np.asarray(Theta, dtype=np.float64)))
        B, p = Th.shape
        out = np.zeros(B)
        info = np.zeros(B, dtype=np.int32)
        self._check(self._lib.gphip_loglik_batch(self._h, _d(Th), B, p, _d(out), info.ctypes.data_as(_ip)))
        return out, info

    @staticmethod
    def _rows(a, rows: int, cols: int, what: str):
        """optional per-point array -> (contiguous float64 [rows, cols] or None, ctypes pointer or None)"""
        if a is None:
            return None, None
        arr = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(rows, -1))
        if arr.shape != (rows, cols):
            raise GphipError(2, f"{what} must have shape ({rows}, {cols})")
        return arr, _d(arr)

    def loglik_batch_pw(self, Theta, mean_train=None, nugget_train=None):
        """gphip_loglik_batch_pw: point-dependent mean m(x_i) / nugget nu(x_i) VALUES per theta, each [B, N] or None
        (BGP:37, 300: the host evaluates the functions, the device gets the values)."""
        Th = np.ascontiguousarray(np.atleast_2d(np.asarray(Theta, dtype=np.float64)))
        B, p = Th.shape
        mt, mtp = self._rows(mean_train, B, self.N, "mean_train")
        nt, ntp = self._rows(nugget_train, B, self.N, "nugget_train")
        out = np.zeros(B)
        info = np.zeros(B, dtype=np.int32)
        self._check(self._lib.gphip_loglik_batch_pw(self._h, _d(Th), B, p, mtp, ntp, _d(out), info.ctypes.data_as(_ip)))
        return out, info

    def fit_pw(self, theta, mean_train=None, nugget_train=None) -> int:
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        mt, mtp = self._rows(mean_train, 1, self.N, "mean_train")
        nt, ntp = self._rows(nugget_train, 1, self.N, "nugget_train")
        info = C.c_int(0)
        self._check(self._lib.gphip_fit_pw(self._h, _d(th), th.size, mtp, ntp, C.byref(info)))
        return info.value

    def predict_pw(self, Xs, mean_test=None, nugget_test=None):
        Xs = np.ascontiguousarray(np.atleast_2d(np.asarray(Xs, dtype=np.float64)))
        if Xs.shape[1] != self.d:
            raise GphipError(2, "test points have the wrong dimension")
        M = Xs.shape[0]
        ms, msp = self._rows(mean_test, 1, M, "mean_test")
        ns, nsp = self._rows(nugget_test, 1, M, "nugget_test")
        mean, var = np.zeros(M), np.zeros(M)
        self._check(self._lib.gphip_predict_pw(self._h, Xs.ctypes.data, M, msp, nsp, _d(mean), _d(var)))
        return mean, var

    def predict_samples_pw(self, Thetas, Xs, mean_train=None, nugget_train=None, mean_test=None, nugget_test=None):
        Th = np.ascontiguousarray(np.atleast_2d(np.asarray(Thetas, dtype=np.float64)))
        Xs = np.ascontiguousarray(np.atleast_2d(np.asarray(Xs, dtype=np.float64)))
        if Xs.shape[1] != self.d:
            raise GphipError(2, "test points have the wrong dimension")
        S, M = Th.shape[0], Xs.shape[0]
        mt, mtp = self._rows(mean_train, S, self.N, "mean_train")
        nt, ntp = self._rows(nugget_train, S, self.N, "nugget_train")
        ms, msp = self._rows(mean_test, S, M, "mean_test")
        ns, nsp = self._rows(nugget_test, S, M, "nugget_test")
        mean, var = np.zeros((S, M)), np.zeros((S, M))
        info = np.zeros(S, dtype=np.int32)
        self._check(self._lib.gphip_predict_samples_pw(self._h, _d(Th), S, Th.shape[1], mtp, ntp, Xs.ctypes.data, M, msp, nsp,
                                                       _d(mean), _d(var), info.ctypes.data_as(_ip)))
        return mean, var, info

    def loglik_grad(self, theta):
        """(loglik, grad[p], info)."""
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        out, info = C.c_double(0.0), C.c_int(0)
        grad = np.zeros(th.size)
        self._check(self._lib.gphip_loglik_grad(self._h, _d(th), th.size, C.byref(out), _d(grad), C.byref(info)))
        return out.value, grad, info.value

    def loglik_grad_batch(self, Theta):
        """gphip_loglik_grad_batch: (loglik[B], grad[B, p], info[B]) for the rows of Theta [B, p] (a 1-D theta is one row) in one
        call; a failing row has its own info and a NaN grad row.  Drops any resident fit."""
        Th = np.ascontiguousarray(np.atleast_2d(np.asarray(Theta, dtype=np.float64)))
        if Th.ndim != 2 or Th.shape[1] != self.p:
            raise GphipError(2, f"Theta has rows of {Th.shape[-1]} entries, the handle takes {self.p}")
        B, p = Th.shape
        out, grad = np.zeros(B), np.zeros((B, p))
        info = np.zeros(B, dtype=np.int32)
        self._check(self._lib.gphip_loglik_grad_batch(self._h, _d(Th), B, p, _d(out), _d(grad), info.ctypes.data_as(_ip)))
        return out, grad, info

    def _theta(self, theta):
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        if th.size != self.p:
            raise GphipError(2, f"theta has {th.size} entries, the handle takes {self.p}")
        return th

    def loo(self, theta, mean: bool = True, var: bool = True, logp: bool = True) -> dict:
        """Leave-one-out cross-validation at theta (gphip_loo): {"mean", "var", "logp"} (each [N], or None when not asked
        for), "total" = the log pseudo-likelihood, "info".  Leaves the fit of theta resident."""
        th = self._theta(theta)
        out, info = C.c_double(0.0), C.c_int(0)
        arrs = [np.zeros(self.N) if want else None for want in (mean, var, logp)]
        ptrs = [_d(a) if a is not None else None for a in arrs]
        self._check(self._lib.gphip_loo(self._h, _d(th), th.size, ptrs[0], ptrs[1], ptrs[2], C.byref(out), C.byref(info)))
        return {"mean": arrs[0], "var": arrs[1], "logp": arrs[2], "total": out.value, "info": info.value}

    def loo_grad(self, theta):
        """(log pseudo-likelihood, grad[p], info) from gphip_loo_grad; grad has the layout of loglik_grad's."""
        th = self._theta(theta)
        out, info = C.c_double(0.0), C.c_int(0)
        grad = np.zeros(th.size)
        self._check(self._lib.gphip_loo_grad(self._h, _d(th), th.size, C.byref(out), _d(grad), C.byref(info)))
        return out.value, grad, info.value

    def fit(self, theta) -> int:
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        info = C.c_int(0)
        self._check(self._lib.gphip_fit(self._h, _d(th), th.size, C.byref(info)))
        return info.value

    def predict(self, Xs):
        Xs = np.ascontiguousarray(np.atleast_2d(np.asarray(Xs, dtype=np.float64)))
        if Xs.shape[1] != self.d:
            raise GphipError(2, "test points have the wrong dimension")
        M = Xs.shape[0]
        mean, var = np.zeros(M), np.zeros(M)
        self._check(self._lib.gphip_predict(self._h, Xs.ctypes.data, M, _d(mean), _d(var)))
        return mean, var

    def predict_samples(self, Thetas, Xs):
        """All posterior samples in one batched pass: (mean[S,M], var[S,M], info[S])."""
        Th = np.ascontiguousarray(np.atleast_2d(np.asarray(Thetas, dtype=np.float64)))
        Xs = np.ascontiguousarray(np.atleast_2d(np.asarray(Xs, dtype=np.float64)))
        if Xs.shape[1] != self.d:
            raise GphipError(2, "test points have the wrong dimension")
        S, M = Th.shape[0], Xs.shape[0]
        mean, var = np.zeros((S, M)), np.zeros((S, M))
        info = np.zeros(S, dtype=np.int32)
        self._check(self._lib.gphip_predict_samples(self._h, _d(Th), S, Th.shape[1], Xs.ctypes.data, M,
                                                    _d(mean), _d(var), info.ctypes.data_as(_ip)))
        return mean, var, info

    def _test_points(self, Xs):
        Xs = np.ascontiguousarray(np.atleast_2d(np.asarray(Xs, dtype=np.float64)))
        if Xs.ndim != 2 or Xs.shape[1] != self.d:
            raise GphipError(2, "test points have the wrong dimension")
        if Xs.shape[0] < 1:
            raise GphipError(2, "M < 1")
        return Xs

    def predict_cov(self, Xs, latent: bool = False):
        """Joint predictive distribution at Xs[M, d]: (mean[M], cov[M, M]).  latent=False: covariance of noisy observations
        (its diagonal is predict()'s var); latent=True: of the latent function."""
        Xs = self._test_points(Xs)
        M = Xs.shape[0]
        mean, cov = np.zeros(M), np.zeros((M, M))
        self._check(self._lib.gphip_predict_cov(self._h, Xs.ctypes.data, M, int(bool(latent)), _d(mean), _d(cov)))
        return mean, cov

    def predict_draws(self, Xs, S: int, seed: int = 0, z=None, latent: bool = True, jitter: float = -1.0):
        """S draws from the joint predictive distribution: (out[S, M], info).  z: the caller's standard normals [S, M]
        (None: generated on the device from (seed, s, j)); jitter < 0: the library's default, 0: none."""
        Xs = self._test_points(Xs)
        M, S = Xs.shape[0], int(S)
        if S < 1:
            raise GphipError(2, "S < 1")
        zp = None
        if z is not None:
            z = np.ascontiguousarray(np.asarray(z, dtype=np.float64))
            if z.shape != (S, M):
                raise GphipError(2, f"z must have shape ({S}, {M})")
            zp = _d(z)
        if not np.isfinite(jitter):
            raise GphipError(1, "non-finite jitter")
        out = np.zeros((S, M))
        info = C.c_int(0)
        self._check(self._lib.gphip_predict_draws(self._h, Xs.ctypes.data, M, int(bool(latent)), S, int(seed) & (2**64 - 1), zp,
                                                  float(jitter), _d(out), C.byref(info)))
        return out, info.value

    def predict_logpdf(self, Xs, ystar):
        """log N(ystar | mean, cov) with the noisy-observation covariance at Xs: (value, info)."""
        Xs = self._test_points(Xs)
        M = Xs.shape[0]
        ys = np.ascontiguousarray(np.asarray(ystar, dtype=np.float64).ravel())
        if ys.shape != (M,):
            raise GphipError(2, f"ystar must have length {M}")
        out, info = C.c_double(0.0), C.c_int(0)
        self._check(self._lib.gphip_predict_logpdf(self._h, Xs.ctypes.data, M, _d(ys), C.byref(out), C.byref(info)))
        return out.value, info.value

    def extend(self, X_new, y_new):
        """gphip_extend: the observations (X_new[M, d], y_new[M]) into the resident fit without refactoring it.  Returns
        (Handle on the N + M points with the fit of the same theta resident, or None; log p(y_new | X_new, X, y, theta) -- the
        bytes of predict_logpdf(X_new, y_new); info).  info != 0 (Sigma not positive definite under the pivot rule, non-finite
        data): no handle, logp = NaN.  This handle is untouched; the new one is closed on its own."""
        Xn = self._test_points(X_new)
        M = Xn.shape[0]
        yn = np.ascontiguousarray(np.asarray(y_new, dtype=np.float64).ravel())
        if yn.shape != (M,):
            raise GphipError(2, f"y_new must have length {M}")
        out, logp, info = _h(), C.c_double(0.0), C.c_int(0)
        self._check(self._lib.gphip_extend(self._h, Xn.ctypes.data, _d(yn), M, C.byref(out), C.byref(logp), C.byref(info)))
        if not out.value:
            return None, logp.value, info.value
        new = Handle.__new__(Handle)
        new._lib, new._h = self._lib, out
        new.N, new.d = self.N + M, self.d
        new.kernel, new.mean, new.dtype, new.p = self.kernel, self.mean, self.dtype, self.p
        return new, logp.value, info.value

    def sample_paths(self, S: int, F: int = 1024, seed: int = 0):
        """gphip_paths_create: S pathwise draws of the latent posterior function of the resident fit, F random Fourier features
        per term.  Returns a Paths (close it before this handle), or None when v is not finite (info = GPHIP_INFO_NAN)."""
        out, info = _h(), C.c_int(0)
        self._check(self._lib.gphip_paths_create(self._h, int(S), int(F), int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(out), C.byref(info)))
        if not out.value:
            return None
        return Paths(self, out)

    def sample_paths_samples(self, Thetas, counts, seeds, F: int = 1024):
        """gphip_paths_create_samples: ONE mixture paths object over the rows of Thetas [R, p]; row r gives counts[r] draws (>= 0),
        draw q of row r being draw q of fit(Thetas[r]) + sample_paths(counts[r], F, seeds[r]).  The draws are ordered by row.  No
        fit stays resident.  Returns a Paths whose .info [R] holds the rows' verdicts (the draws of a failed row are NaN), or None
        when every row with draws failed; the verdicts are then in self.last_paths_info.  Wrong shapes raise ValueError before
        any library call."""
        Th = np.ascontiguousarray(np.asarray(Thetas, dtype=np.float64))
        if Th.ndim == 1:
            Th = Th.reshape(1, -1)
        cnt = np.ascontiguousarray(np.asarray(counts, dtype=np.int64).ravel())
        sd = np.ascontiguousarray(np.array([int(s) & 0xFFFFFFFFFFFFFFFF for s in np.ravel(np.asarray(seeds, dtype=object))], dtype=np.uint64))
        if Th.ndim != 2 or Th.shape[0] < 1 or Th.shape[1] != self.p:
            raise ValueError("Thetas must have shape [R, %d] with R >= 1, got %s" % (self.p, list(Th.shape)))
        R = Th.shape[0]
        if cnt.shape != (R,) or sd.shape != (R,):
            raise ValueError("counts and seeds must have %d entries each, got %d and %d" % (R, cnt.size, sd.size))
        if np.any(cnt < 0) or cnt.sum() < 1 or int(F) < 1:
            raise ValueError("counts must be >= 0 with at least one draw in all, and F >= 1")
        cnt = np.ascontiguousarray(cnt.astype(np.int32))
        out, info = _h(), np.zeros(R, dtype=np.int32)
        self.last_paths_info = info
        self._check(self._lib.gphip_paths_create_samples(self._h, _d(Th), R, Th.shape[1], cnt.ctypes.data_as(_ip),
                                                         sd.ctypes.data_as(C.POINTER(C.c_uint64)), int(F), C.byref(out),
                                                         info.ctypes.data_as(_ip)))
        if not out.value:
            return None
        paths = Paths(self, out)
        paths.info = info
        return paths

    def predict_grad(self, Xs, variance: bool = True):
        """Gradients of the prediction in the test inputs (gphip_predict_grad): (mean[M], var[M], dmean[M, d], dvar[M, d]);
        variance=False skips the backward substitution and returns dvar = None."""
        Xs = self._test_points(Xs)
        M = Xs.shape[0]
        mean, var, dmean = np.zeros(M), np.zeros(M), np.zeros((M, self.d))
        dvar = np.zeros((M, self.d)) if variance else None
        self._check(self._lib.gphip_predict_grad(self._h, Xs.ctypes.data, M, _d(mean), _d(var), _d(dmean),
                                                 _d(dvar) if variance else None))
        return mean, var, dmean, dvar

    def covariance(self, theta):
        """theta[p] -> K[N, N]; Theta[B, p] -> K[B, N, N] (the Listable form, BGP:59)."""
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64))
        if th.ndim == 2:
            K = np.zeros((th.shape[0], self.N, self.N))
            self._check(self._lib.gphip_covariance_batch(self._h, _d(th), th.shape[0], th.shape[1], _d(K)))
            return K
        th = th.ravel()
        K = np.zeros((self.N, self.N))
        self._check(self._lib.gphip_covariance(self._h, _d(th), th.size, _d(K)))
        return K

    def cross_covariance(self, theta, Xs):
        """compiledKandKappa (BGP:91-124): (k[N, M], kappa[M])."""
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        Xs = np.ascontiguousarray(np.atleast_2d(np.asarray(Xs, dtype=np.float64)))
        if Xs.shape[1] != self.d:
            raise GphipError(2, "test points have the wrong dimension")
        M = Xs.shape[0]
        k, kappa = np.zeros((self.N, M)), np.zeros(M)
        self._check(self._lib.gphip_cross_covariance(self._h, _d(th), th.size, Xs.ctypes.data, M, _d(k), _d(kappa)))
        return k, kappa

    def comm_info(self) -> dict:
        w, nl, name = C.c_int(0), C.c_int(0), C.c_char_p()
        self._check(self._lib.gphip_comm_info(self._h, C.byref(w), C.byref(nl), C.byref(name)))
        return {"world": w.value, "local": nl.value, "comm": (name.value or b"").decode()}

    def solve(self, rhs):
        rhs = np.asarray(rhs, dtype=np.float64)
        vec = rhs.ndim == 1
        B = np.ascontiguousarray(rhs.reshape(self.N, -1).T)      # each rhs contiguous
        out = np.zeros_like(B)
        self._check(self._lib.gphip_solve(self._h, _d(B), B.shape[0], _d(out)))
        return out[0] if vec else out.T.copy()

    def logdet(self) -> float:
        out = C.c_double(0.0)
        self._check(self._lib.gphip_logdet(self._h, C.byref(out)))
        return out.value

    def nested_sampling(self, box, prior_kind=None, logprior=None, start=None, cap=None, **options):
        """gphip_nested_sampling: the native batched sampler.  options: pool, max_iterations, min_iterations, mc_steps,
        walkers, termination_fraction, min_accept, max_accept, seed.  Returns a dict with Points, LogLikelihood,
        LogPriorPDF, AcceptanceRate (generation order), CrudeLogEvidence, LikelihoodEvaluations, SamplePoolSize."""
        o = NsOptions()
        self._check(self._lib.gphip_ns_default_options(C.byref(o)))
        for k, v in options.items():
            if not hasattr(o, k):
                raise GphipError(1, f"unknown sampler option {k!r}")
            setattr(o, k, v)
        box = np.ascontiguousarray(np.asarray(box, dtype=np.float64).reshape(self.p, 2))
        kinds = None if prior_kind is None else np.ascontiguousarray(np.asarray(prior_kind, dtype=np.int32))
        cb = None
        if logprior is not None:
            cb = LOGPRIOR_FN(lambda th, p, _u: float(logprior(np.ctypeslib.as_array(th, shape=(p,)).copy())))
        st = None if start is None else np.ascontiguousarray(np.asarray(start, dtype=np.float64).reshape(o.pool, self.p))
        cap = int(cap or (o.pool + max(o.max_iterations, o.min_iterations) + 1))
        pts, ll, lp, ar = np.zeros((cap, self.p)), np.zeros(cap), np.zeros(cap), np.zeros(cap)
        ns, ne, z = C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        self._check(self._lib.gphip_nested_sampling(
            self._h, _d(box), None if kinds is None else kinds.ctypes.data_as(_ip), C.cast(cb, C.c_void_p) if cb else None, None,
            C.byref(o), None if st is None else _d(st), cap, _d(pts), _d(ll), _d(lp), _d(ar), C.byref(ns), C.byref(z), C.byref(ne)))
        m = ns.value
        return {"Points": pts[:m].copy(), "LogLikelihood": ll[:m].copy(), "LogPriorPDF": lp[:m].copy(),
                "AcceptanceRate": ar[:m].copy(), "SamplePoolSize": int(o.pool), "GeneratedNestedSamples": m - int(o.pool),
                "TotalSamples": m, "CrudeLogEvidence": z.value, "LikelihoodEvaluations": ne.value, "Seed": int(o.seed)}

    # -- measurement ---------------------------------------------------------------------
    def reset_profile(self):
        self._check(self._lib.gphip_reset_profile(self._h))

    def profile(self) -> dict:
        res = {}
        for i, name in enumerate(PROFILE_CLASSES):
            v = [C.c_double(0.0) for _ in range(4)]
            self._check(self._lib.gphip_get_profile(self._h, i, *[C.byref(x) for x in v]))
            res[name] = dict(ms=v[0].value, launches=v[1].value, flops=v[2].value, bytes=v[3].value)
        return res

    def sync(self):
        self._check(self._lib.gphip_sync(self._h))

    def factor_bytes(self, member: int = 0) -> float:
        """device bytes local rank `member` holds for factor storage right now (workspace + own panels + receive buffers)"""
        v = C.c_double(0.0)
        self._check(self._lib.gphip_factor_bytes(self._h, member, C.byref(v)))
        return v.value

    def factor(self, winv: bool = False):
        """gphip_factor_get (diagnostics): the resident factor as (L[N, N] lower triangular, z[N] = L^-1 (y - mean)); winv=True adds
        W[Nt, 128, 128] with W[b, i, j] = element (i, j) of the inverse of the b-th 128 x 128 diagonal block of the padded factor
        (the library keeps these blocks column-major; this is the transposed view of its bytes)."""
        L, z = np.zeros((self.N, self.N)), np.zeros(self.N)
        W = np.zeros(((self.N + 127) // 128, 128, 128)) if winv else None
        self._check(self._lib.gphip_factor_get(self._h, _d(L), _d(z), _d(W) if winv else None))
        return (L, z, W.transpose(0, 2, 1)) if winv else (L, z)

    # -- multi-GPU block-cyclic Cholesky steps (driven by dist_cholesky.py) ---------------
    def set_streams(self, main_stream: int, panel_stream: int):
        self._check(self._lib.gphip_set_streams(self._h, C.c_void_p(main_stream), C.c_void_p(panel_stream)))

    def dist_num_panels(self) -> int:
        n = C.c_int(0)
        self._check(self._lib.gphip_dist_num_panels(self._h, C.byref(n)))
        return n.value

    def dist_panel_shape(self, k: int):
        r, c = C.c_int64(0), C.c_int64(0)
        self._check(self._lib.gphip_dist_panel_shape(self._h, k, C.byref(r), C.byref(c)))
        return r.value, c.value

    def dist_begin(self, theta, rank: int, world: int):
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        self._check(self._lib.gphip_dist_begin(self._h, _d(th), th.size, rank, world))

    @staticmethod
    def _dev_ptr(packed) -> int:
        """device address of a packed-panel buffer: a torch tensor (data_ptr) or a raw integer"""
        return int(packed.data_ptr()) if hasattr(packed, "data_ptr") else int(packed)

    def dist_factor_panel(self, k: int, packed):
        self._check(self._lib.gphip_dist_factor_panel(self._h, k, C.c_void_p(self._dev_ptr(packed))))

    def dist_update(self, k: int, packed, j_first: int, j_last: int, on_panel_stream: bool):
        self._check(self._lib.gphip_dist_update(self._h, k, C.c_void_p(self._dev_ptr(packed)), j_first, j_last,
                                                int(on_panel_stream)))

    def dist_end(self):
        ld, qd, info = C.c_double(0.0), C.c_double(0.0), C.c_int(0)
        self._check(self._lib.gphip_dist_end(self._h, C.byref(ld), C.byref(qd), C.byref(info)))
        return ld.value, qd.value, info.value


SPARSE_MAX_M = 16384
SPARSE_PARTS = ("logdet_B", "ctc", "rtr", "tr_VVt", "sum_kxx")
SPARSE_PHASES = ("ms_kuu_factor", "ms_cross", "ms_forward", "ms_accumulate", "ms_b_factor")
SPARSE_GRAD_PHASES = ("ms_grad_small", "ms_grad_weights", "ms_grad_backward", "ms_grad_reduce")
SPARSE_ZGRAD_PHASES = ("ms_grad_inducing",)
SPARSE_JOINT_PHASES = ("ms_joint_v", "ms_joint_build", "ms_joint_downdate", "ms_joint_factor")
SPARSE_SAMPLES_PHASES = ("ms_samples_v1", "ms_samples_handover", "ms_samples_v2", "ms_samples_reduce")
SPARSE_PGRAD_PHASES = ("ms_pgrad_backward", "ms_pgrad_reduce")


class SparseHandle:
    """Owns one gphip_sparse_handle: a sparse inducing-point GP (the collapsed bound of Titsias 2009, include/gphip.h
    gphip_sparse_*).  The data X, y stay resident on the device; Z [m, d] are the inducing points.  theta has the layout of the
    same kernel of `Handle`; jitter < 0 = the library's default (get_option("last_jitter") returns the value used)."""

    def __init__(self, X, y, Z, kernel="se_ard", mean: str = "zero", dtype: int = 64, device=None):
        lib = load()
        X = np.ascontiguousarray(np.atleast_2d(np.asarray(X, dtype=np.float64)))
        y = np.ascontiguousarray(np.asarray(y, dtype=np.float64).ravel())
        Z = np.ascontiguousarray(np.atleast_2d(np.asarray(Z, dtype=np.float64)))
        if X.shape[0] != y.shape[0]:
            raise GphipError(2, "Input and output data are not of same length")
        if Z.shape[1] != X.shape[1]:
            raise GphipError(2, "inducing points and data differ in dimension")
        if mean not in MEAN_IDS:
            raise GphipError(1, f"unknown mean {mean!r}")
        self.N, self.d = X.shape
        self.m = Z.shape[0]
        self.kernel, self.mean, self.dtype = kernel, mean, int(dtype)
        self._lib = lib
        self._h = _h()
        dev = -1 if device is None else int(device)
        if isinstance(kernel, CustomKernel):
            rc = lib.gphip_sparse_create_custom(X.ctypes.data, y.ctypes.data, self.N, self.d, Z.ctypes.data, self.m, kernel.body.encode(),
                                                int(kernel.nparams), MEAN_IDS[mean], int(dtype), dev, C.byref(self._h))
        else:
            rc = lib.gphip_sparse_create(X.ctypes.data, y.ctypes.data, self.N, self.d, Z.ctypes.data, self.m, kernel_id(kernel),
                                         MEAN_IDS[mean], int(dtype), dev, C.byref(self._h))
        if rc != OK:
            self._h = None
            why = {5: "no gfx950 GPU visible, or a device ordinal that does not exist", 6: "unsupported (the null kernel, dtype other than 64 / 32)",
                   1: "bad argument (unknown kernel / mean id) " + (lib.gphip_create_error() or b"").decode(),
                   2: f"bad shape (N < 1, d < 1, m < 1 or m > {SPARSE_MAX_M})"}.get(rc, "is a gfx950 GPU visible?")
            raise GphipError(rc, "gphip_sparse_create failed: " + why)
        p = C.c_int(0)
        lib.gphip_sparse_num_params(self._h, C.byref(p))
        self.p = p.value

    def _check(self, rc: int):
        if rc != OK:
            raise GphipError(rc, (self._lib.gphip_sparse_last_error(self._h) or b"").decode())

    def close(self):
        """gphip_sparse_destroy; refused (GphipError, status 4) while Paths objects of this handle are open"""
        if getattr(self, "_h", None):
            self._check(self._lib.gphip_sparse_destroy(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sample_paths(self, S: int, F: int = 1024, seed: int = 0):
        """gphip_sparse_paths_create: S pathwise draws of the latent posterior function of the resident fit, F random Fourier
        features per term.  Returns a Paths (close it before this handle), or None when v is not finite (info = GPHIP_INFO_NAN)."""
        S, F = int(S), int(F)
        if S < 1 or F < 1 or S > 2048:
            raise ValueError("S must be 1 .. 2048 and F at least 1, got S = %d, F = %d" % (S, F))
        out, info = _h(), C.c_int(0)
        self._check(self._lib.gphip_sparse_paths_create(self._h, S, F, int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(out), C.byref(info)))
        if not out.value:
            return None
        return Paths(self, out)

    def set_option(self, name: str, value: float):
        self._check(self._lib.gphip_sparse_set_option(self._h, name.encode(), float(value)))

    def get_option(self, name: str) -> float:
        v = C.c_double()
        self._check(self._lib.gphip_sparse_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def set_inducing(self, Z):
        """Replace the inducing points (any m); the resident fit is dropped.  With an unchanged m the points are replaced in
        place (no buffer, stream or compiled program is made again)."""
        Z = np.ascontiguousarray(np.atleast_2d(np.asarray(Z, dtype=np.float64)))
        if Z.shape[1] != self.d:
            raise GphipError(2, "inducing points and data differ in dimension")
        self._check(self._lib.gphip_sparse_set_inducing(self._h, Z.ctypes.data, Z.shape[0]))
        self.m = Z.shape[0]

    def bound_parts(self, theta, jitter: float = -1.0):
        """(F, parts[5] = (log det B, c'c, r'r, tr(V V'), sum_i k(x_i, x_i)), info); the fit stays resident."""
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        out, info, parts = C.c_double(0.0), C.c_int(0), np.zeros(5)
        self._check(self._lib.gphip_sparse_bound(self._h, _d(th), th.size, float(jitter), C.byref(out), _d(parts), C.byref(info)))
        return out.value, parts, info.value

    def bound(self, theta, jitter: float = -1.0):
        """(F(theta), info): the collapsed lower bound on the log marginal likelihood; the fit stays resident."""
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        out, info = C.c_double(0.0), C.c_int(0)
        self._check(self._lib.gphip_sparse_bound(self._h, _d(th), th.size, float(jitter), C.byref(out), None, C.byref(info)))
        return out.value, info.value

    def bound_batch(self, Theta, jitter: float = -1.0, parts: bool = False):
        """gphip_sparse_bound_batch: (F[B], info[B]) -- with parts=True (F[B], info[B], parts[B, 5]) -- for the rows of Theta
        [B, p] in ONE call; row s is `bound(Theta[s], jitter)` up to rounding, jitter < 0 the default rule per row.  A row that
        fails has info != 0 and F (and its parts) NaN without disturbing the others.  No fit stays resident."""
        Th = np.ascontiguousarray(np.asarray(Theta, dtype=np.float64))
        if Th.ndim == 1:
            Th = Th.reshape(1, -1)
        B, p = Th.shape
        out, info = np.zeros(B), np.zeros(B, dtype=np.int32)
        pr = np.zeros((B, 5)) if parts else None
        self._check(self._lib.gphip_sparse_bound_batch(self._h, _d(Th), B, p, float(jitter), _d(out), _d(pr) if parts else None,
                                                       info.ctypes.data_as(_ip)))
        return (out, info, pr) if parts else (out, info)

    def nested_sampling(self, box, jitter: float = -1.0, prior_kind=None, logprior=None, start=None, cap=None, **options):
        """gphip_sparse_nested_sampling: the native batched sampler with the bound F(theta; jitter) as the log-likelihood (one
        bound_batch per Metropolis step).  Options and the returned dict as Handle.nested_sampling."""
        o = NsOptions()
        self._check(self._lib.gphip_ns_default_options(C.byref(o)))
        for k, v in options.items():
            if not hasattr(o, k):
                raise GphipError(1, f"unknown sampler option {k!r}")
            setattr(o, k, v)
        box = np.ascontiguousarray(np.asarray(box, dtype=np.float64).reshape(self.p, 2))
        kinds = None if prior_kind is None else np.ascontiguousarray(np.asarray(prior_kind, dtype=np.int32))
        cb = None
        if logprior is not None:
            cb = LOGPRIOR_FN(lambda th, p, _u: float(logprior(np.ctypeslib.as_array(th, shape=(p,)).copy())))
        st = None if start is None else np.ascontiguousarray(np.asarray(start, dtype=np.float64).reshape(o.pool, self.p))
        cap = int(cap or (o.pool + max(o.max_iterations, o.min_iterations) + 1))
        pts, ll, lp, ar = np.zeros((cap, self.p)), np.zeros(cap), np.zeros(cap), np.zeros(cap)
        ns, ne, z = C.c_int64(0), C.c_int64(0), C.c_double(0.0)
        self._check(self._lib.gphip_sparse_nested_sampling(
            self._h, float(jitter), _d(box), None if kinds is None else kinds.ctypes.data_as(_ip), C.cast(cb, C.c_void_p) if cb else None,
            None, C.byref(o), None if st is None else _d(st), cap, _d(pts), _d(ll), _d(lp), _d(ar), C.byref(ns), C.byref(z), C.byref(ne)))
        m = ns.value
        return {"Points": pts[:m].copy(), "LogLikelihood": ll[:m].copy(), "LogPriorPDF": lp[:m].copy(),
                "AcceptanceRate": ar[:m].copy(), "SamplePoolSize": int(o.pool), "GeneratedNestedSamples": m - int(o.pool),
                "TotalSamples": m, "CrudeLogEvidence": z.value, "LikelihoodEvaluations": ne.value, "Seed": int(o.seed)}

    def bound_grad(self, theta, jitter: float = -1.0):
        """(F(theta), dF/dtheta, info): the bound -- the same bytes as `bound` -- and its gradient in theta's layout, the jitter
        held fixed; the gradient is NaN when info != 0.  get_option("grad_analytic") tells whether the analytic route ran.  The
        fit stays resident."""
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        out, info, grad = C.c_double(0.0), C.c_int(0), np.zeros(th.size)
        self._check(self._lib.gphip_sparse_bound_grad(self._h, _d(th), th.size, float(jitter), C.byref(out), _d(grad), None, C.byref(info)))
        return out.value, grad, info.value

    def bound_grad_inducing(self, theta, jitter: float = -1.0, with_theta: bool = True):
        """(F(theta), dF/dtheta or None, dF/dZ [m, d], info): the bound -- the same bytes as `bound` --, its gradient in theta
        (the same bytes as `bound_grad`; None with with_theta=False, which skips those reductions) and its gradient in the
        inducing locations, in the coordinates Z was given in, all from one pass; the jitter is held fixed.  The gradients are
        NaN when info != 0.  Named and composed kernels only: a run-time compiled one raises GphipError (status 6).  The fit
        stays resident."""
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        out, info = C.c_double(0.0), C.c_int(0)
        grad = np.zeros(th.size) if with_theta else None
        gz = np.zeros((self.m, self.d))
        self._check(self._lib.gphip_sparse_bound_grad_inducing(self._h, _d(th), th.size, float(jitter), C.byref(out),
                                                               _d(grad) if with_theta else None, _d(gz), None, C.byref(info)))
        return out.value, grad, gz, info.value

    def fit(self, theta, jitter: float = -1.0) -> int:
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        info = C.c_int(0)
        self._check(self._lib.gphip_sparse_fit(self._h, _d(th), th.size, float(jitter), C.byref(info)))
        return info.value

    def predict(self, Xs, latent: bool = False):
        """(mean[M], var[M]) at Xs from the resident fit; latent: the variance of f(x*) without the noise sn^2."""
        Xs = np.ascontiguousarray(np.atleast_2d(np.asarray(Xs, dtype=np.float64)))
        if Xs.shape[1] != self.d:
            raise GphipError(2, "test points and data differ in dimension")
        M = Xs.shape[0]
        mean, var = np.zeros(M), np.zeros(M)
        self._check(self._lib.gphip_sparse_predict(self._h, Xs.ctypes.data, M, 1 if latent else 0, _d(mean), _d(var)))
        return mean, var

    def predict_grad(self, Xs, variance: bool = True):
        """Gradients of the resident fit's prediction in the test inputs (gphip_sparse_predict_grad): (mean[M], var[M],
        dmean[M, d], dvar[M, d]); var is that of a noisy observation; variance=False returns dvar = None."""
        Xs = self._test_points(Xs)
        M = Xs.shape[0]
        mean, var, dmean = np.zeros(M), np.zeros(M), np.zeros((M, self.d))
        dvar = np.zeros((M, self.d)) if variance else None
        self._check(self._lib.gphip_sparse_predict_grad(self._h, Xs.ctypes.data, M, _d(mean), _d(var), _d(dmean),
                                                        _d(dvar) if variance else None))
        return mean, var, dmean, dvar

    def predict_samples(self, Thetas, Xs, jitter: float = -1.0, latent: bool = False, bound: bool = False):
        """gphip_sparse_predict_samples: (mean[S, M], var[S, M], info[S]) -- with bound=True also F[S] -- at Xs for the rows of
        Thetas [S, p] in ONE call; row s is `fit(Thetas[s], jitter)` followed by `predict(Xs, latent)` up to rounding, jitter < 0
        the default rule per row.  A row that fails has info != 0 and its rows of mean and var (and its F) NaN without disturbing
        the others.  No fit stays resident."""
        Th = np.ascontiguousarray(np.asarray(Thetas, dtype=np.float64))
        if Th.ndim == 1:
            Th = Th.reshape(1, -1)
        Xs = self._test_points(Xs)
        S, p = Th.shape
        M = Xs.shape[0]
        mean, var, info = np.zeros((S, M)), np.zeros((S, M)), np.zeros(S, dtype=np.int32)
        F = np.zeros(S) if bound else None
        self._check(self._lib.gphip_sparse_predict_samples(self._h, _d(Th), S, p, float(jitter), Xs.ctypes.data, M, int(bool(latent)),
                                                           _d(mean), _d(var), _d(F) if bound else None, info.ctypes.data_as(_ip)))
        return (mean, var, info, F) if bound else (mean, var, info)

    # ---- a mean and a noise variance that depend on the point (gphip_sparse_*_pw)
    @staticmethod
    def _pw_array(a, rows, cols, what):
        """None, or the contiguous fp64 [rows, cols] array of a point-dependent quantity (one row may be given 1-D)."""
        if a is None:
            return None
        a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
        if a.size != rows * cols:
            raise GphipError(2, f"{what} needs {rows} x {cols} values, got an array of shape {a.shape}")
        return a.reshape(rows, cols)

    def bound_pw(self, theta, jitter: float = -1.0, mean_train=None, nugget_train=None, parts: bool = False):
        """gphip_sparse_bound_pw: (F, info) -- with parts=True (F, parts[6], info) -- with the mean m_i and the noise VARIANCE
        nu_i at the N training points as arrays (None: the constant of theta).  parts = (log det B, c'c, r'W r, tr(V W V'),
        sum_i k_ii / nu_i, sum_i log nu_i) with W = diag(1 / nu) and B = I + V W V'.  The fit stays resident."""
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        mt = self._pw_array(mean_train, 1, self.N, "mean_train")
        nt = self._pw_array(nugget_train, 1, self.N, "nugget_train")
        out, info, pr = C.c_double(0.0), C.c_int(0), np.zeros(6)
        self._check(self._lib.gphip_sparse_bound_pw(self._h, _d(th), th.size, float(jitter), None if mt is None else _d(mt),
                                                    None if nt is None else _d(nt), C.byref(out), _d(pr) if parts else None, C.byref(info)))
        return (out.value, pr, info.value) if parts else (out.value, info.value)

    def bound_batch_pw(self, Theta, jitter: float = -1.0, mean_train=None, nugget_train=None, parts: bool = False):
        """gphip_sparse_bound_batch_pw: (F[B], info[B]) -- with parts=True also parts[B, 6] -- for the rows of Theta [B, p] with
        the arrays mean_train / nugget_train [B, N] (row s for row s of Theta; None: the constant of theta) in ONE call."""
        Th = np.ascontiguousarray(np.asarray(Theta, dtype=np.float64))
        if Th.ndim == 1:
            Th = Th.reshape(1, -1)
        B, p = Th.shape
        mt = self._pw_array(mean_train, B, self.N, "mean_train")
        nt = self._pw_array(nugget_train, B, self.N, "nugget_train")
        out, info = np.zeros(B), np.zeros(B, dtype=np.int32)
        pr = np.zeros((B, 6)) if parts else None
        self._check(self._lib.gphip_sparse_bound_batch_pw(self._h, _d(Th), B, p, float(jitter), None if mt is None else _d(mt),
                                                          None if nt is None else _d(nt), _d(out), _d(pr) if parts else None,
                                                          info.ctypes.data_as(_ip)))
        return (out, info, pr) if parts else (out, info)

    def fit_pw(self, theta, jitter: float = -1.0, mean_train=None, nugget_train=None) -> int:
        th = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).ravel())
        mt = self._pw_array(mean_train, 1, self.N, "mean_train")
        nt = self._pw_array(nugget_train, 1, self.N, "nugget_train")
        info = C.c_int(0)
        self._check(self._lib.gphip_sparse_fit_pw(self._h, _d(th), th.size, float(jitter), None if mt is None else _d(mt),
                                                  None if nt is None else _d(nt), C.byref(info)))
        return info.value

    def predict_pw(self, Xs, latent: bool = False, mean_test=None, nugget_test=None):
        """gphip_sparse_predict_pw: (mean[M], var[M]) at Xs from the resident fit with m(x*) and nu(x*) at the test points as
        arrays (None: the constant of the fit's theta); nugget_test is not read for a latent prediction."""
        Xs = self._test_points(Xs)
        M = Xs.shape[0]
        mt = self._pw_array(mean_test, 1, M, "mean_test")
        nt = self._pw_array(nugget_test, 1, M, "nugget_test")
        mean, var = np.zeros(M), np.zeros(M)
        self._check(self._lib.gphip_sparse_predict_pw(self._h, Xs.ctypes.data, M, 1 if latent else 0, None if mt is None else _d(mt),
                                                      None if nt is None else _d(nt), _d(mean), _d(var)))
        return mean, var

    def predict_samples_pw(self, Thetas, Xs, jitter: float = -1.0, latent: bool = False, mean_train=None, nugget_train=None,
                           mean_test=None, nugget_test=None, bound: bool = False):
        """gphip_sparse_predict_samples_pw: `predict_samples` with the training arrays [S, N] and the test arrays [S, M] of a
        point-dependent mean and noise variance (None: the constant of the row's theta)."""
        Th = np.ascontiguousarray(np.asarray(Thetas, dtype=np.float64))
        if Th.ndim == 1:
            Th = Th.reshape(1, -1)
        Xs = self._test_points(Xs)
        S, p = Th.shape
        M = Xs.shape[0]
        arrs = [self._pw_array(mean_train, S, self.N, "mean_train"), self._pw_array(nugget_train, S, self.N, "nugget_train"),
                self._pw_array(mean_test, S, M, "mean_test"), self._pw_array(nugget_test, S, M, "nugget_test")]
        ptr = [None if a is None else _d(a) for a in arrs]
        mean, var, info = np.zeros((S, M)), np.zeros((S, M)), np.zeros(S, dtype=np.int32)
        F = np.zeros(S) if bound else None
        self._check(self._lib.gphip_sparse_predict_samples_pw(self._h, _d(Th), S, p, float(jitter), ptr[0], ptr[1], Xs.ctypes.data, M,
                                                              int(bool(latent)), ptr[2], ptr[3], _d(mean), _d(var),
                                                              _d(F) if bound else None, info.ctypes.data_as(_ip)))
        return (mean, var, info, F) if bound else (mean, var, info)

    def _test_points(self, Xs):
        Xs = np.ascontiguousarray(np.atleast_2d(np.asarray(Xs, dtype=np.float64)))
        if Xs.shape[1] != self.d:
            raise GphipError(2, "test points and data differ in dimension")
        return Xs

    def predict_cov(self, Xs, latent: bool = False):
        """Joint predictive distribution at Xs[M, d] from the resident fit: (mean[M], cov[M, M]).  latent=False: covariance of
        noisy observations (its diagonal is predict()'s var); latent=True: of the latent function.  The fit stays resident."""
        Xs = self._test_points(Xs)
        M = Xs.shape[0]
        mean, cov = np.zeros(M), np.zeros((M, M))
        self._check(self._lib.gphip_sparse_predict_cov(self._h, Xs.ctypes.data, M, int(bool(latent)), _d(mean), _d(cov)))
        return mean, cov

    def predict_draws(self, Xs, S: int, seed: int = 0, z=None, latent: bool = True, jitter: float = -1.0):
        """S draws from the joint predictive distribution: (out[S, M], info).  z: the caller's standard normals [S, M]
        (None: generated on the device from (seed, s, j)); jitter < 0: the library's default, 0: none."""
        Xs = self._test_points(Xs)
        M, S = Xs.shape[0], int(S)
        zp = None
        if z is not None:
            z = np.ascontiguousarray(np.asarray(z, dtype=np.float64))
            if z.shape != (S, M):
                raise GphipError(2, f"z must have shape ({S}, {M})")
            zp = _d(z)
        out = np.zeros((max(S, 0), M))
        info = C.c_int(0)
        self._check(self._lib.gphip_sparse_predict_draws(self._h, Xs.ctypes.data, M, int(bool(latent)), S, int(seed) & (2**64 - 1), zp,
                                                         float(jitter), _d(out), C.byref(info)))
        return out, info.value

    def predict_logpdf(self, Xs, ystar):
        """log N(ystar | mean, cov) with the noisy-observation covariance at Xs: (value, info)."""
        Xs = self._test_points(Xs)
        M = Xs.shape[0]
        ys = np.ascontiguousarray(np.asarray(ystar, dtype=np.float64).ravel())
        if ys.shape != (M,):
            raise GphipError(2, f"ystar must have length {M}")
        out, info = C.c_double(0.0), C.c_int(0)
        self._check(self._lib.gphip_sparse_predict_logpdf(self._h, Xs.ctypes.data, M, _d(ys), C.byref(out), C.byref(info)))
        return out.value, info.value
