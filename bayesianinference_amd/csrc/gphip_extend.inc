// gphip_extend.inc -- new observations into a resident fit without refactoring it (include/gphip.h: gphip_extend; DESIGN.md
// section 8k).  Included at the end of gphip.hip, after gphip_joint.inc.
//
// After the joint log density of the new points the parts of the factor of all N + M points are resident:
//   parent (the fitted handle)   L, z = L^-1 r in its workspace, V = L^-1 k(X, X_new) in dV
//   child  (h->joint)            L_Sigma = chol(k(X_new, X_new) + sn^2 I - V^T V), z_new = L_Sigma^-1 (y_new - mu)
//   L' = [L 0; V^T L_Sigma],  z' = [z; z_new],  log det K' = log det K + log det Sigma
// A NEW context on the concatenated host data takes them:
//   create_ctx + ensure_slots    the buffers of a fresh handle after its first fit
//   stage_theta / copy_theta, queue_scale_train, queue_custom_prep    scaled inputs and slot scalars as queue_build leaves them
//   extend_assemble_kernel       slot 0 of the tile-major workspace from the three sources (gp_extend.h), behind events of the
//                                parent's and the child's streams
//   trtri128_kernel              the 128-block inverses of the new diagonal tiles, as after a look-ahead-schedule fit
// Everything made lazily per factor (dW64, dLT / dW64T, dTrsvP, U) carries a generation that no factor of the new context has: it is
// made on first use.  The parent is only read.
#include "gp_extend.h"

namespace {

template <typename T>
int queue_extend_assemble(gphip_ctx* h, gphip_ctx* n, int64_t M, int64_t mpad) {
    const gphip_ctx* c = h->joint;
    ExtendArgs<T> a{};
    a.out = (T*)n->dA.p; a.Rn = (int)n->R;
    a.A = (const T*)h->dA.p; a.Rp = (int)h->R;
    a.V = (const T*)h->dV.p; a.mpad = (long)mpad;
    a.C = (const T*)c->dA.p; a.Rc = (int)c->R;
    a.N = (int)h->N; a.M = (int)M;
    const long ntiles = (long)n->R * (n->R + 1) / 2;
    hipLaunchKernelGGL(extend_assemble_kernel<T>, dim3((unsigned)ntiles), dim3(256), 0, n->stream, a);
    return GPHIP_OK;
}

template <typename T>
int queue_extend_inverses(gphip_ctx* n) {
    hipLaunchKernelGGL(trtri128_kernel<T>, dim3((unsigned)n->Nt, 1), dim3(256), potrf_lds<T>(), n->stream, (const T*)n->dA.p,
                       (long)n->slot_elems, (T*)n->dW.p, (int)n->Nt);
    return GPHIP_OK;
}

// the context of the N + M points, on the parent's device, from the fp64 host values both were given
int extend_create(gphip_ctx* h, const double* Xn, const double* yn, int64_t M, gphip_ctx** out) {
    const int64_t N = h->N, d = h->d;
    std::vector<double> X(h->hostX), y(h->hostY);
    X.insert(X.end(), Xn, Xn + (size_t)M * (size_t)d);
    y.insert(y.end(), yn, yn + (size_t)M);
    gphip_handle n = nullptr;
    std::string why;
    const int rc = create_ctx(X.data(), y.data(), N + M, d, h->custom ? (int)GPHIP_KERNEL_CUSTOM : h->kernel_id, h->mean_id, h->dtype, h->device,
                              &n, h->custom ? h->custom_body.c_str() : nullptr, h->ncp, &why);
    (void)hipSetDevice(h->device);
    if (rc) return fail(h, rc, ("gphip_extend: creating the context of the N + M points failed " + why).c_str());
    *out = n;
    return GPHIP_OK;
}

int extend_us(std::chrono::steady_clock::time_point t0) {
    return (int)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

extern "C" {

int gphip_extend(gphip_handle h, const void* X_new, const double* y_new, int64_t M, gphip_handle* out, double* logp, int* info) {
    if (!h || !X_new || !y_new || !out || !info) return fail(h, GPHIP_ERR_ARG, "null argument");
    *out = nullptr;
    if (logp) *logp = NAN;
    if (int rc = joint_dim_check(h, M)) return rc;
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (int rc = joint_common_checks(h)) return rc;
    if ((int64_t)h->hostX.size() != h->N * h->d || (int64_t)h->hostY.size() != h->N)
        return fail(h, GPHIP_ERR_STATE, "gphip_extend: the handle has no host copy of its data");
    *info = GPHIP_INFO_OK;
    const double* Xn = static_cast<const double*>(X_new);
    for (int64_t j = 0; j < M; ++j)
        if (!std::isfinite(y_new[j])) { *info = GPHIP_INFO_NAN; return GPHIP_OK; }
    gphip_ctx* n = nullptr;
    if (h->null_fit) {                             // K = diag(sn^2): independent normals, and nothing to assemble
        double lp = 0.0;
        int inf = 0;
        if (int rc = gphip_predict_logpdf(h, X_new, M, y_new, &lp, &inf)) return rc;
        if (inf != 0) { *info = inf; return GPHIP_OK; }
        if (int rc = extend_create(h, Xn, y_new, M, &n)) return rc;
        n->fitted = n->null_fit = true;
        n->fit_pw = false; n->dist_fit = false;
        stamp_fit(n);
        n->theta_fit = h->theta_fit;
        n->mu_fit = h->mu_fit; n->kappa_fit = h->kappa_fit;
        n->logdet_fit = (double)n->N * std::log(h->kappa_fit);
        if (logp) *logp = lp;
        *out = n;
        return GPHIP_OK;
    }
    // L_Sigma, z_new, log det Sigma and the quadratic form: the joint log density's own route (noisy Sigma, no jitter)
    auto t0 = std::chrono::steady_clock::now();
    int rc = joint_sigma(h, Xn, M, y_new, true, nullptr);
    if (rc) return rc;
    double lp = 0.0;
    int inf = 0;
    if ((rc = joint_logpdf_tail(h, M, &lp, &inf))) return rc;
    h->extend_logpdf_us = extend_us(t0);
    if (inf != 0) { *info = inf; return GPHIP_OK; }
    gphip_ctx* c = h->joint;
    const double logdet = h->logdet_fit + c->hRes.as<double>()[0];
    const int64_t mpad = (M + TB - 1) / TB * TB;

    t0 = std::chrono::steady_clock::now();
    if ((rc = extend_create(h, Xn, y_new, M, &n))) return rc;
    auto bail = [&](int code, const std::string& why) {
        gphip_destroy(n);
        (void)hipSetDevice(h->device);
        return fail(h, code, ("gphip_extend: " + why).c_str());
    };
    if ((rc = ensure_slots(n, 1))) return bail(rc, n->err);
    h->extend_create_us = extend_us(t0);
    if (!stage_theta(n, 0, h->theta_fit.data())) return bail(GPHIP_ERR_ARG, "the fitted theta does not stage");
    if ((rc = copy_theta(n, 1))) return bail(rc, n->err);
    if (hipMemsetAsync(n->dInfo.p, 0, 4, n->stream) != hipSuccess) return bail(GPHIP_ERR_HIP, "clearing the info word failed");
    DISPATCH(n, queue_scale_train, n);
    queue_custom_prep(n, 1);
    // the assembly reads the parent's factor and V and the child's factor: behind both streams by events
    hipEvent_t ev[5];
    for (hipEvent_t& e : ev) e = get_event(n);
    hipError_t e1 = hipEventRecord(ev[0], h->stream);
    if (e1 == hipSuccess) e1 = hipStreamWaitEvent(n->stream, ev[0], 0);
    if (e1 == hipSuccess) e1 = hipEventRecord(ev[1], c->stream);
    if (e1 == hipSuccess) e1 = hipStreamWaitEvent(n->stream, ev[1], 0);
    if (e1 == hipSuccess) e1 = hipEventRecord(ev[2], n->stream);
    if (e1 == hipSuccess) {
        DISPATCH(n, queue_extend_assemble, h, n, M, mpad);
        e1 = hipEventRecord(ev[3], n->stream);
    }
    if (e1 == hipSuccess) {
        DISPATCH(n, queue_extend_inverses, n);
        e1 = hipEventRecord(ev[4], n->stream);
    }
    if (e1 == hipSuccess) rc = complete_call(n);
    float ms_a = 0.f, ms_d = 0.f;
    if (e1 == hipSuccess && !rc) {
        (void)hipEventElapsedTime(&ms_a, ev[2], ev[3]);
        (void)hipEventElapsedTime(&ms_d, ev[3], ev[4]);
    }
    for (hipEvent_t e : ev) n->pool.push_back(e);
    if (e1 != hipSuccess) { (void)hipGetLastError(); return bail(GPHIP_ERR_HIP, std::string("queueing the assembly failed: ") + hipGetErrorString(e1)); }
    if (rc) return bail(rc, n->err);
    h->extend_assemble_us = (int)(ms_a * 1000.f);
    h->extend_derive_us = (int)(ms_d * 1000.f);
    record_fit(n, true, h->theta_fit.data(), (int)h->theta_fit.size(), logdet);
    if (logp) *logp = lp;
    *out = n;
    return GPHIP_OK;
}

}  // extern "C"
