// gphip_loo.inc -- leave-one-out cross-validation from one factorisation (include/gphip.h: gphip_loo, gphip_loo_grad; kernels
// and formulas: gp_loo.h).  Included at the end of gphip.hip.
//
//   both calls   factor under FactorMode as gphip_loglik_grad does on its potri route; queue_u says where U = L^-T is (InvBufs)
//                loo_rownorm_partial_kernel    alpha = U z and k = squared row norms of U, one pass over U
//                loo_moments_kernel            mean, var, logp, g, sqrt(c) per point;   loo_total_kernel   L_LOO
//   gradient     queue_kinv                    K^-1 = U U^T, lower tiles, into the OTHER buffer
//                loo_mirror_scale_kernel       B = K^-1 diag(sqrt c) in place (full matrix) + the partial sums of beta = K^-1 g
//                launch_gemm                   M = B B^T, lower tiles, into the buffer U occupied (U is dead by then)
//                queue_grad_full               the gradient reductions with GradArgs::beta set, Kinv = M
// The value path touches ONE N x N buffer, the gradient two; there is no third.
#include "gp_loo.h"

namespace {

// dLoo: [z | beta | mean var logp g s k | total | partial sums], every part 256-byte aligned
struct LooScratch {
    void *z, *beta;
    double *out6, *total, *part;
    int nch;                                   // 128-column chunks of the row-norm pass (the beta pass uses 2 nch 64-row chunks)
};
int loo_scratch(gphip_ctx* h, LooScratch* s) {
    const size_t npad = (size_t)h->Npad, vec = (npad * 8 + 255) / 256 * 256;
    s->nch = (int)(npad / TB);
    const size_t part = (size_t)2 * s->nch * npad * 8;
    HIPCHK(h->dLoo.grow(8 * vec + 256 + part));
    char* b = static_cast<char*>(h->dLoo.p);
    s->z = b; s->beta = b + vec;
    s->out6 = reinterpret_cast<double*>(b + 2 * vec);          // (6 npad doubles: contiguous, the kernel strides by npad)
    s->total = reinterpret_cast<double*>(b + 8 * vec);
    s->part = reinterpret_cast<double*>(b + 8 * vec + 256);
    return GPHIP_OK;
}

void loo_nan(gphip_ctx* h, double* mean, double* var, double* logp, double* out) {
    const double q = std::nan("");
    for (int64_t i = 0; i < h->N; ++i) {
        if (mean) mean[i] = q;
        if (var) var[i] = q;
        if (logp) logp[i] = q;
    }
    if (out) *out = q;
}

// behind the factorisation, U = L^-T on the device (b.U): z, alpha and k in one pass, the per-point quantities in s.out6, L_LOO
template <typename T>
int loo_queue_values(gphip_ctx* h, const LooScratch& s, const InvBufs& b) {
    const int npad = (int)h->Npad, n = (int)h->N, chunk = TB;
    double* part_a = s.part;
    double* part_k = s.part + (size_t)s.nch * npad;
    hipLaunchKernelGGL(gather_rhs_row_kernel<T>, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, h->stream, (const T*)h->dA.p,
                       (int)h->R, 0, npad, (T*)s.z, 1l);
    hipLaunchKernelGGL(loo_rownorm_partial_kernel<T>, dim3((unsigned)(npad / TB), (unsigned)s.nch), dim3(TB), 0, h->stream, (const T*)b.U,
                       b.ld, (const T*)s.z, npad, chunk, part_a, part_k);
    hipLaunchKernelGGL(loo_moments_kernel<T>, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, h->stream, (const double*)part_a,
                       (const double*)part_k, s.nch, npad, n, (const T*)h->dY.p, (T*)h->dAlpha.p, s.out6);
    hipLaunchKernelGGL(loo_total_kernel, dim3(1), dim3(LOO_RED), 0, h->stream, (const double*)(s.out6 + 2 * (size_t)npad), n, s.total);
    return GPHIP_OK;
}

// the rest of the gradient: K^-1, beta, B, M, the reductions
template <typename T>
int loo_queue_grad(gphip_ctx* h, const LooScratch& s, const InvBufs& b) {
    const long npad = h->Npad;
    T *Ub = (T*)b.U, *Kb = (T*)b.other;
    queue_kinv<T>(h, b);
    const unsigned nb = (unsigned)(npad / LOO_BLK);
    hipLaunchKernelGGL(loo_mirror_scale_kernel<T>, dim3(nb, nb), dim3(256), 0, h->stream, Kb, b.ld, (int)npad,
                       (const double*)(s.out6 + 4 * (size_t)npad), (const double*)(s.out6 + 3 * (size_t)npad), s.part);
    hipLaunchKernelGGL(utri_gemv_finish_kernel<T>, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, h->stream, (const double*)s.part,
                       (int)nb, (int)npad, (T*)s.beta);
    // M = B B^T over the full contraction length (B is not triangular), lower tiles, over the dead U
    launch_gemm<T>(h, 2, cm<T>(Ub, b.ld, 0), cm<T>(Kb, b.ld, 0), cm<T>(Kb, b.ld, 0), (int)npad, 0, (int)h->Nt, 0, (int)h->Nt, 1, 1, 1, 0);
    queue_grad_full<T>(h, Ub, b.ld, s.beta);
    return GPHIP_OK;
}

// Null kernel: K = sn^2 I, so leaving a point out changes nothing: mu_-i = m, var_-i = sn^2 (host; y comes back from the device once)
int loo_null(gphip_ctx* h, const double* theta, double* mean, double* var, double* logp, double* out, double* grad, int* info) {
    double mu = 0.0;
    *info = null_theta_info(h, theta, &mu);
    const double sn = theta[0], v = sn * sn;
    if (grad) for (int i = 0; i < h->p; ++i) grad[i] = std::nan("");
    if (*info != 0) { loo_nan(h, mean, var, logp, out); return GPHIP_OK; }
    HIPCHK(hipSetDevice(h->device));
    std::vector<double> y;
    const int rc = DISPATCH(h, download, h, y, h->dY.p, (size_t)h->N, h->stream);
    if (rc) return rc;
    double sr = 0.0, srr = 0.0;
    std::vector<double> part((size_t)LOO_RED, 0.0);            // L_LOO in the order of loo_total_kernel
    for (int64_t i = 0; i < h->N; ++i) {
        const double r = y[(size_t)i] - mu, lp = -0.5 * std::log(v) - 0.5 * r * r / v - 0.5 * LOG_TWO_PI;
        if (mean) mean[i] = mu;
        if (var) var[i] = v;
        if (logp) logp[i] = lp;
        part[(size_t)(i % LOO_RED)] += lp; sr += r; srr += r * r;
    }
    for (int off = LOO_RED / 2; off > 0; off >>= 1)
        for (int t = 0; t < off; ++t) part[(size_t)t] += part[(size_t)(t + off)];
    *out = part[0];
    if (grad) {
        grad[0] = (srr / v - (double)h->N) / sn;
        if (h->mean_id == GPHIP_MEAN_CONST) grad[1] = sr / v;
    }
    if (grad) h->grad_analytic = 1;
    return GPHIP_OK;
}

// grad == nullptr: the value call
int loo_call(gphip_ctx* h, const double* theta, int p, double* mean, double* var, double* logp, double* out, double* grad, int* info) {
    if (p != h->p) return fail(h, GPHIP_ERR_DIM, "theta has the wrong length for this kernel/mean");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (h->pw_mean_host || h->pw_nug_host)
        return fail(h, GPHIP_ERR_UNSUPPORTED, "leave-one-out with a point-dependent nugget / mean is not implemented");
    if (h->kernel_id == GPHIP_KERNEL_NULL) return loo_null(h, theta, mean, var, logp, out, grad, info);
    HIPCHK(hipSetDevice(h->device));
    const int64_t N = h->N, Npad = h->Npad;
    auto unsupported = [&]() {
        return fail(h, GPHIP_ERR_UNSUPPORTED, grad ? "gphip_loo_grad: two N x N scratch buffers do not fit in a quarter of the free device memory"
                                                   : "gphip_loo: one N x N scratch buffer does not fit in a quarter of the free device memory");
    };
    double parts[2] = {0, 0};
    int rc = GPHIP_OK;
    {
        // Where U will be: a single-launch factorisation goes on to the inverse launch, every other schedule leaves U to the
        // forward substitution of the identity (queue_u).  The value call claims that one buffer, the gradient both
        // (claim_inverse_scratch).  There is no row-block route here.
        FactorMode mode(h, true, h->grad_potri == 1);
        const bool inverse_launch = h->want_u && use_dataflow(h, 1);
        FactorMode predicted(h, true, inverse_launch);         // (the inverse launch runs only where its buffer was claimed)
        if (!claim_inverse_scratch(h, grad || inverse_launch, grad || !inverse_launch)) return unsupported();
        rc = eval_batch_local(h, theta, 1, p, out, parts, info);      // (a multi-device handle factors on its first device, as the gradient does)
    }
    if (rc) return rc;
    if (grad) for (int i = 0; i < p; ++i) grad[i] = std::nan("");
    if (*info != 0) { loo_nan(h, mean, var, logp, out); return GPHIP_OK; }
    if (!inverse_launch_ran(h) && (rc = ensure_vbuf(h, Npad + GRAD_LD_PAD))) return rc;   // (no-op unless the schedule chose otherwise than predicted)
    LooScratch s{};
    if ((rc = loo_scratch(h, &s))) return rc;
    HIPCHK(h->dAlpha.grow((size_t)Npad * h->es));
    if (grad && (rc = ensure_gacc(h))) return rc;
    const InvBufs ib = DISPATCH(h, queue_u, h);
    rc = DISPATCH(h, loo_queue_values, h, s, ib);
    if (rc) return rc;
    double total = 0.0;
    std::vector<double> gacc(grad ? h->ngacc : 0), beta;
    if (grad) {
        HIPCHK(hipMemsetAsync(h->dGacc.p, 0, gacc.size() * 8, h->stream));
        rc = DISPATCH(h, loo_queue_grad, h, s, ib);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(gacc.data(), h->dGacc.p, gacc.size() * 8, hipMemcpyDeviceToHost, h->stream));
    }
    // only what the caller asked for comes back
    double* want[3] = {mean, var, logp};
    for (int q = 0; q < 3; ++q)
        if (want[q]) HIPCHK(hipMemcpyAsync(want[q], s.out6 + (size_t)q * Npad, (size_t)N * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(&total, s.total, 8, hipMemcpyDeviceToHost, h->stream));
    rc = complete_call(h, [&]() -> int {
        if (grad) return DISPATCH(h, download, h, beta, s.beta, (size_t)N, h->stream);
        HIPCHK(hipStreamSynchronize(h->stream));
        return GPHIP_OK;
    });
    if (rc) return rc;
    *out = total;
    if (!std::isfinite(total)) {               // (a factor that passed the pivot test but whose U overflowed: fp32, extreme theta)
        *info = GPHIP_INFO_NAN;
        loo_nan(h, mean, var, logp, out);
        record_fit(h, true, theta, p, parts[0]);
        return GPHIP_OK;
    }
    if (grad) grad_from_acc(h, theta, gacc, beta, grad);
    record_fit(h, true, theta, p, parts[0]);   // the factor of theta is still resident (whole, on this device)
    return GPHIP_OK;
}

}  // namespace

extern "C" {

int gphip_loo(gphip_handle h, const double* theta, int p, double* mean, double* var, double* logp, double* out, int* info) {
    if (!h || !theta || !out || !info) return fail(h, GPHIP_ERR_ARG, "null argument");
    return loo_call(h, theta, p, mean, var, logp, out, nullptr, info);
}

int gphip_loo_grad(gphip_handle h, const double* theta, int p, double* out, double* grad, int* info) {
    if (!h || !theta || !out || !grad || !info) return fail(h, GPHIP_ERR_ARG, "null argument");
    if (p != h->p) return fail(h, GPHIP_ERR_DIM, "theta has the wrong length for this kernel/mean");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (h->custom) {
        if (const int rc = ensure_custom_grad(h)) return rc;
    }
    h->grad_analytic = 0;
    if (h->custom && !(h->custom_grad && h->cgrad_state == 1)) {
        // central differences of gphip_loo with the step rule of gphip_loglik_grad (fd_step); the value at theta itself is
        // evaluated last, so the fit the call leaves resident is theta's
        std::vector<double> th(theta, theta + p);
        for (int k = 0; k < p; ++k) {
            const double step = fd_step(h, theta[k]);
            double lp = 0.0, lm = 0.0;
            int ip = 0, im = 0;
            th[(size_t)k] = theta[k] + step;
            int rc = loo_call(h, th.data(), p, nullptr, nullptr, nullptr, &lp, nullptr, &ip);
            th[(size_t)k] = theta[k] - step;
            if (!rc) rc = loo_call(h, th.data(), p, nullptr, nullptr, nullptr, &lm, nullptr, &im);
            th[(size_t)k] = theta[k];
            if (rc) return rc;
            grad[k] = (ip == 0 && im == 0) ? (lp - lm) / (2.0 * step) : std::nan("");
        }
        const int rc = loo_call(h, theta, p, nullptr, nullptr, nullptr, out, nullptr, info);
        if (rc) return rc;
        if (*info != 0) for (int k = 0; k < p; ++k) grad[k] = std::nan("");
        return GPHIP_OK;
    }
    return loo_call(h, theta, p, nullptr, nullptr, nullptr, out, grad, info);
}

}  // extern "C"
