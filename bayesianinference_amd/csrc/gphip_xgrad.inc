// gphip_xgrad.inc -- gradients of the predictive mean and variance in the test inputs (include/gphip.h: gphip_predict_grad;
// DESIGN.md section 8j).  Included at the end of gphip.hip, before gphip_sparse.inc (gphip_sparse_predict_grad shares queue_xgrad).
//
//   per chunk of test points     V = L^-1 k(X, X*)     stage_test_chunk + queue_forward_fit, as gphip_predict
//                                mean / var            queue_predict_reduce (only when asked for), BEFORE V is overwritten
//                                W = L^-T V            the backward substitution of gphip_solve on the same rows, in place (dvar only)
//                                predict_xgrad_kernel  both gradients from one pass over the distances, strips of training points
//                                predict_xgrad_finish_kernel   strips added in order, / l_c, signs
//   once per call                alpha = K^-1 (y - m)  queue_alpha (the single-vector backward launch, or the row route)
#include "gp_xgrad.h"

namespace {

// The reduction over the contraction points of context h (its scaled training inputs dXs / dXs2, all h->N of them) for the mc test
// points staged in dXsS / dXsS2 (leading dimension mpad): weights W (mpad x Npad, W(t, j) at W[j mpad + t]; read only when var) and
// the broadcast vector a [N].  Results: dXgOut = [dmean (mc x d, row-major)] [dvar (the same, at mpad d)].
// Strip rule: whole slabs of XG_TS points, strips x test tiles >= 2 workgroups per CU while there are slabs; split > 0 forces
// that many strips (at most one per slab).  *nsplit_out: the strips used.
template <typename T>
int queue_xgrad(gphip_ctx* h, const void* W, const void* a_vec, int64_t mc, int64_t mpad, bool var, int split, int* nsplit_out) {
    XGradArgs<T> a{};
    a.W = (const T*)W; a.ldw = (long)mpad; a.a = (const T*)a_vec;
    a.xt = (const T*)h->dXsS.p; a.xt2 = (const T*)h->dXsS2.p; a.ldt = (int)mpad;
    a.xc = (const T*)h->dXs.p; a.xc2 = (const T*)h->dXs2.p; a.ldc = (int)h->Npad;
    a.ntest = (int)mc; a.ncon = (int)h->N; a.d = (int)h->d; a.d0 = 0;
    a.slotp = h->dSlotp.as<double>(); a.ks = h->ks; a.mpad = (int)mpad;
    const int Mt = (int)(mpad / TB), nterm = h->ks.op != 0 ? 2 : 1, nv = var ? 2 : 1, d = a.d;
    const int64_t nslabs = (h->N + XG_TS - 1) / XG_TS;
    int64_t nstrips = split > 0 ? std::min<int64_t>(split, nslabs) : std::min<int64_t>(nslabs, (2l * std::max(h->ncu, 1) + Mt - 1) / Mt);
    const int64_t strip_slabs = (nslabs + nstrips - 1) / nstrips;
    nstrips = (nslabs + strip_slabs - 1) / strip_slabs;
    a.strip_cols = (int)(strip_slabs * XG_TS);
    *nsplit_out = (int)nstrips;
    const long md = (long)mpad * d;
    HIPCHK(h->dXgPart.grow((size_t)(nstrips * nterm * nv) * md * 8));
    HIPCHK(h->dXgOut.grow((size_t)2 * md * 8));
    a.part = h->dXgPart.as<double>();
    const dim3 grid((unsigned)Mt, (unsigned)nstrips);
    // profile class 6 (prediction epilogue): flops = the accumulations, 2 per coordinate, term and weight; bytes = W once
    ProfScope ps(h, 6, 2.0 * d * nterm * nv * (double)mpad * (double)h->N, var ? (double)sizeof(T) * mpad * h->Npad : 0.0);
#define XG_GO(DW, GLB, TWO)                                                                                                            \
    do {                                                                                                                               \
        if (var) hipLaunchKernelGGL((predict_xgrad_kernel<T, DW, GLB, TWO, true>), grid, dim3(TB), (predict_xgrad_lds<T, DW, GLB>(TWO ? 2 : 1)), h->stream, a);  \
        else hipLaunchKernelGGL((predict_xgrad_kernel<T, DW, GLB, TWO, false>), grid, dim3(TB), (predict_xgrad_lds<T, DW, GLB>(TWO ? 2 : 1)), h->stream, a);     \
    } while (0)
#define XG_LAUNCH(DW, GLB)                                                                                                             \
    do {                                                                                                                               \
        if (nterm == 2) XG_GO(DW, GLB, true);                                                                                          \
        else XG_GO(DW, GLB, false);                                                                                                    \
    } while (0)
    if (d <= 2) XG_LAUNCH(2, false);
    else if (d <= 4) XG_LAUNCH(4, false);
    else if (d <= 8) XG_LAUNCH(8, false);
    else if (d <= 16) XG_LAUNCH(16, false);
    else if (d <= KB_LDS_MAXD && nterm == 1) XG_GO(32, false, false);
    else                                       // (two terms beyond 16 dimensions: 4 x 32 accumulators would not stay in registers)
        for (a.d0 = 0; a.d0 < d; a.d0 += 16) XG_LAUNCH(16, true);      // the points from global memory, a window of 16 coordinates per launch
#undef XG_LAUNCH
#undef XG_GO
    const long n = (long)mc * d;
    hipLaunchKernelGGL(predict_xgrad_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, (const double*)a.part,
                       (int)nstrips, nterm, nv, md, n, d, (const double*)h->dInvEll.as<double>(),
                       (const double*)(nterm == 2 ? h->dInvEll2.as<double>() : nullptr), h->dXgOut.as<double>(),
                       var ? h->dXgOut.as<double>() + md : nullptr);
    return GPHIP_OK;
}

// the statuses of both gradient calls that depend on the exact context's state (no device work)
int xgrad_kernel_check(gphip_ctx* h) {
    if (h->custom) return fail(h, GPHIP_ERR_UNSUPPORTED, "no gradient in the test inputs for a run-time compiled covariance function");
    return GPHIP_OK;
}

// the chunk of test points: option predict_grad_chunk n > 0 = n points rounded up to whole tiles, else gphip_predict's rule, halved
// beyond 2048 rows (the partials and the gradient block sit next to V)
int xgrad_chunk(gphip_ctx* h, int64_t M, int64_t* rows) {
    const int64_t want = h->predict_grad_chunk > 0 ? h->predict_grad_chunk : M;
    int64_t MC = 0;
    const int rc = ensure_vchunk(h, std::min<int64_t>(32768, (want + TB - 1) / TB * TB), &MC);
    if (rc) return rc;
    if (h->predict_grad_chunk <= 0 && MC > 2048) MC = (MC / 2 + TB - 1) / TB * TB;
    h->predict_grad_chunk_last = (int)MC;
    *rows = MC;
    return GPHIP_OK;
}

}  // namespace

extern "C" {

int gphip_predict_grad(gphip_handle h, const void* Xs, int64_t M, double* mean, double* var, double* dmean, double* dvar) {
    if (!h || !Xs || !dmean) return fail(h, GPHIP_ERR_ARG, "null argument");
    if (M < 1) return fail(h, GPHIP_ERR_DIM, "M < 1");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (!has_fit(h)) return fail(h, GPHIP_ERR_STATE, "gphip_predict_grad before a successful gphip_fit");
    if (int rc = xgrad_kernel_check(h)) return rc;
    if (h->fit_pw) return fail(h, GPHIP_ERR_UNSUPPORTED, "gphip_predict_grad after gphip_fit_pw with a point-dependent nugget / mean");
    if (h->dist_fit) return fail(h, GPHIP_ERR_UNSUPPORTED, "gphip_predict_grad from a sharded factor (replicate_factor = 0)");
    const int64_t d = h->d;
    if (h->null_fit) {                             // null kernel: k = 0, the prediction does not depend on x*
        for (int64_t t = 0; t < M; ++t) {
            if (mean) mean[t] = h->mu_fit;
            if (var) var[t] = h->kappa_fit;
        }
        for (int64_t e = 0; e < M * d; ++e) {
            dmean[e] = 0.0;
            if (dvar) dvar[e] = 0.0;
        }
        return GPHIP_OK;
    }
    HIPCHK(hipSetDevice(h->device));
    const double* X = static_cast<const double*>(Xs);
    int64_t MC = 0;
    int rc = xgrad_chunk(h, M, &MC);
    if (rc) return rc;
    HIPCHK(h->dAlpha.grow((size_t)h->Npad * h->es));
    if ((rc = DISPATCH(h, queue_alpha, h))) return rc;        // (its row route borrows dV: before the first chunk is staged)
    std::vector<double> xt;
    for (int64_t m0 = 0; m0 < M; m0 += MC) {
        const int64_t mc = (M - m0 < MC) ? (M - m0) : MC;
        const int64_t mpad = stage_test_chunk(h, X, m0, mc, 1, 0, xt, &rc);
        if (rc) return rc;
        const bool df_fwd = queue_forward_fit(h, mpad);
        if (mean || var) {
            if ((rc = DISPATCH(h, queue_predict_reduce, h, mc, mpad, 1))) return rc;
            if (mean) HIPCHK(hipMemcpyAsync(mean + m0, h->dMean.p, (size_t)mc * 8, hipMemcpyDeviceToHost, h->stream));
            if (var) HIPCHK(hipMemcpyAsync(var + m0, h->dVar.p, (size_t)mc * 8, hipMemcpyDeviceToHost, h->stream));
        }
        if (dvar) {                                // V <- V L^-1 in place, the route of gphip_solve
            if (df_fwd && df_backward_ready<double>(h)) launch_dataflow_inverse<double, 64>(h, mpad, true);
            else DISPATCH(h, queue_backward_rows, h, mpad);
        }
        if ((rc = DISPATCH(h, queue_xgrad, h, h->dV.p, h->dAlpha.p, mc, mpad, dvar != nullptr, h->predict_grad_split, &h->predict_grad_nsplit)))
            return rc;
        const double* out = h->dXgOut.as<double>();
        HIPCHK(hipMemcpyAsync(dmean + m0 * d, out, (size_t)(mc * d) * 8, hipMemcpyDeviceToHost, h->stream));
        if (dvar) HIPCHK(hipMemcpyAsync(dvar + m0 * d, out + mpad * d, (size_t)(mc * d) * 8, hipMemcpyDeviceToHost, h->stream));
        if ((rc = complete_call(h))) return rc;
    }
    return GPHIP_OK;
}

}  // extern "C"
