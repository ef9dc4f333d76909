// gphip_joint.inc -- joint predictive distribution of the current fit (include/gphip.h: gphip_predict_cov, gphip_predict_draws,
// gphip_predict_logpdf).  Included at the end of gphip.hip.
//
//   parent (the fitted handle)   V = L^-1 K(X, X*)    queue_cross + the forward substitution of gphip_predict, all M rows at once
//                                Z = [z^T; 0]         z = L^-1 r gathered from the factor's rhs tile row
//   child  (h->joint)            a context whose TRAINING points are X*, same kernel / theta / dtype, y = y* (or 0):
//                                queue_build         C = K(X*, X*) + nugget (+ jitter), rhs row = y* - m(X*)
//                                downdate_kernel     C -= [V; z^T] V^T   -> Sigma, rhs row = y* - mu
//                                queue_factor        L_Sigma, log det Sigma, (y* - mu)^T Sigma^-1 (y* - mu)   (draws / logpdf)
// The child is made on the first call and kept while M stays the same (its points and y are uploaded again per call); it dies
// with the parent.  It never runs the fused single-launch evaluation (h->fused_eval: that one builds K inside the factorisation).
// The sparse object (gphip_sparse.inc) owns such a child through its inducing-point context: joint_build, queue_downdate_any
// and the joint_*_tail functions below take the owning context, whichever object it belongs to.
#include "gp_joint.h"

namespace {

constexpr int64_t JOINT_MAX_M = GPHIP_JOINT_MAX_M;
// default jitter, relative to the prior variance k(x*, x*) + sn^2: far above the rounding of Sigma, and above the factorisation's
// pivot tolerance (64 eps, pivot_tol_rel) -- fp32: 7.6e-6, so 1e-6 would still leave a smooth latent Sigma "not SPD"
double joint_jitter_rel(const gphip_ctx* h) { return h->dtype == 64 ? 1e-10 : 1e-4; }

int joint_common_checks(gphip_ctx* h) {
    if (!has_fit(h)) return fail(h, GPHIP_ERR_STATE, "joint prediction before a successful gphip_fit");
    if (h->dist_fit) return fail(h, GPHIP_ERR_UNSUPPORTED, "joint prediction from a sharded factor (replicate_factor = 0)");
    if (h->fit_pw) return fail(h, GPHIP_ERR_UNSUPPORTED, "joint prediction after gphip_fit_pw with a point-dependent nugget / mean");
    return GPHIP_OK;
}

int joint_dim_check(gphip_ctx* h, int64_t M) {
    if (M < 1) return fail(h, GPHIP_ERR_DIM, "M < 1");
    if (M > JOINT_MAX_M) return fail(h, GPHIP_ERR_DIM, "M above GPHIP_JOINT_MAX_M (all rows of V must be resident at once)");
    return GPHIP_OK;
}

// the child context for M test points at Xs with outputs y (nullptr: zeros)
int joint_child(gphip_ctx* h, const double* Xs, int64_t M, const double* y) {
    std::vector<double> y0;
    if (!y) { y0.assign((size_t)M, 0.0); y = y0.data(); }
    gphip_ctx* c = h->joint;
    if (c && c->N != M) {
        gphip_destroy(c);
        h->joint = c = nullptr;
    }
    if (!c) {
        gphip_handle out = nullptr;
        std::string why;
        const int rc = create_ctx(Xs, y, M, h->d, h->custom ? (int)GPHIP_KERNEL_CUSTOM : h->kernel_id, h->mean_id, h->dtype, h->device,
                                  &out, h->custom ? h->custom_body.c_str() : nullptr, h->ncp, &why);
        (void)hipSetDevice(h->device);
        if (rc) return fail(h, rc, ("joint prediction: creating the test-point context failed " + why).c_str());
        c = h->joint = out;
        c->kbuild_mfma = 0;                    // K(X*, X*) by the direct build: its diagonal is k(x, x) to the last bit
    } else {
        std::vector<double> xt((size_t)h->d * c->Npad, 0.0), yp((size_t)c->Npad, 0.0);
        for (int64_t i = 0; i < M; ++i) {
            for (int64_t j = 0; j < h->d; ++j) xt[(size_t)j * c->Npad + i] = Xs[i * h->d + j];
            yp[(size_t)i] = y[i];
        }
        c->hostX.assign(Xs, Xs + (size_t)M * (size_t)h->d);       // (the host copy stays what the device holds)
        c->hostY.assign(y, y + (size_t)M);
        int rc = DISPATCH(c, upload, c, c->dXt.p, xt, c->stream);
        if (!rc) rc = DISPATCH(c, upload, c, c->dY.p, yp, c->stream);
        if (rc) return fail(h, rc, c->err.c_str());
    }
    const int rc = ensure_slots(c, 1);
    if (rc) return fail(h, rc, c->err.c_str());
    return GPHIP_OK;
}

// k(x*, x*) of a run-time compiled kernel averaged over the test points (the default jitter's scale)
int joint_mean_kss(gphip_ctx* h, int64_t M, int64_t mpad, double* out) {
    int rc = queue_custom_kss(h, M, mpad, 1);         // (the test points are in dXsT)
    if (rc) return rc;
    std::vector<double> k((size_t)M);
    HIPCHK(hipMemcpyAsync(k.data(), h->dKss.p, (size_t)M * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    double s = 0.0;
    for (double v : k) s += v;
    *out = s / (double)M;
    return GPHIP_OK;
}

// C -= [V; z^T] V^T on the child's workspace, in the strips of strip_split (gp_contract.h).
// SEG (the sparse object): h->dV holds [V1 | V2], the contraction runs over the stacked index of 2 x h->Npad columns and sn2
// scales the second segment (gp_joint.h); split > 0 forces that many strips; *nsplit_out: the strips used.
template <typename T, bool SEG>
int queue_downdate_any(gphip_ctx* h, gphip_ctx* c, int64_t mpad, int split, int* nsplit_out, double sn2) {
    DowndateArgs<T> g{};
    g.C = (T*)c->dA.p; g.R = (int)c->R;
    g.V = (const T*)h->dV.p; g.ldv = (long)mpad; g.Z = (const T*)h->dJZ.p;
    g.Mt = (int)(mpad / TB); g.ntri = g.Mt * (g.Mt + 1) / 2; g.ntiles = g.ntri + g.Mt;
    g.K = (int)(SEG ? 2 * h->Npad : h->Npad);
    int strip_tiles;
    const int nsplit = strip_split(g.ntiles, (int)(SEG ? 2 * h->Nt : h->Nt), split, h->ncu, &strip_tiles);
    g.kstrip = strip_tiles * TB;
    *nsplit_out = nsplit;
    if (nsplit > 1) {
        HIPCHK(h->dJPart.grow((size_t)nsplit * g.ntiles * TS * sizeof(T)));
        g.P = (T*)h->dJPart.p;
    }
    if (SEG) {                                 // accumulators that start at C take the update itself, a partial tile its negative
        g.kseg = (int)h->Npad;
        g.s1 = (T)(nsplit > 1 ? 1.0 : -1.0);
        g.s2 = (T)(nsplit > 1 ? -sn2 : sn2);
    }
    {
        // algorithmic flops M (M + 1) N (the lower triangle and the rhs row of an M x M downdate of contraction length N)
        ProfScope ps(c, 4, (double)mpad * (mpad + 1) * (double)(SEG ? 2 * h->N : h->N), (double)sizeof(T) * (mpad + TB) * (double)g.K);
        hipLaunchKernelGGL((downdate_kernel<T, SEG>), dim3((unsigned)g.ntiles, (unsigned)nsplit), dim3(256), StridedK<T>::LDS, c->stream, g);
        if (nsplit > 1)
            hipLaunchKernelGGL(strip_reduce_kernel<T>, dim3((unsigned)g.ntiles, 16), dim3(256), 0, c->stream, g.C, g.R, g.ntri, g.Mt,
                               g.ntiles, (const T*)g.P, nsplit, -1.0, 0l, 0l);
    }
    return GPHIP_OK;
}
template <typename T>
int queue_downdate(gphip_ctx* h, gphip_ctx* c, int64_t mpad) {
    return queue_downdate_any<T, false>(h, c, mpad, h->joint_split, &h->joint_nsplit, 0.0);
}

// The child of h (made by joint_child): K(X*, X*) at h's fitted theta with (noisy: sn^2) + (*jitter_io, which a negative value
// turns into the default first; kss_mean: the mean of k(x*, x*) of a run-time compiled kernel) on the diagonal, rhs row
// y* - m(X*), queued on the child's stream.
int joint_build(gphip_ctx* h, bool noisy, double* jitter_io, double kss_mean) {
    int rc;
    gphip_ctx* c = h->joint;
    HIPCHK(hipSetDevice(c->device));
    invalidate_fit(c);
    if (!stage_theta(c, 0, h->theta_fit.data())) return fail(h, GPHIP_ERR_ARG, "the fitted theta does not stage");
    const double sn2 = c->hSlotp.as<double>()[1];
    if (jitter_io && *jitter_io < 0.0)                // default jitter: relative to the prior variance k(x*, x*) + sn^2
        *jitter_io = joint_jitter_rel(h) * ((h->custom ? kss_mean : c->hSlotp.as<double>()[SP_KXX]) + sn2);
    c->hSlotp.as<double>()[1] = (noisy ? sn2 : 0.0) + (jitter_io ? *jitter_io : 0.0);
    c->hSlotp.as<double>()[SP_MFMA] = 0.0;
    if ((rc = copy_theta(c, 1))) return fail(h, rc, c->err.c_str());
    HIPCHK(hipMemsetAsync(c->dInfo.p, 0, 4, c->stream));
    c->theta_packed = false; c->fused_eval = false;      // (want_w / want_u: no FactorMode is ever open on the child)
    DISPATCH(c, queue_build, c, 1);
    return GPHIP_OK;
}

// Everything up to Sigma in the child's workspace: V and z on the parent, then build + downdate on the child.  The child's
// diagonal carries k(x*, x*) + (noisy: sn^2) + (*jitter_io, which a negative value turns into the default first).
int joint_sigma(gphip_ctx* h, const double* Xs, int64_t M, const double* ystar, bool noisy, double* jitter_io) {
    HIPCHK(hipSetDevice(h->device));
    const int64_t mpad = (M + TB - 1) / TB * TB;
    int rc = ensure_vbuf(h, mpad);
    if (rc) { (void)hipGetLastError(); return fail(h, GPHIP_ERR_HIP, "joint prediction: no device memory for all M rows of V"); }
    HIPCHK(h->dJZ.grow((size_t)TB * h->Npad * h->es));
    HIPCHK(hipMemsetAsync(h->dJZ.p, 0, (size_t)TB * h->Npad * h->es, h->stream));
    std::vector<double> xt;
    stage_test_chunk(h, Xs, 0, M, 1, 0, xt, &rc);         // all M rows as one chunk
    if (rc) return rc;
    queue_forward_fit(h, mpad);
    if (h->dtype == 64)
        hipLaunchKernelGGL(gather_rhs_row_kernel<double>, dim3((unsigned)((h->Npad + 255) / 256)), dim3(256), 0, h->stream,
                           (const double*)h->dA.p, (int)h->R, 0, (int)h->Npad, (double*)h->dJZ.p, (long)TB, 0);
    else
        hipLaunchKernelGGL(gather_rhs_row_kernel<float>, dim3((unsigned)((h->Npad + 255) / 256)), dim3(256), 0, h->stream,
                           (const float*)h->dA.p, (int)h->R, 0, (int)h->Npad, (float*)h->dJZ.p, (long)TB, 0);
    double kss_mean = 0.0;                            // (run-time compiled kernels: k(x*, x*) is a function of the point)
    if (jitter_io && *jitter_io < 0.0 && h->custom && (rc = joint_mean_kss(h, M, mpad, &kss_mean))) return rc;
    if ((rc = complete_call(h))) return rc;           // (the forward substitution's abort word)
    if ((rc = joint_child(h, Xs, M, ystar))) return rc;
    if ((rc = joint_build(h, noisy, jitter_io, kss_mean))) return rc;
    return DISPATCH(h, queue_downdate, h, h->joint, mpad);
}

// the child's rhs row -> out[M] (y* = 0: the predictive mean)
template <typename T>
int queue_joint_rhs(gphip_ctx* c, int64_t M, double* out) {
    hipLaunchKernelGGL(joint_rhs_kernel<T>, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, c->stream, (const T*)c->dA.p, (int)c->R, (int)M,
                       (const double*)nullptr, out);
    return GPHIP_OK;
}

// the child's factorisation; *info as gphip_loglik's (ev: two events to record around it on the child's stream, or null)
int joint_factor(gphip_ctx* h, int* info, hipEvent_t* ev = nullptr) {
    gphip_ctx* c = h->joint;
    if (ev) (void)hipEventRecord(ev[0], c->stream);
    DISPATCH(c, queue_factor, c, 1);
    if (ev) (void)hipEventRecord(ev[1], c->stream);
    c->abort_unread = "joint prediction: the factorisation of Sigma timed out (set option dataflow=0 and report)";
    const int rc = complete_call(c);
    if (rc) return fail(h, rc, c->err.c_str());
    *info = c->hInfo.as<int>()[0];
    return GPHIP_OK;
}

int joint_download(gphip_ctx* h, gphip_ctx* c, double* dst, const double* src, size_t n) {
    HIPCHK(hipMemcpyAsync(dst, src, n * 8, hipMemcpyDeviceToHost, c->stream));
    const int rc = complete_call(c);
    return rc ? fail(h, rc, c->err.c_str()) : GPHIP_OK;
}

// Sigma and the rhs row in h's child -> dense cov [M][M] (both triangles) and mean [M] on the host
int joint_cov_tail(gphip_ctx* h, int64_t M, double* mean, double* cov) {
    gphip_ctx* c = h->joint;
    HIPCHK(h->dJOut.grow(((size_t)M * M + (size_t)M) * 8));
    const long n = (long)M * M;
    if (h->dtype == 64) {
        hipLaunchKernelGGL(joint_unpack_kernel<double>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->dA.p,
                           (int)c->R, (int)M, h->dJOut.as<double>());
    } else {
        hipLaunchKernelGGL(joint_unpack_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (const float*)c->dA.p,
                           (int)c->R, (int)M, h->dJOut.as<double>());
    }
    DISPATCH(c, queue_joint_rhs, c, M, h->dJOut.as<double>() + n);
    HIPCHK(hipMemcpyAsync(mean, h->dJOut.as<double>() + n, (size_t)M * 8, hipMemcpyDeviceToHost, c->stream));
    return joint_download(h, c, cov, h->dJOut.as<double>(), (size_t)n);
}

// Sigma (+ jitter) and the rhs row (-mu, y* = 0) in h's child -> S draws [S][M] on the host; *info as gphip_predict_draws'
int joint_draws_tail(gphip_ctx* h, int64_t M, int S, uint64_t seed, const double* z, double* out, int* info, hipEvent_t* ev = nullptr) {
    const size_t total = (size_t)S * (size_t)M;
    gphip_ctx* c = h->joint;
    const int64_t mpad = (M + TB - 1) / TB * TB;
    // the mean (rhs row = -mu with y* = 0) before the factorisation overwrites that row
    HIPCHK(h->dJOut.grow((size_t)mpad * 8));
    DISPATCH(c, queue_joint_rhs, c, M, h->dJOut.as<double>());
    int inf = 0, rc;
    if ((rc = joint_factor(h, &inf, ev))) return rc;
    if (inf != 0) {
        *info = inf;
        for (size_t e = 0; e < total; ++e) out[e] = NAN;
        return GPHIP_OK;
    }
    // draws in chunks of at most ~512 MiB of Z and of out each
    const int sc = (int)std::max<int64_t>(1, std::min<int64_t>(S, ((int64_t)1 << 26) / mpad));
    Buf dZ, dOut;                              // double
    if (dZ.grow((size_t)sc * mpad * 8) != hipSuccess || dOut.grow((size_t)sc * M * 8) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, GPHIP_ERR_HIP, "joint prediction: no device memory for the draws");
    }
    std::vector<double> zh;
    for (int s0 = 0; s0 < S && !rc; s0 += sc) {
        const int ns = std::min(sc, S - s0);
        if (z) {
            zh.assign((size_t)ns * mpad, 0.0);
            for (int s = 0; s < ns; ++s)
                for (int64_t j = 0; j < M; ++j) zh[(size_t)s * mpad + j] = z[(size_t)(s0 + s) * M + j];
            if (hipMemcpyAsync(dZ.p, zh.data(), zh.size() * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = GPHIP_ERR_HIP; break; }
        } else {
            const long n = (long)ns * mpad;
            hipLaunchKernelGGL(joint_normal_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, dZ.as<double>(), (long)mpad, ns, (int)M,
                               s0, (uint64_t)seed);
        }
        const dim3 grid((unsigned)((M + JT_B - 1) / JT_B), (unsigned)((ns + JT_B - 1) / JT_B));
        if (h->dtype == 64)
            hipLaunchKernelGGL(joint_trmm_kernel<double>, grid, dim3(256), 0, c->stream, (const double*)c->dA.p, (int)c->R, (int)M,
                               dZ.as<double>(), (long)mpad, ns, h->dJOut.as<double>(), dOut.as<double>(), (long)M);
        else
            hipLaunchKernelGGL(joint_trmm_kernel<float>, grid, dim3(256), 0, c->stream, (const float*)c->dA.p, (int)c->R, (int)M,
                               dZ.as<double>(), (long)mpad, ns, h->dJOut.as<double>(), dOut.as<double>(), (long)M);
        rc = joint_download(h, c, out + (size_t)s0 * M, dOut.as<double>(), (size_t)ns * M);
    }
    if (rc == GPHIP_ERR_HIP && h->err.empty()) h->err = "joint prediction: copying the normals failed";
    if (rc) return rc;
    for (size_t e = 0; e < total; ++e)
        if (!std::isfinite(out[e])) { *info = GPHIP_INFO_NAN; break; }
    return GPHIP_OK;
}

// Sigma (noisy) and the rhs row y* - mu in h's child -> the joint log density
int joint_logpdf_tail(gphip_ctx* h, int64_t M, double* out, int* info, hipEvent_t* ev = nullptr) {
    int inf = 0;
    if (const int rc = joint_factor(h, &inf, ev)) return rc;
    const gphip_ctx* c = h->joint;
    const double logdet = c->hRes.as<double>()[0], quad = c->hRes.as<double>()[1];
    *out = -0.5 * ((double)M * LOG_TWO_PI + logdet + quad);
    *info = inf != 0 ? inf : (std::isfinite(*out) ? GPHIP_INFO_OK : GPHIP_INFO_NAN);
    return GPHIP_OK;
}

}  // namespace

extern "C" {

int gphip_predict_cov(gphip_handle h, const void* Xs, int64_t M, int latent, double* mean, double* cov) {
    if (!h || !Xs || !mean || !cov) return fail(h, GPHIP_ERR_ARG, "null argument");
    if (int rc = joint_dim_check(h, M)) return rc;
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (int rc = joint_common_checks(h)) return rc;
    if (h->null_fit) {                             // null kernel: k = 0, Sigma = diag(nugget) (latent: 0)
        for (int64_t i = 0; i < M; ++i) {
            mean[i] = h->mu_fit;
            for (int64_t j = 0; j < M; ++j) cov[i * M + j] = (i == j && !latent) ? h->kappa_fit : 0.0;
        }
        return GPHIP_OK;
    }
    const double* X = static_cast<const double*>(Xs);
    int rc = joint_sigma(h, X, M, nullptr, !latent, nullptr);
    if (rc) return rc;
    return joint_cov_tail(h, M, mean, cov);
}

int gphip_predict_draws(gphip_handle h, const void* Xs, int64_t M, int latent, int S, uint64_t seed, const double* z, double jitter,
                        double* out, int* info) {
    if (!h || !Xs || !out || !info) return fail(h, GPHIP_ERR_ARG, "null argument");
    if (!std::isfinite(jitter)) return fail(h, GPHIP_ERR_ARG, "non-finite jitter");
    if (int rc = joint_dim_check(h, M)) return rc;
    if (S < 1) return fail(h, GPHIP_ERR_DIM, "S < 1");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (int rc = joint_common_checks(h)) return rc;
    *info = GPHIP_INFO_OK;
    const size_t total = (size_t)S * (size_t)M;
    if (h->null_fit) {                             // Sigma = diag(nugget) (latent: 0) + jitter: independent draws
        const double jit = jitter < 0.0 ? joint_jitter_rel(h) * h->kappa_fit : jitter;
        const double v = (latent ? 0.0 : h->kappa_fit) + jit;
        if (!(v > 0.0)) {
            *info = GPHIP_INFO_NOT_SPD;
            for (size_t e = 0; e < total; ++e) out[e] = NAN;
            return GPHIP_OK;
        }
        const double sd = std::sqrt(v);
        for (int s = 0; s < S; ++s)
            for (int64_t j = 0; j < M; ++j) {
                const double zz = z ? z[(size_t)s * M + j] : philox_normal(seed, (uint32_t)s, (uint32_t)j);
                out[(size_t)s * M + j] = h->mu_fit + sd * zz;
            }
        for (size_t e = 0; e < total; ++e)
            if (!std::isfinite(out[e])) *info = GPHIP_INFO_NAN;
        return GPHIP_OK;
    }
    const double* X = static_cast<const double*>(Xs);
    double jit = jitter;
    int rc = joint_sigma(h, X, M, nullptr, !latent, &jit);
    if (rc) return rc;
    return joint_draws_tail(h, M, S, seed, z, out, info);
}

int gphip_predict_logpdf(gphip_handle h, const void* Xs, int64_t M, const double* ystar, double* out, int* info) {
    if (!h || !Xs || !ystar || !out || !info) return fail(h, GPHIP_ERR_ARG, "null argument");
    if (int rc = joint_dim_check(h, M)) return rc;
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (int rc = joint_common_checks(h)) return rc;
    for (int64_t j = 0; j < M; ++j)
        if (!std::isfinite(ystar[j])) { *out = NAN; *info = GPHIP_INFO_NAN; return GPHIP_OK; }
    if (h->null_fit) {                             // independent normals N(mu, nugget)
        const double v = h->kappa_fit;
        double q = 0.0;
        for (int64_t j = 0; j < M; ++j) q += (ystar[j] - h->mu_fit) * (ystar[j] - h->mu_fit) / v;
        *out = -0.5 * ((double)M * LOG_TWO_PI + (double)M * std::log(v) + q);
        *info = v > 0.0 ? (std::isfinite(*out) ? GPHIP_INFO_OK : GPHIP_INFO_NAN) : GPHIP_INFO_NOT_SPD;
        return GPHIP_OK;
    }
    int rc = joint_sigma(h, static_cast<const double*>(Xs), M, ystar, true, nullptr);
    if (rc) return rc;
    return joint_logpdf_tail(h, M, out, info);
}

}  // extern "C"
