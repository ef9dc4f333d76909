// gphip_sparse_paths.inc -- pathwise posterior function draws of the sparse object (include/gphip.h: gphip_sparse_paths_create /
// _get; DESIGN.md section 8o).  Included at the end of gphip.hip, behind gphip_paths.inc.  The result is an ordinary gphip_paths:
// its contraction side is Z (raw Z, 1 / l, the slot scalars of the K_uu context, v), so gphip_paths_eval / _eval_own / _shape /
// _get / _destroy serve it with the kernels of the exact object and no branch in them.  What is here is Matheron's rule for the
// collapsed bound's optimal q(u) at creation: with u' = L_u^-1 u ~ N(L_B^-T c, sn^2 L_B^-T L_B^-1),
//     v_s = L_u^-T [ L_B^-T (c + sn xi_s) - L_u^-1 (f~_s(Z) + sqrt(j) zeta_s) ]
// (sqrt(j) zeta: K_uu holds the jitter, so the prior value conditioned on must have covariance K_uu, not k(Z, Z)).
//
//   u's stream  gphip_rff_table(fitted theta) -> Omega, b, a;  paths_weights_kernel;  paths_contract_kernel<GenFeature> at Z
//               sparse_paths_prior_kernel     -(f~(Z) + sqrt(j) zeta) into u's vector block (strips in order)
//               queue_forward_fit             L_u^-1 (..)
//   b's stream  waits for an event of u's (not the host: see sparse_paths_create_device)
//               sparse_paths_rhs_kernel       c + sn xi into b's vector block (c: b's rhs row)
//               queue_backward_rows           L_B^-T (..)
//   u's stream  waits for an event of b's (not the host);  sparse_paths_join_kernel: u's block += b's
//               queue_backward_rows, refined  L_u^-T (..) with the diagonal solves refined once (dLd / dRes, as
//                                             gphip_sparse_predict_grad: the two terms cancel as cond(K_uu) grows)
//               copy into the object, paths_finite_kernel
// Neither N nor V appears: O(m^2 S + m Ftot S).  Fixed summation order, no atomics.  The fit is read only.
// Locks: the sparse object's mutex, then the K_uu context's (PathsLock, gphip_paths.inc).  The object counts in u->paths_live:
// gphip_sparse_destroy and a gphip_sparse_set_inducing that changes m are refused while it is above zero.
#include "gp_sparse_paths.h"

namespace {

constexpr int RFF_TAG_XI = 10, RFF_TAG_ZETA = 11;     // (documented beside the table's tags in gphip_hostlogic.inc)

// the device part of gphip_sparse_paths_create (both mutexes held): *nan_out = a non-finite v
template <typename T>
int sparse_paths_create_device(gphip_sparse_ctx* h, gphip_paths* q, bool* nan_out) {
    gphip_ctx *u = h->u, *b = h->b;
    const int64_t m = q->N, mpad = q->Npad, d = q->d, Ftot = q->Ftot, Spad = q->Spad;
    const int S = q->S;
    HIPCHK(hipSetDevice(u->device));
    HIPCHK(q->dXt.grow((size_t)d * mpad * 8));
    HIPCHK(q->dIe1.grow((size_t)d * 8));
    HIPCHK(q->dIe2.grow((size_t)d * 8));
    HIPCHK(q->dSlotp.grow((size_t)SLOTP * 8));
    HIPCHK(q->dOmT.grow((size_t)d * Ftot * 8));
    HIPCHK(q->dPhase.grow((size_t)Ftot * 8));
    HIPCHK(q->dWa.grow((size_t)Ftot * Spad * sizeof(T)));
    HIPCHK(q->dW.grow((size_t)S * Ftot * 8));
    HIPCHK(q->dEps.grow((size_t)S * m * 8));
    HIPCHK(q->dXi.grow((size_t)S * m * 8));
    HIPCHK(q->dZeta.grow((size_t)S * m * 8));
    HIPCHK(q->dV.grow((size_t)mpad * Spad * sizeof(T)));
    HIPCHK(q->dFlag.grow(8 + 8 * (size_t)Ftot));               // [0]: the flag word; then amp staging
    HIPCHK(h->dLd.grow((size_t)u->Nt * TS * sizeof(T)));
    HIPCHK(h->dRes.grow((size_t)Spad * TB * sizeof(T)));
    int rc;
    if ((rc = ensure_vbuf(u, Spad))) { (void)hipGetLastError(); return sfail(h, rc, "no device memory for the draws' vector block: " + u->err); }
    if ((rc = ensure_vbuf(b, Spad))) { (void)hipGetLastError(); return sfail(h, rc, "no device memory for the draws' vector block: " + b->err); }
    std::vector<double> zt((size_t)d * mpad, 0.0), omt((size_t)d * Ftot);
    for (int64_t i = 0; i < m; ++i)
        for (int64_t c = 0; c < d; ++c) zt[(size_t)c * mpad + i] = u->hostX[(size_t)i * d + c];
    for (int64_t j = 0; j < Ftot; ++j)
        for (int64_t c = 0; c < d; ++c) omt[(size_t)c * Ftot + j] = q->omega[(size_t)j * d + c];
    hipStream_t su = u->stream, sb = b->stream;
    HIPCHK(hipMemcpyAsync(q->dXt.p, zt.data(), zt.size() * 8, hipMemcpyHostToDevice, su));
    HIPCHK(hipMemcpyAsync(q->dOmT.p, omt.data(), omt.size() * 8, hipMemcpyHostToDevice, su));
    HIPCHK(hipMemcpyAsync(q->dPhase.p, q->phase.data(), (size_t)Ftot * 8, hipMemcpyHostToDevice, su));
    // the fit's own staged hyper-parameters (slot 0 of the K_uu context), as its kernel build read them
    HIPCHK(hipMemcpyAsync(q->dIe1.p, u->dInvEll.p, (size_t)d * 8, hipMemcpyDeviceToDevice, su));
    if (q->two) HIPCHK(hipMemcpyAsync(q->dIe2.p, u->dInvEll2.p, (size_t)d * 8, hipMemcpyDeviceToDevice, su));
    HIPCHK(hipMemcpyAsync(q->dSlotp.p, u->dSlotp.p, (size_t)SLOTP * 8, hipMemcpyDeviceToDevice, su));
    double* stage = q->dFlag.as<double>() + 1;
    HIPCHK(hipMemsetAsync(q->dFlag.p, 0, 8, su));
    HIPCHK(hipMemcpyAsync(stage, q->amp.data(), (size_t)Ftot * 8, hipMemcpyHostToDevice, su));
    HIPCHK(hipMemsetAsync(q->dWa.p, 0, (size_t)Ftot * Spad * sizeof(T), su));
    const long nw = (long)S * Ftot;
    hipLaunchKernelGGL(paths_weights_kernel<T>, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, su, q->dW.as<double>(), (T*)q->dWa.p,
                       (const double*)stage, S, (long)Ftot, (long)Spad, q->seed);
    HIPCHK(hipStreamSynchronize(su));                          // (zt, omt: the copies have read the host vectors)
    const auto t_feat = std::chrono::steady_clock::now();
    int nsf = 0;
    if ((rc = queue_paths_contract<T>(q, false, false, q->dXt.as<double>(), (long)mpad, m, q->dPartF, u->paths_split, &nsf))) return sfail(h, rc, u->err);
    const long nv = (long)mpad * Spad;
    const unsigned gv = (unsigned)((nv + 255) / 256);
    hipLaunchKernelGGL(sparse_paths_prior_kernel<T>, dim3(gv), dim3(256), 0, su, (const double*)q->dPartF.p, nsf, S, (long)m, (long)mpad,
                       std::sqrt(h->jit_fit), rff_key(q->seed, RFF_TAG_ZETA), q->dZeta.as<double>(), q->dEps.as<double>(), (T*)u->dV.p,
                       (long)Spad);
    HIPCHK(hipStreamSynchronize(su));
    u->paths_feature_us = paths_us(t_feat);
    const auto t_sub = std::chrono::steady_clock::now();
    // The two streams hand over through events, not the host.  b starts behind u's forward substitution: where that is the
    // dataflow launch it spin-waits, and no call of the sparse object runs such a launch beside work of the other context.
    struct Handed { gphip_ctx* u; hipEvent_t e; ~Handed() { u->pool.push_back(e); } } fwd{u, get_event(u)}, back{u, get_event(u)};
    queue_forward_fit(u, Spad);
    HIPCHK(hipEventRecord(fwd.e, su));
    HIPCHK(hipStreamWaitEvent(sb, fwd.e, 0));
    hipLaunchKernelGGL(sparse_paths_rhs_kernel<T>, dim3(gv), dim3(256), 0, sb, (const T*)b->dA.p, (int)b->R, S, (long)m, (long)mpad,
                       std::sqrt(h->sn2_fit), rff_key(q->seed, RFF_TAG_XI), q->dXi.as<double>(), (T*)b->dV.p, (long)Spad);
    if ((rc = queue_backward_rows<T>(b, Spad))) return sfail(h, rc, b->err);
    HIPCHK(hipEventRecord(back.e, sb));
    HIPCHK(hipStreamWaitEvent(su, back.e, 0));
    hipLaunchKernelGGL(sparse_paths_join_kernel<T>, dim3((unsigned)std::min<long>((nv + 255) / 256, 4096)), dim3(256), 0, su, (T*)u->dV.p,
                       (const T*)b->dV.p, nv);
    if ((rc = queue_backward_rows<T>(u, Spad, u->dV.p, h->dLd.p, h->dRes.p))) return sfail(h, rc, u->err);
    HIPCHK(hipMemcpyAsync(q->dV.p, u->dV.p, (size_t)nv * sizeof(T), hipMemcpyDeviceToDevice, su));
    hipLaunchKernelGGL(paths_finite_kernel<T>, dim3(1024), dim3(256), 0, su, (const T*)q->dV.p, nv, reinterpret_cast<int*>(q->dFlag.p));
    int flag = 0;
    rc = complete_call(u, [&]() -> int {
        HIPCHK(hipMemcpyAsync(&flag, q->dFlag.p, sizeof(int), hipMemcpyDeviceToHost, su));
        HIPCHK(hipStreamSynchronize(su));
        return GPHIP_OK;
    });
    if (rc) return sfail(h, rc, u->err);
    if ((rc = complete_call(b))) return sfail(h, rc, b->err);  // (u's stream waited for b's: it is idle)
    u->paths_subst_us = paths_us(t_sub);
    *nan_out = flag != 0;
    q->dPartF.release();                                       // (m-sized: an evaluation sizes its own)
    return GPHIP_OK;
}

}  // namespace

extern "C" {

int gphip_sparse_paths_create(gphip_sparse_handle h, int S, int F, uint64_t seed, gphip_paths_handle* out, int* info) {
    if (out) *out = nullptr;
    if (!h || !out || !info) return sfail(h, GPHIP_ERR_ARG, "null argument");
    *info = GPHIP_INFO_OK;
    if (S < 1 || F < 1 || S > PATHS_MAX_S) return sfail(h, GPHIP_ERR_DIM, "S < 1, F < 1 or S > 2048");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    gphip_ctx *u = h->u, *b = h->b;
    if (!h->fitted || !has_fit(u) || !has_fit(b)) return sfail(h, GPHIP_ERR_STATE, "gphip_sparse_paths_create before a successful gphip_sparse_fit");
    if (h->custom) return sfail(h, GPHIP_ERR_UNSUPPORTED, "no spectral law is known for a run-time compiled covariance function");
    if (h->pw_fit) return sfail(h, GPHIP_ERR_UNSUPPORTED, "gphip_sparse_paths_create after a fit with a point-dependent nugget / mean array");
    std::lock_guard<std::recursive_mutex> lku(u->mu);
    const auto t0 = std::chrono::steady_clock::now();
    gphip_paths* q = new gphip_paths;
    q->h = u; q->sp = h; q->S = S; q->F = F; q->seed = seed;
    q->N = u->N; q->Npad = u->Npad; q->d = u->d; q->Spad = ((int64_t)S + TB - 1) / TB * TB;
    q->mu = h->mu_fit;
    const std::vector<double>& th = u->theta_fit;
    const int p = (int)th.size();
    int rc = gphip_rff_table(h->kernel_id, h->d, th.data(), p, F, seed, &q->Ftot, nullptr, nullptr, nullptr);
    if (!rc && q->Ftot * S > PATHS_MAX_FS) rc = GPHIP_ERR_DIM;
    if (!rc) {
        q->omega.resize((size_t)q->Ftot * q->d); q->phase.resize((size_t)q->Ftot); q->amp.resize((size_t)q->Ftot);
        rc = gphip_rff_table(h->kernel_id, h->d, th.data(), p, F, seed, &q->Ftot, q->omega.data(), q->phase.data(), q->amp.data());
    }
    if (rc) {
        delete q;
        return sfail(h, rc, rc == GPHIP_ERR_DIM ? "Ftot x S above 2^26" : "no feature table for the fitted kernel (a negative constant offset?)");
    }
    q->ks = u->ks; q->two = u->ks.op != 0;
    q->sn = std::sqrt(h->sn2_fit);
    bool nan = false;
    rc = DISPATCH(h, sparse_paths_create_device, h, q, &nan);
    if (rc || nan) {
        (void)hipSetDevice(u->device);
        delete q;
        if (rc) return rc;
        *info = GPHIP_INFO_NAN;
        return GPHIP_OK;
    }
    ++u->paths_live;
    *out = q;
    u->paths_create_us = paths_us(t0);
    return GPHIP_OK;
}

int gphip_sparse_paths_get(gphip_paths_handle q, double* xi, double* zeta) {
    if (!q || !q->sp) return GPHIP_ERR_ARG;
    gphip_sparse_ctx* h = q->sp;
    PathsLock lk(q);
    HIPCHK(hipSetDevice(q->h->device));
    hipStream_t st = q->h->stream;
    const size_t bytes = (size_t)q->S * q->N * 8;
    if (xi) HIPCHK(hipMemcpyAsync(xi, q->dXi.p, bytes, hipMemcpyDeviceToHost, st));
    if (zeta) HIPCHK(hipMemcpyAsync(zeta, q->dZeta.p, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return GPHIP_OK;
}

}  // extern "C"
