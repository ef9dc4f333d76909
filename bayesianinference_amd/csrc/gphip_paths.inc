// gphip_paths.inc -- pathwise posterior function draws (include/gphip.h: gphip_paths_create / _eval / _eval_own / _shape / _get /
// _destroy; DESIGN.md sections 8m and 8n).  Included at the end of gphip.hip.  gphip_paths_create serves the exact object; a sparse
// object's draws are created in gphip_sparse_paths.inc and evaluated by the code here as they are (sp below).  Out of scope:
// run-time compiled covariance functions, point-dependent fits, sharding over devices, conditioning a paths object on new data.
//
//   create   gphip_rff_table(fitted theta)             host: Omega, b, a
//            paths_weights_kernel                      w_sj = philox_normal(seed, s, j), Wa = a_j w_sj
//            paths_contract_kernel<GenFeature>         f~_s(x_i) on the training points, strips of features
//            paths_resid_kernel                        r - f~ - eps straight into the vector block dV (eps = sn philox_normal(rff_key(seed, RFF_TAG_EPS), s, i))
//            queue_forward_fit + backward              v = K^-1 (..): the substitutions of gphip_solve on the same block, in place
//            copy                                      v stays in the object, in the vector block's layout (draw index contiguous)
//   eval     per chunk of points: paths_contract_kernel<GenFeature> over the features, <GenKernel> over the training points,
//            paths_finish_kernel (mean + strips in order), one download; with dout the GRAD forms and paths_finish_grad_kernel.
//            The values come from the value launches whether dout is asked for or not: the same bytes.
//   eval_own per chunk of points per draw: paths_own_kernel (gp_paths_own.h; a thread owns one (draw, point) pair) over the
//            features, then over the training points, paths_own_finish_kernel, one download.  With dout the GRAD form leaves the
//            value and the d gradient components of a pair from one generator evaluation; the value is summed in the same order.
// A mixture object (gphip_paths_create_samples, gphip_paths_mix.inc: draws over R hyper-parameter rows) is a gphip_paths too;
// eval and eval_own hand it to paths_mix_eval, everything else here serves it as it is.
// The object owns device copies of all it needs (raw X, 1 / l, slot scalars, Omega, b, Wa, w, eps, v): a later fit of the parent at
// another theta does not touch it.  It borrows the parent's device, stream and mutex and must be destroyed before the parent.
#include "gp_paths.h"
#include "gp_paths_own.h"

struct gphip_paths {
    gphip_ctx* h = nullptr;
    gphip_sparse_ctx* sp = nullptr;                 // a sparse paths object (gphip_sparse_paths.inc): h = sp->u, the contraction points are Z
    int S = 0, F = 0;
    int64_t Ftot = 0, N = 0, Npad = 0, d = 0, Spad = 0;
    uint64_t seed = 0;
    bool null_k = false;
    double mu = 0.0, sn = 0.0;
    KSpec ks{0, 0, 0, 0};
    bool two = false;
    std::vector<double> omega, phase, amp;          // the table, as gphip_rff_table returned it
    Buf dXt;                                        // double [d][Npad] raw training inputs
    Buf dIe1, dIe2, dSlotp;                         // double [d], [d], [SLOTP]
    Buf dOmT, dPhase;                               // double [d][Ftot], [Ftot]
    Buf dWa;                                        // typed [Ftot][Spad]: a_j w_sj
    Buf dW, dEps;                                   // double [S][Ftot], [S][N]
    Buf dXi, dZeta;                                 // double [S][N], [S][N]: the unit normals of a sparse paths object
    Buf dV;                                         // typed [Npad][Spad]: v
    Buf dPartF, dPartK, dXs, dOut, dDout, dFlag;    // scratch of a call
    // a mixture object (gphip_paths_mix.inc): draw s belongs to hyper-parameter row row_of[s] of R; the tables and every buffer
    // that depends on theta hold R rows (omega [R][Ftot][d], dOmT [R][d][Ftot], dIe1 [R][d], dSlotp [R][SLOTP], ..)
    bool mix = false;
    int R = 1;
    std::vector<int> row_of;                        // [S], non-decreasing
    std::vector<double> mu_r;                       // [R] m_r (NaN for a failed row of the null kernel)
    Buf dRowOf, dMu;                                // int [S], double [R]
};

namespace {

constexpr int PATHS_MAX_S = 2048;
constexpr int64_t PATHS_MAX_FS = (int64_t)1 << 26;

// The mutexes of a call on q: the context's, and in front of it the sparse object's when q came from one (its calls hold theirs
// while they work on the context of K_uu).
struct PathsLock {
    std::unique_lock<std::recursive_mutex> outer, inner;
    explicit PathsLock(gphip_paths* q)
        : outer(q->sp ? std::unique_lock<std::recursive_mutex>(q->sp->mu) : std::unique_lock<std::recursive_mutex>()), inner(q->h->mu) {}
};

// the status of a call on q; an error's text is readable through the sparse object too when q came from one
int paths_ret(gphip_paths* q, int rc) {
    if (rc && q->sp) q->sp->err = q->h->err;
    return rc;
}

// strips of a contraction of ncon indices when the launch has wgs workgroups without them: whole slabs, wgs x strips >= 2 per CU
// while there are slabs; forced > 0: that many (at most one per slab)
int paths_strips(const gphip_ctx* h, long wgs, long ncon, int forced, int* strip_slabs) {
    const long nslabs = (ncon + PC_TJ - 1) / PC_TJ, target = 2l * std::max(h->ncu, 1);
    long n = forced > 0 ? std::min<long>(forced, nslabs) : (wgs >= target ? 1 : std::min<long>(nslabs, (target + wgs - 1) / wgs));
    n = std::max<long>(n, 1);
    *strip_slabs = (int)((nslabs + n - 1) / n);
    return (int)((nslabs + *strip_slabs - 1) / *strip_slabs);
}

// The contraction side of q for the points xt ([d][ldt], ntest of them): the features (kernel = false) or the training points
template <typename T>
PathsArgs<T> paths_side(const gphip_paths* q, bool kernel, const double* xt, long ldt, int64_t ntest) {
    PathsArgs<T> a{};
    a.xt = xt; a.ldt = ldt;
    a.con = kernel ? q->dXt.as<double>() : q->dOmT.as<double>();
    a.ldc = kernel ? (long)q->Npad : (long)q->Ftot;
    a.phase = kernel ? nullptr : q->dPhase.as<double>();
    a.W = kernel ? (const T*)q->dV.p : (const T*)q->dWa.p; a.ldw = (long)q->Spad;
    a.ntest = (int)ntest; a.ncon = (int)(kernel ? q->N : q->Ftot); a.S = q->S; a.d = (int)q->d;
    a.ie1 = kernel ? q->dIe1.as<double>() : nullptr;
    a.ie2 = (kernel && q->two) ? q->dIe2.as<double>() : nullptr;
    a.slotp = q->dSlotp.as<double>(); a.ks = q->ks;
    a.mpad = ldt;
    return a;
}

// One contraction: the points xt ([d][ldt], ntest of them) against the features (kernel = false) or the training points of q, into
// part (grown here).  grad: the GRAD form, d components.  *nstrips_out: the strips used.
template <typename T>
int queue_paths_contract(gphip_paths* q, bool kernel, bool grad, const double* xt, long ldt, int64_t ntest, Buf& part, int split, int* nstrips_out) {
    gphip_ctx* h = q->h;
    const int d = (int)q->d;
    PathsArgs<T> a = paths_side<T>(q, kernel, xt, ldt, ntest);
    a.ncomp = grad ? d : 1;
    const int SG = grad ? 64 : 128;
    const unsigned gz = (unsigned)((q->S + SG - 1) / SG) * (unsigned)(grad ? (d + PC_GW - 1) / PC_GW : 1);
    const unsigned gx = (unsigned)(ldt / PC_TP);
    const int nstrips = paths_strips(h, (long)gx * gz, a.ncon, split, &a.strip_slabs);
    *nstrips_out = nstrips;
    HIPCHK(part.grow((size_t)nstrips * a.ncomp * q->S * ldt * 8));
    a.part = part.as<double>();
    const dim3 grid(gx, (unsigned)nstrips, gz);
    // profile class 6 (prediction epilogue): flops = the MFMA accumulations; bytes = the weights once per point tile
    ProfScope ps(h, 6, 2.0 * a.ncomp * (double)ldt * a.ncon * q->S, (double)sizeof(T) * gx * a.ncon * q->S);
#define PATHS_GO(GEN, GRAD, DW) \
    hipLaunchKernelGGL((paths_contract_kernel<T, GEN, GRAD, DW>), grid, dim3(256), (paths_contract_lds<T, GRAD, DW>()), h->stream, a)
#define PATHS_DW(GEN, GRAD)                                  \
    do {                                                     \
        if (d <= 8) PATHS_GO(GEN, GRAD, 8);                  \
        else if (d <= 16) PATHS_GO(GEN, GRAD, 16);           \
        else if (d <= KB_LDS_MAXD) PATHS_GO(GEN, GRAD, 32);  \
        else PATHS_GO(GEN, GRAD, 0);                         \
    } while (0)
    if (kernel) { if (grad) PATHS_DW(GenKernel, true); else PATHS_DW(GenKernel, false); }
    else { if (grad) PATHS_DW(GenFeature, true); else PATHS_DW(GenFeature, false); }
#undef PATHS_DW
#undef PATHS_GO
    return GPHIP_OK;
}

// a mixture object's evaluation (gphip_paths_mix.inc): shared = all draws at the same M points, else every draw at its own
int paths_mix_eval(gphip_paths* q, const double* X, int64_t M, bool shared, double* out, double* dout);

// the null kernel's answer, f = m (a mixture object: m of the draw's row), gradients 0
void paths_null_eval(const gphip_paths* q, int64_t M, double* out, double* dout) {
    for (int s = 0; s < q->S; ++s)
        for (int64_t t = 0; t < M; ++t) out[(int64_t)s * M + t] = q->mix ? q->mu_r[(size_t)q->row_of[(size_t)s]] : q->mu;
    if (dout)
        for (int64_t e = 0; e < (int64_t)q->S * M * q->d; ++e) dout[e] = 0.0;
}

int paths_us(std::chrono::steady_clock::time_point t0) {
    return (int)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
}

// the device part of gphip_paths_create (h->mu held): *nan_out = a non-finite v
template <typename T>
int paths_create_device(gphip_paths* q, bool* nan_out) {
    gphip_ctx* h = q->h;
    const int64_t N = q->N, Npad = q->Npad, d = q->d, Ftot = q->Ftot, Spad = q->Spad;
    const int S = q->S;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(q->dXt.grow((size_t)d * Npad * 8));
    HIPCHK(q->dIe1.grow((size_t)d * 8));
    HIPCHK(q->dIe2.grow((size_t)d * 8));
    HIPCHK(q->dSlotp.grow((size_t)SLOTP * 8));
    HIPCHK(q->dOmT.grow((size_t)d * Ftot * 8));
    HIPCHK(q->dPhase.grow((size_t)Ftot * 8));
    HIPCHK(q->dWa.grow((size_t)Ftot * Spad * sizeof(T)));
    HIPCHK(q->dW.grow((size_t)S * Ftot * 8));
    HIPCHK(q->dEps.grow((size_t)S * N * 8));
    HIPCHK(q->dV.grow((size_t)Npad * Spad * sizeof(T)));
    HIPCHK(q->dFlag.grow(2 * sizeof(double) * (size_t)std::max<int64_t>(Ftot, Npad)));        // [0]: the flag word; then amp / r staging
    std::vector<double> xt((size_t)d * Npad, 0.0), omt((size_t)d * Ftot), r((size_t)Npad, 0.0);
    for (int64_t i = 0; i < N; ++i) {
        for (int64_t c = 0; c < d; ++c) xt[(size_t)c * Npad + i] = h->hostX[(size_t)i * d + c];
        r[(size_t)i] = h->hostY[(size_t)i] - q->mu;
    }
    for (int64_t j = 0; j < Ftot; ++j)
        for (int64_t c = 0; c < d; ++c) omt[(size_t)c * Ftot + j] = q->omega[(size_t)j * d + c];
    hipStream_t st = h->stream;
    HIPCHK(hipMemcpyAsync(q->dXt.p, xt.data(), xt.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(q->dOmT.p, omt.data(), omt.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(q->dPhase.p, q->phase.data(), (size_t)Ftot * 8, hipMemcpyHostToDevice, st));
    // the fit's own staged hyper-parameters (slot 0), as the prediction kernels read them
    HIPCHK(hipMemcpyAsync(q->dIe1.p, h->dInvEll.p, (size_t)d * 8, hipMemcpyDeviceToDevice, st));
    if (q->two) HIPCHK(hipMemcpyAsync(q->dIe2.p, h->dInvEll2.p, (size_t)d * 8, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(q->dSlotp.p, h->dSlotp.p, (size_t)SLOTP * 8, hipMemcpyDeviceToDevice, st));
    double* stage = q->dFlag.as<double>() + 1;                 // amp now, r after the weights kernel
    HIPCHK(hipMemsetAsync(q->dFlag.p, 0, 8, st));
    HIPCHK(hipMemcpyAsync(stage, q->amp.data(), (size_t)Ftot * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(q->dWa.p, 0, (size_t)Ftot * Spad * sizeof(T), st));
    const long nw = (long)S * Ftot;
    hipLaunchKernelGGL(paths_weights_kernel<T>, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, q->dW.as<double>(), (T*)q->dWa.p,
                       (const double*)stage, S, (long)Ftot, (long)Spad, q->seed);
    HIPCHK(hipStreamSynchronize(st));                          // (xt, omt: the copies have read the host vectors)
    const auto t_feat = std::chrono::steady_clock::now();
    int nsf = 0;
    if (int rc = queue_paths_contract<T>(q, false, false, q->dXt.as<double>(), (long)Npad, N, q->dPartF, h->paths_split, &nsf)) return rc;
    HIPCHK(hipMemcpyAsync(stage, r.data(), (size_t)Npad * 8, hipMemcpyHostToDevice, st));
    if (int rc = ensure_vbuf(h, Spad)) return rc;
    const long nv = (long)Npad * Spad;
    hipLaunchKernelGGL(paths_resid_kernel<T>, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, (const double*)q->dPartF.p, nsf, S, (long)N,
                       (long)Npad, (const double*)stage, q->sn, rff_key(q->seed, RFF_TAG_EPS), q->dEps.as<double>(), (T*)h->dV.p, (long)Spad);
    HIPCHK(hipStreamSynchronize(st));
    h->paths_feature_us = paths_us(t_feat);
    const auto t_sub = std::chrono::steady_clock::now();
    // v = K^-1 R: the rows of the vector block, as gphip_solve
    const bool df_fwd = queue_forward_fit(h, Spad);
    if (df_fwd && df_backward_ready<double>(h)) launch_dataflow_inverse<double, 64>(h, Spad, true);
    else DISPATCH(h, queue_backward_rows, h, Spad);
    HIPCHK(hipMemcpyAsync(q->dV.p, h->dV.p, (size_t)nv * sizeof(T), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(paths_finite_kernel<T>, dim3(1024), dim3(256), 0, st, (const T*)q->dV.p, nv, reinterpret_cast<int*>(q->dFlag.p));
    int flag = 0;
    const int rc = complete_call(h, [&]() -> int {
        HIPCHK(hipMemcpyAsync(&flag, q->dFlag.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return GPHIP_OK;
    });
    h->paths_subst_us = paths_us(t_sub);
    if (rc) return rc;
    *nan_out = flag != 0;
    q->dPartF.release();                                        // (N-sized: an evaluation sizes its own)
    return GPHIP_OK;
}

// points per chunk: option paths_chunk n > 0 = n points rounded up to whole tiles; else up to 16384, halved while the partials
// (8 strips assumed at most) and the outputs would pass 1 GiB
int64_t paths_chunk_rows(const gphip_paths* q, int64_t M, bool grad) {
    const gphip_ctx* h = q->h;
    if (h->paths_chunk > 0) return ((int64_t)h->paths_chunk + PC_TP - 1) / PC_TP * PC_TP;
    int64_t mc = std::min<int64_t>(16384, (M + PC_TP - 1) / PC_TP * PC_TP);
    const double per_point = 8.0 * q->S * (grad ? (double)q->d + 1.0 : 1.0) * 3.0;
    while (mc > PC_TP && per_point * (double)mc > 1073741824.0) mc = (mc / 2 + PC_TP - 1) / PC_TP * PC_TP;
    return mc;
}

template <typename T>
int paths_eval_device(gphip_paths* q, const double* X, int64_t M, double* out, double* dout) {
    gphip_ctx* h = q->h;
    const int64_t d = q->d;
    const int S = q->S;
    HIPCHK(hipSetDevice(h->device));
    const int64_t MC = paths_chunk_rows(q, M, dout != nullptr);
    HIPCHK(q->dXs.grow((size_t)d * MC * 8));
    HIPCHK(q->dOut.grow((size_t)S * MC * 8));
    if (dout) HIPCHK(q->dDout.grow((size_t)S * MC * d * 8));
    std::vector<double> xt, ho, hd;
    hipStream_t st = h->stream;
    for (int64_t m0 = 0; m0 < M; m0 += MC) {
        const int64_t mc = std::min<int64_t>(MC, M - m0), mpad = (mc + PC_TP - 1) / PC_TP * PC_TP;
        xt.assign((size_t)d * mpad, 0.0);
        for (int64_t i = 0; i < mc; ++i)
            for (int64_t c = 0; c < d; ++c) xt[(size_t)c * mpad + i] = X[(m0 + i) * d + c];
        HIPCHK(hipMemcpyAsync(q->dXs.p, xt.data(), xt.size() * 8, hipMemcpyHostToDevice, st));
        int nsf = 0, nsk = 0;
        if (int rc = queue_paths_contract<T>(q, false, false, q->dXs.as<double>(), (long)mpad, mc, q->dPartF, h->paths_split, &nsf)) return rc;
        if (int rc = queue_paths_contract<T>(q, true, false, q->dXs.as<double>(), (long)mpad, mc, q->dPartK, h->paths_split, &nsk)) return rc;
        h->paths_nsplit = nsk;
        const long no = (long)S * mc;
        hipLaunchKernelGGL(paths_finish_kernel, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, st, (const double*)q->dPartF.p, nsf,
                           (const double*)q->dPartK.p, nsk, S, (long)mpad, (long)mc, q->mu, q->dOut.as<double>());
        ho.resize((size_t)no);
        HIPCHK(hipMemcpyAsync(ho.data(), q->dOut.p, (size_t)no * 8, hipMemcpyDeviceToHost, st));
        if (dout) {                                // (the partial buffers are reused: stream order keeps the finish kernel in front)
            if (int rc = queue_paths_contract<T>(q, false, true, q->dXs.as<double>(), (long)mpad, mc, q->dPartF, h->paths_split, &nsf)) return rc;
            if (int rc = queue_paths_contract<T>(q, true, true, q->dXs.as<double>(), (long)mpad, mc, q->dPartK, h->paths_split, &nsk)) return rc;
            const long nd = no * d;
            hipLaunchKernelGGL(paths_finish_grad_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, st, (const double*)q->dPartF.p, nsf,
                               (const double*)q->dPartK.p, nsk, S, (long)mpad, (long)mc, (int)d, q->dDout.as<double>());
            hd.resize((size_t)nd);
            HIPCHK(hipMemcpyAsync(hd.data(), q->dDout.p, (size_t)nd * 8, hipMemcpyDeviceToHost, st));
        }
        if (int rc = complete_call(h)) return rc;
        for (int s = 0; s < S; ++s) {
            memcpy(out + (size_t)s * M + m0, ho.data() + (size_t)s * mc, (size_t)mc * 8);
            if (dout) memcpy(dout + ((size_t)s * M + m0) * d, hd.data() + (size_t)s * mc * d, (size_t)(mc * d) * 8);
        }
    }
    return GPHIP_OK;
}

// ---- gphip_paths_eval_own: every draw at its own points (gp_paths_own.h)

// One contraction of the E pairs xt ([d][ldt], pair e = s mc + t at column e) against the features (kernel = false) or the
// training points of q, into part (grown here): ncomp = 1 (values) or 1 + d (grad) components per pair and strip.  The strips
// follow from the pairs alone, not from grad: the value is summed in the same order in both forms.
template <typename T>
int queue_paths_own(gphip_paths* q, bool kernel, bool grad, const double* xt, long ldt, int64_t E, int64_t mc, Buf& part, int split,
                    int* nstrips_out) {
    gphip_ctx* h = q->h;
    const int d = (int)q->d;
    PathsOwnArgs<T> o{};
    o.a = paths_side<T>(q, kernel, xt, ldt, E);
    PathsArgs<T>& a = o.a;
    a.ncomp = grad ? d + 1 : 1;
    o.mc = (int)mc;
    o.span = (int)std::min<int64_t>(q->S, (PO_P - 1) / mc + 2);
    const unsigned gx = (unsigned)(ldt / PO_P);
    const bool glb = d > KB_LDS_MAXD;
    // the strip rule counts 256-thread workgroups: two of this kernel's count as one
    const int nstrips = paths_strips(h, ((long)gx + 1) / 2, a.ncon, split, &a.strip_slabs);
    *nstrips_out = nstrips;
    HIPCHK(part.grow((size_t)nstrips * a.ncomp * ldt * 8));
    a.part = part.as<double>();
    const dim3 grid(gx, (unsigned)nstrips, (unsigned)(grad && glb ? (d + PO_GW - 1) / PO_GW : 1));
    // profile class 6 (prediction epilogue): flops = the FMAs of the dot products; bytes = the weight slabs once per workgroup
    ProfScope ps(h, 6, 2.0 * a.ncomp * (double)E * a.ncon, (double)sizeof(T) * gx * a.ncon * o.span);
#define PATHS_OWN_GO(GEN, GRAD, DW) \
    hipLaunchKernelGGL((paths_own_kernel<T, GEN, GRAD, DW>), grid, dim3(PO_P), (paths_own_lds<T, DW>(o.span)), h->stream, o)
#define PATHS_OWN_DW(GEN, GRAD)                                  \
    do {                                                         \
        if (d <= 8) PATHS_OWN_GO(GEN, GRAD, 8);                  \
        else if (d <= 16) PATHS_OWN_GO(GEN, GRAD, 16);           \
        else if (!glb) PATHS_OWN_GO(GEN, GRAD, 32);              \
        else PATHS_OWN_GO(GEN, GRAD, 0);                         \
    } while (0)
    if (kernel) { if (grad) PATHS_OWN_DW(GenKernel, true); else PATHS_OWN_DW(GenKernel, false); }
    else { if (grad) PATHS_OWN_DW(GenFeature, true); else PATHS_OWN_DW(GenFeature, false); }
#undef PATHS_OWN_DW
#undef PATHS_OWN_GO
    return GPHIP_OK;
}

// points per draw and chunk: option paths_chunk n > 0 = n, else all M; halved while the staged points, the partials of both
// contractions (the forced strips; the strip rule adds strips only while the pairs are few) and the outputs of the chunk would
// pass 1 GiB.  Sized for the gradient form whether dout is asked for or not: the chunks, and with them the strips and the bytes
// of out, do not depend on dout.
int64_t paths_own_chunk_rows(const gphip_paths* q, int64_t M) {
    const gphip_ctx* h = q->h;
    int64_t mc = h->paths_chunk > 0 ? std::min<int64_t>(M, h->paths_chunk) : M;
    const double per_pair = 8.0 * ((double)q->d + ((double)q->d + 1.0) * (2.0 * std::max(h->paths_split, 1) + 1.0));
    while (mc > 1 && per_pair * (double)q->S * (double)mc > 1073741824.0) mc = (mc + 1) / 2;
    return mc;
}

template <typename T>
int paths_eval_own_device(gphip_paths* q, const double* X, int64_t M, double* out, double* dout) {
    gphip_ctx* h = q->h;
    const int64_t d = q->d;
    const int S = q->S;
    HIPCHK(hipSetDevice(h->device));
    const int64_t MC = paths_own_chunk_rows(q, M);
    const int64_t EPAD = ((int64_t)S * MC + PO_P - 1) / PO_P * PO_P;
    HIPCHK(q->dXs.grow((size_t)d * EPAD * 8));
    HIPCHK(q->dOut.grow((size_t)S * MC * 8));
    if (dout) HIPCHK(q->dDout.grow((size_t)S * MC * d * 8));
    std::vector<double> xt, ho, hd;
    hipStream_t st = h->stream;
    const bool grad = dout != nullptr;
    for (int64_t m0 = 0; m0 < M; m0 += MC) {
        const int64_t mc = std::min<int64_t>(MC, M - m0), E = (int64_t)S * mc, epad = (E + PO_P - 1) / PO_P * PO_P;
        xt.assign((size_t)d * epad, 0.0);
        for (int64_t s = 0; s < S; ++s)
            for (int64_t i = 0; i < mc; ++i)
                for (int64_t c = 0; c < d; ++c) xt[(size_t)c * epad + s * mc + i] = X[((int64_t)s * M + m0 + i) * d + c];
        HIPCHK(hipMemcpyAsync(q->dXs.p, xt.data(), xt.size() * 8, hipMemcpyHostToDevice, st));
        int nsf = 0, nsk = 0;
        if (int rc = queue_paths_own<T>(q, false, grad, q->dXs.as<double>(), (long)epad, E, mc, q->dPartF, h->paths_split, &nsf)) return rc;
        if (int rc = queue_paths_own<T>(q, true, grad, q->dXs.as<double>(), (long)epad, E, mc, q->dPartK, h->paths_split, &nsk)) return rc;
        h->paths_own_nsplit = nsk;
        const int ncomp = grad ? (int)d + 1 : 1;
        const long nf = (long)E * ncomp;
        hipLaunchKernelGGL(paths_own_finish_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, (const double*)q->dPartF.p, nsf,
                           (const double*)q->dPartK.p, nsk, ncomp, (long)epad, (long)E, q->mu, q->dOut.as<double>(),
                           grad ? q->dDout.as<double>() : nullptr);
        ho.resize((size_t)E);
        HIPCHK(hipMemcpyAsync(ho.data(), q->dOut.p, (size_t)E * 8, hipMemcpyDeviceToHost, st));
        if (grad) {
            hd.resize((size_t)(E * d));
            HIPCHK(hipMemcpyAsync(hd.data(), q->dDout.p, (size_t)(E * d) * 8, hipMemcpyDeviceToHost, st));
        }
        if (int rc = complete_call(h)) return rc;
        for (int s = 0; s < S; ++s) {
            memcpy(out + (size_t)s * M + m0, ho.data() + (size_t)s * mc, (size_t)mc * 8);
            if (grad) memcpy(dout + ((size_t)s * M + m0) * d, hd.data() + (size_t)s * mc * d, (size_t)(mc * d) * 8);
        }
    }
    return GPHIP_OK;
}

}  // namespace

extern "C" {

int gphip_paths_create(gphip_handle h, int S, int F, uint64_t seed, gphip_paths_handle* out, int* info) {
    if (out) *out = nullptr;
    if (!h || !out || !info) return fail(h, GPHIP_ERR_ARG, "null argument");
    *info = GPHIP_INFO_OK;
    if (S < 1 || F < 1 || S > PATHS_MAX_S) return fail(h, GPHIP_ERR_DIM, "S < 1, F < 1 or S > 2048");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (!has_fit(h)) return fail(h, GPHIP_ERR_STATE, "gphip_paths_create before a successful gphip_fit");
    if (h->custom) return fail(h, GPHIP_ERR_UNSUPPORTED, "no spectral law is known for a run-time compiled covariance function");
    if (h->fit_pw) return fail(h, GPHIP_ERR_UNSUPPORTED, "gphip_paths_create after gphip_fit_pw with a point-dependent nugget / mean");
    if (h->dist_fit) return fail(h, GPHIP_ERR_UNSUPPORTED, "gphip_paths_create from a sharded factor (replicate_factor = 0)");
    const auto t0 = std::chrono::steady_clock::now();
    gphip_paths* q = new gphip_paths;
    q->h = h; q->S = S; q->F = F; q->seed = seed;
    q->N = h->N; q->Npad = h->Npad; q->d = h->d; q->Spad = ((int64_t)S + TB - 1) / TB * TB;
    q->mu = h->mu_fit;
    if (h->null_fit) {                             // null kernel: f = m, answered on the host
        q->null_k = true;
        ++h->paths_live;
        *out = q;
        return GPHIP_OK;
    }
    const std::vector<double>& th = h->theta_fit;
    const int p = (int)th.size();
    int rc = gphip_rff_table(h->kernel_id, h->d, th.data(), p, F, seed, &q->Ftot, nullptr, nullptr, nullptr);
    if (!rc && q->Ftot * S > PATHS_MAX_FS) rc = GPHIP_ERR_DIM;
    if (!rc) {
        q->omega.resize((size_t)q->Ftot * q->d); q->phase.resize((size_t)q->Ftot); q->amp.resize((size_t)q->Ftot);
        rc = gphip_rff_table(h->kernel_id, h->d, th.data(), p, F, seed, &q->Ftot, q->omega.data(), q->phase.data(), q->amp.data());
    }
    if (rc) {
        delete q;
        return fail(h, rc, rc == GPHIP_ERR_DIM ? "Ftot x S above 2^26" : "no feature table for the fitted kernel (a negative constant offset?)");
    }
    q->ks = h->ks; q->two = h->ks.op != 0;
    q->sn = std::fabs(th[(size_t)p - 1 - (h->mean_id == GPHIP_MEAN_CONST ? 1 : 0)]);
    bool nan = false;
    rc = DISPATCH(h, paths_create_device, q, &nan);
    if (rc || nan) {
        (void)hipSetDevice(h->device);
        delete q;
        if (rc) return rc;
        *info = GPHIP_INFO_NAN;
        return GPHIP_OK;
    }
    ++h->paths_live;
    *out = q;
    h->paths_create_us = paths_us(t0);
    return GPHIP_OK;
}

int gphip_paths_eval(gphip_paths_handle q, const void* Xs, int64_t M, double* out, double* dout) {
    if (!q) return GPHIP_ERR_ARG;
    gphip_ctx* h = q->h;
    if (!Xs || !out) return paths_ret(q, fail(h, GPHIP_ERR_ARG, "null argument"));
    if (M < 1) return paths_ret(q, fail(h, GPHIP_ERR_DIM, "M < 1"));
    PathsLock lk(q);
    if (q->null_k) {
        paths_null_eval(q, M, out, dout);
        return GPHIP_OK;
    }
    if (q->mix) return paths_ret(q, paths_mix_eval(q, static_cast<const double*>(Xs), M, true, out, dout));
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = DISPATCH(h, paths_eval_device, q, static_cast<const double*>(Xs), M, out, dout);
    h->paths_eval_us = paths_us(t0);
    return paths_ret(q, rc);
}

int gphip_paths_eval_own(gphip_paths_handle q, const void* Xs, int64_t M, double* out, double* dout) {
    if (!q) return GPHIP_ERR_ARG;
    gphip_ctx* h = q->h;
    if (!Xs || !out) return paths_ret(q, fail(h, GPHIP_ERR_ARG, "null argument"));
    if (M < 1) return paths_ret(q, fail(h, GPHIP_ERR_DIM, "M < 1"));
    PathsLock lk(q);
    if (q->null_k) {
        paths_null_eval(q, M, out, dout);
        return GPHIP_OK;
    }
    if (q->mix) return paths_ret(q, paths_mix_eval(q, static_cast<const double*>(Xs), M, false, out, dout));
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = DISPATCH(h, paths_eval_own_device, q, static_cast<const double*>(Xs), M, out, dout);
    h->paths_own_us = paths_us(t0);
    return paths_ret(q, rc);
}

int gphip_paths_shape(gphip_paths_handle q, int* S, int64_t* Ftot, int64_t* N, int64_t* d) {
    if (!q) return GPHIP_ERR_ARG;
    if (S) *S = q->S;
    if (Ftot) *Ftot = q->Ftot;
    if (N) *N = q->N;
    if (d) *d = q->d;
    return GPHIP_OK;
}

int gphip_paths_get(gphip_paths_handle q, double* omega, double* phase, double* w, double* eps, double* v) {
    if (!q) return GPHIP_ERR_ARG;
    gphip_ctx* h = q->h;
    PathsLock lk(q);
    if (q->mix && (omega || phase)) return fail(h, GPHIP_ERR_ARG, "a mixture object's tables are per row: gphip_paths_get_table");
    if (q->null_k) return GPHIP_OK;                 // no features, no weights: nothing to copy (Ftot = 0)
    if (omega) memcpy(omega, q->omega.data(), q->omega.size() * 8);
    if (phase) memcpy(phase, q->phase.data(), q->phase.size() * 8);
    HIPCHK(hipSetDevice(h->device));
    if (w) HIPCHK(hipMemcpy(w, q->dW.p, (size_t)q->S * q->Ftot * 8, hipMemcpyDeviceToHost));
    if (eps) HIPCHK(hipMemcpy(eps, q->dEps.p, (size_t)q->S * q->N * 8, hipMemcpyDeviceToHost));
    if (v) {
        std::vector<double> tmp;
        if (int rc = DISPATCH(h, download, h, tmp, q->dV.p, (size_t)q->Npad * q->Spad, h->stream)) return paths_ret(q, rc);
        for (int s = 0; s < q->S; ++s)
            for (int64_t i = 0; i < q->N; ++i) v[(size_t)s * q->N + i] = tmp[(size_t)i * q->Spad + s];
    }
    return GPHIP_OK;
}

int gphip_paths_destroy(gphip_paths_handle q) {
    if (!q) return GPHIP_OK;
    gphip_ctx* h = q->h;
    {
        PathsLock lk(q);
        (void)hipSetDevice(h->device);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        --h->paths_live;
        delete q;                                   // (the buffers free themselves, on h->device)
    }
    return GPHIP_OK;
}

}  // extern "C"
