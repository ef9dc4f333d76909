// gphip_sparse.inc -- sparse inducing-point GP: the collapsed variational bound of Titsias (2009), its fit and prediction
// (include/gphip.h: gphip_sparse_*; kernels: gp_sparse.h).  Included at the end of gphip.hip.
//
// The forward pass of the bound exists once, in sparse_group: nb thetas in workspace slots 0 .. nb - 1 of u and b, every launch
// with the slot as its last grid index.  sparse_eval (gphip_sparse_bound / _fit / _bound_grad / _bound_grad_inducing) is the group
// of ONE slot in resident mode (SparseKeep::fit), sparse_eval_batch (gphip_sparse_bound_batch, the native sampler) loops groups in
// batch mode (SparseKeep::nothing), sparse_predict_samples (gphip_sparse_predict_samples) loops them in SparseKeep::group and
// substitutes with the factors each group leaves; DESIGN.md sections 8f and 8h list what the mode decides.  Per slot:
//   u (a context whose TRAINING points are Z, y = 0; its nugget slot scalar carries the jitter j)
//        queue_build + queue_factor        L_u L_u^T = k(Z, Z) + j I, direct-difference kernel build
//        per chunk of data points, treated as test points of u, sparse_chunk_head (the gradient's recomputed chunks share it):
//        queue_cross + queue_forward_slots the chunk of V = L_u^-1 k(Z, X) in u->dV, V(t, k) at V[t + k ld]
//        sparse_resid[_pw]_kernel          r = y - mu of the chunk (row 0 of the rhs operand), partial sums of r^2
//        sparse_accumulate_kernel          b's workspace: lower tiles += V^T V, rhs tile row += r^T V  (chunks in order)
//   b (a context of m points whose workspace is filled by hand)
//        sparse_diag_kernel                tr(V V^T), then B = sn^2 I + V V^T
//        queue_factor                      L_B, log det B, c = L_B^-1 V r in the rhs row, c^T c in the corner
// Gradient (gphip_sparse_bound_grad, DESIGN.md section 8d): after that evaluation
//   b    a = L_B^-T c, B^-1 by substitutions of identity rows, sparse_small_kernel: S = I / sn^2 - B^-1 and the inner matrix of H
//   u    H by two backward substitutions around a transposition, queue_grad_full with Kinv := -2 H (the K_uu term)
//        per chunk, as before: V (kept from the evaluation when the call has one chunk), w = (r - V^T a) / sn^2,
//        sparse_weight_kernel T = -2 (V S + w a^T) into b's dV, queue_backward_rows on it (G = L_u^-T T), the rectangular
//        gradient reduction (rows = the chunk's points, columns = Z) into the same accumulators, chunks in order
// Gradient in the inducing locations (gphip_sparse_bound_grad_inducing, DESIGN.md section 8e): the same pass; sparse_zgrad_kernel
//   contracts -2 H (rows = Z) and every chunk's -2 G (rows = the chunk's points) per COLUMN with the coordinate differences,
//   sparse_zgrad_finish_kernel adds the strip partials, H first and then chunk after chunk, into the m x d accumulator dZacc
// Everything of one evaluation up to B runs on u's stream; b's stream takes over after a host synchronisation.
// Prediction exists once, in sparse_predict_pass (DESIGN.md section 8h): per chunk of test points and for all slots at once,
//   v1 = L_u^-1 k(Z, x*) by u's forward substitution, sparse_handover_kernel takes V1 from u's dV to b's and the norms |v1|^2 on
//   the way, b's stream waits for an event of u's, v2 = L_B^-1 v1 by b's substitution, the exact path's partial launch against c
//   and one finishing kernel.  gphip_sparse_predict[_pw] is the pass for the ONE slot of the resident fit,
//   gphip_sparse_predict_samples[_pw] the pass after every group.
// Gradients in the test inputs (gphip_sparse_predict_grad, DESIGN.md section 8j): the pass for the one slot of the resident fit
//   with one more step per chunk (sparse_queue_pgrad): b substitutes V2 backward and forms V1 - sn^2 (that), an event hands it to u,
//   u substitutes backward with L_u and runs the exact path's reduction kernel (queue_xgrad) against the scaled Z.
// Joint prediction (gphip_sparse_predict_cov / _draws / _logpdf, DESIGN.md section 8g): all M rows of V1 = L_u^-1 k(Z, X*) and
//   V2 = L_B^-1 V1 side by side in u's dV, the rhs-row operand -c / sn^2 in u's dJZ; u owns the child context of the exact
//   path (u->joint, gphip_joint.inc: training points X*, K(X*, X*) by the direct build) and the two-segment downdate_kernel turns
//   the child's workspace into Sigma = K(X*, X*) - V1^T V1 + sn^2 V2^T V2 and its rhs row into y* - mu.  Cov, draws and the log
//   density then are the exact path's own code on that child.
#include "gp_sparse.h"

// The phases timed by HIP events while option "profile" is on, and the options that read them (gphip_sparse_get_option).
// PH_KUU_FACTOR .. PH_GRAD_INDUCING are reset by every evaluation of the bound, PH_JOINT_V .. PH_JOINT_FACTOR by every joint
// prediction, PH_SAMPLES_VU .. by every prediction pass: gphip_sparse_predict, gphip_sparse_predict_grad (the only one that fills
// PH_PGRAD_*) and gphip_sparse_predict_samples (which also evaluates the bound).
enum SparsePhaseId {
    PH_KUU_FACTOR, PH_CROSS, PH_FORWARD, PH_ACCUMULATE, PH_B_FACTOR,                               // the bound
    PH_GRAD_SMALL, PH_GRAD_WEIGHTS, PH_GRAD_BACKWARD, PH_GRAD_REDUCE, PH_GRAD_INDUCING,            // its gradients
    PH_JOINT_V, PH_JOINT_BUILD, PH_JOINT_DOWNDATE, PH_JOINT_FACTOR,                                // joint prediction
    PH_SAMPLES_VU, PH_SAMPLES_HANDOVER, PH_SAMPLES_VB, PH_SAMPLES_REDUCE,                          // prediction over samples
    PH_PGRAD_BACKWARD, PH_PGRAD_REDUCE,                                                            // gradients in the test inputs
    PH_COUNT
};
static const char* const SPARSE_PHASE_OPTION[] = {
    "ms_kuu_factor", "ms_cross", "ms_forward", "ms_accumulate", "ms_b_factor",
    "ms_grad_small", "ms_grad_weights", "ms_grad_backward", "ms_grad_reduce", "ms_grad_inducing",
    "ms_joint_v", "ms_joint_build", "ms_joint_downdate", "ms_joint_factor",
    "ms_samples_v1", "ms_samples_handover", "ms_samples_v2", "ms_samples_reduce",
    "ms_pgrad_backward", "ms_pgrad_reduce"};
static_assert(sizeof SPARSE_PHASE_OPTION / sizeof SPARSE_PHASE_OPTION[0] == PH_COUNT, "one option name per phase");

struct gphip_sparse_ctx {
    std::recursive_mutex mu;
    gphip_ctx *u = nullptr, *b = nullptr;
    int device = 0, dtype = 64;
    size_t es = 8;
    int64_t N = 0, d = 0, Npad = 0, m = 0;
    int kernel_id = 0, mean_id = 0;
    bool custom = false;
    std::string body;
    int ncp = 0;
    std::vector<std::pair<std::string, double>> forwarded;    // options handed on to u and b (replayed after gphip_sparse_set_inducing)
    Buf dXt, dY;                               // typed [d][Npad], [Npad]: the data, resident
    Buf dRz; int64_t rcap = 0; int rz_slots = 0;   // typed [slot][16][rcap]: row 0 = r of the current chunk, the other rows zero
    Buf dPar, hPar;                            // double [slot][SPARSE_PAR]: mu, B's sn^2, k(x, x) and the noise of every slot's theta (device; pinned staging copy)
    Buf dWz;                                   // typed [slot][rcap]: the weight row 1 / nu of the current chunk (point-dependent noise), zero on the pad
    Buf dPwTrain, dPwTest;                     // double: a group's rows of mean_train | nugget_train ([2][slot][N]); a chunk's of mean_test | nugget_test ([2][slot][mpad])
    Buf dAccP;                                 // typed [slot][strip][tile][128 x 128]: strip partials of the accumulation
    Buf dSum; std::vector<double> hSum;        // double, per slot: [0] tr(V V^T), then the per-block partial sums of r^2 and of k(x_i, x_i)
    Buf dBc, dS, dH;                           // gradient, typed: B's tiles before its factorisation; S; the inner matrix of H (mpad x mpad)
    Buf dLd, dRes;                             // refined backward substitutions with L_u: its diagonal tiles [Nt][128 x 128], one block column of residuals
    Buf dZpart, dZacc;                         // gradient in Z, double: [part][term][mpad][d] strip partials; the [mpad][d] accumulator
    Buf dGw;                                   // gradient, double: [0] tr B^-1, [1] a^T a, per-block sums of w, w of a chunk, strip partials of V^T a
    // options
    int chunk = 0, split = 0, profile = 0;
    int joint_split = 0;                       // joint prediction: strips of the stacked contraction (0 = by the split rule)
    int batch_slots = 0;                       // gphip_sparse_bound_batch / _predict_samples: most thetas per group (0 = by the group rule)
    int samples_chunk = 0;                     // the prediction pass: most test points per chunk (0 = by the caller's rule)
    int samples_handover = 1;                  // the prediction pass: 1 = sparse_handover_kernel, 0 = copy + norm launch (measurement)
    int pgrad_refine = 1;                      // gphip_sparse_predict_grad: 1 = the backward substitution with L_u refines its diagonal solves
    int pw_fused = 0;                          // the _pw calls: 1 = the weight inside the contraction, 0 = sparse_scale_rows_kernel + the unweighted one
                                               // (the default since the measurement of DESIGN.md section 8i: fused lost at the largest size)
    // read-only results of the last call
    int last_nsplit = 0;
    int joint_nsplit = 0;                      // strips the last joint prediction's downdate used
    int last_slots = 0;                        // thetas in the last group of the last gphip_sparse_bound_batch
    int last_chunk = 0;                        // data points per chunk of the last evaluation
    int last_samples_chunk = 0;           // test points per chunk of the last prediction pass
    double last_jitter = 0.0;
    int grad_analytic = 0;                     // the last gphip_sparse_bound_grad: 1 = the analytic route, 0 = central differences
    double ms[PH_COUNT] = {};                  // K_uu factor, cross build, forward substitution, accumulation, B factor;
                                               // gradient: small m x m work, weights, backward substitution, reductions, the reduction in Z;
                                               // joint prediction: V1 and V2, K(X*, X*), the downdate, the factorisation of Sigma;
                                               // prediction over samples: V1, the handover to b, V2, the reductions;
                                               // gradients in the test inputs: the backward substitutions, the reduction
    // the resident fit
    bool fitted = false;
    bool pw_fit = false;                       // the fit was made with a point-dependent array: B = I + V W V^T, no joint prediction
    double sn2_fit = 0, mu_fit = 0, kxx_fit = 0, jit_fit = 0;
    std::string err;
};

namespace {

constexpr int64_t SPARSE_MAX_M = GPHIP_SPARSE_MAX_M;

int sfail(gphip_sparse_ctx* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}

void sparse_reset_phases(gphip_sparse_ctx* h, SparsePhaseId first, SparsePhaseId end) {
    for (int k = first; k < end; ++k) h->ms[k] = 0.0;
}

struct SparsePhase { SparsePhaseId phase; hipEvent_t e0, e1; };

// The event pairs of one call.  They come from u's pool and go back to it when the call ends, on every exit path: declare the
// owner BEFORE the call's scopes, so that every scope has closed when it is destroyed.
struct SparsePhases {
    gphip_sparse_ctx* h;
    std::vector<SparsePhase> recs;
    explicit SparsePhases(gphip_sparse_ctx* h_) : h(h_) {}
    SparsePhases(const SparsePhases&) = delete;
    SparsePhases& operator=(const SparsePhases&) = delete;
    ~SparsePhases() { harvest(); }
    void harvest() {                           // adds the times to h->ms (waits for each closing event)
        for (const SparsePhase& r : recs) {
            float ms = 0.f;
            (void)hipEventSynchronize(r.e1);   // (a scope's closing event may have been recorded after the call's last synchronisation)
            if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) h->ms[r.phase] += ms;
            else (void)hipGetLastError();
            h->u->pool.push_back(r.e0);
            h->u->pool.push_back(r.e1);
        }
        recs.clear();
    }
};

// HIP-event pair around a phase of the evaluation while option "profile" is on
struct SparseScope {
    SparsePhases& ph; SparsePhase r; hipStream_t st; bool on;
    SparseScope(SparsePhases& ph_, SparsePhaseId phase, hipStream_t st_) : ph(ph_), st(st_), on(ph_.h->profile > 0) {
        if (!on) return;
        r.phase = phase; r.e0 = get_event(ph.h->u); r.e1 = get_event(ph.h->u);
        (void)hipEventRecord(r.e0, st);
    }
    ~SparseScope() {
        if (!on) return;
        (void)hipEventRecord(r.e1, st);
        ph.recs.push_back(r);
    }
};

template <typename T>
int sparse_func_attrs(gphip_sparse_ctx* h) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(sparse_accumulate_kernel<T, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)SwizzledK<T>::LDS));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(sparse_accumulate_kernel<T, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)SwizzledK<T>::LDS));
#define ZG_ATTR(DW)                                                                                                              \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(sparse_zgrad_kernel<T, DW, false, false>),                          \
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)sparse_zgrad_lds<T, DW, false>(1)));             \
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(sparse_zgrad_kernel<T, DW, false, true>),                           \
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)sparse_zgrad_lds<T, DW, false>(2)));
    ZG_ATTR(2) ZG_ATTR(4) ZG_ATTR(8) ZG_ATTR(16)
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(sparse_zgrad_kernel<T, 32, false, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)sparse_zgrad_lds<T, 32, false>(1)));
#undef ZG_ATTR
    return GPHIP_OK;
}

// the two contexts for the inducing points Z [m][d]
int sparse_make_children(gphip_sparse_ctx* h, const double* Z, int64_t m) {
    std::vector<double> y0((size_t)m, 0.0);
    gphip_handle u = nullptr, b = nullptr;
    std::string why;
    int rc = create_ctx(Z, y0.data(), m, h->d, h->custom ? (int)GPHIP_KERNEL_CUSTOM : h->kernel_id, h->mean_id, h->dtype, h->device, &u,
                        h->custom ? h->body.c_str() : nullptr, h->ncp, &why);
    if (rc) return sfail(h, rc, "creating the inducing-point context failed " + why);
    rc = create_ctx(Z, y0.data(), m, h->d, GPHIP_KERNEL_SE, GPHIP_MEAN_ZERO, h->dtype, u->device, &b);
    if (rc) { gphip_destroy(u); return sfail(h, rc, "creating the context of B failed"); }
    if (h->u) gphip_destroy(h->u);
    if (h->b) gphip_destroy(h->b);
    h->u = u; h->b = b; h->m = m; h->device = u->device;
    h->fitted = false;
    for (const auto& o : h->forwarded) {
        (void)gphip_set_option(u, o.first.c_str(), o.second);
        (void)gphip_set_option(b, o.first.c_str(), o.second);
    }
    u->kbuild_mfma = 0;                        // K_uu and k(Z, X) from the same, direct-difference form of the kernel build
    return GPHIP_OK;
}

// data points [c0, c0 + mpad) of a resident [d][ld] block -> u's test-point block [d][mpad]
int sparse_load_points(gphip_sparse_ctx* h, const void* xt, int64_t ld, int64_t c0, int64_t mpad) {
    gphip_ctx* u = h->u;
    HIPCHK(hipMemcpy2DAsync(u->dXsT.p, (size_t)mpad * h->es, static_cast<const char*>(xt) + (size_t)c0 * h->es, (size_t)ld * h->es,
                            (size_t)mpad * h->es, (size_t)h->d, hipMemcpyDeviceToDevice, u->stream));
    u->test_ratio = HUGE_VAL;                  // (no verdict of the MFMA kernel build applies: u builds with the direct form)
    return GPHIP_OK;
}

// [slot][16][rcap] residual rows for nb slots of `rows` data points each (zeroed whenever they are laid out again)
int sparse_ensure_rz(gphip_sparse_ctx* h, int nb, int64_t rows) {
    if (rows <= h->rcap && nb <= h->rz_slots) return GPHIP_OK;
    const int64_t rcap = std::max(rows, h->rcap);
    const int ns = std::max(nb, h->rz_slots);
    h->rcap = 0; h->rz_slots = 0;
    const size_t bytes = (size_t)ns * 16 * rcap * h->es;
    HIPCHK(h->dRz.grow(bytes));
    HIPCHK(hipMemsetAsync(h->dRz.p, 0, bytes, h->u->stream));
    h->rcap = rcap; h->rz_slots = ns;
    return GPHIP_OK;
}

// mu, sn^2 and k(x, x) of the first nb slots, staged in hPar -> device, on u's stream
int sparse_copy_par(gphip_sparse_ctx* h, int nb) {
    HIPCHK(hipMemcpyAsync(h->dPar.p, h->hPar.p, (size_t)nb * SPARSE_PAR * 8, hipMemcpyHostToDevice, h->u->stream));
    return GPHIP_OK;
}
int sparse_ensure_par(gphip_sparse_ctx* h, int nb) {
    HIPCHK(h->dPar.grow((size_t)nb * SPARSE_PAR * 8));
    HIPCHK(h->hPar.grow((size_t)nb * SPARSE_PAR * 8, true));
    return GPHIP_OK;
}

// C += V^T V, rhs row += r^T V for the chunk of mpad rows in u->dV, for every one of nb slots by ONE launch (slot s: V at
// dV + s mpad Npad, C = b's workspace slot s), in the strips of strip_split (gp_contract.h) for output tiles x slots workgroups.
// weighted: C += V^T W V, rhs row += r^T W V with the slots' weight rows in dWz (the kernel's other instantiation).
template <typename T>
int sparse_queue_accumulate(gphip_sparse_ctx* h, int64_t mpad, int nb, bool weighted) {
    gphip_ctx *u = h->u, *b = h->b;
    SparseAccArgs<T> g{};
    g.C = (T*)b->dA.p; g.R = (int)b->R;
    g.V = (const T*)u->dV.p; g.ldv = (long)mpad;
    g.Z = (const T*)h->dRz.p; g.ldr = (long)h->rcap;
    g.W = weighted ? (const T*)h->dWz.p : nullptr; g.ldw = (long)h->rcap;
    g.Mt = (int)u->Nt; g.ntri = g.Mt * (g.Mt + 1) / 2; g.ntiles = g.ntri + g.Mt;
    g.K = (int)mpad;
    g.c_bstride = (long)b->slot_elems; g.v_bstride = (long)mpad * u->Npad; g.z_bstride = 16l * h->rcap;
    int strip_tiles;
    const int nsplit = strip_split((long)g.ntiles * nb, (int)(mpad / TB), h->split, u->ncu, &strip_tiles);
    g.kstrip = strip_tiles * TB;
    h->last_nsplit = nsplit;
    if (nsplit > 1) {
        g.p_bstride = (long)nsplit * g.ntiles * TS;
        HIPCHK(h->dAccP.grow((size_t)nb * g.p_bstride * sizeof(T)));
        g.P = (T*)h->dAccP.p;
    }
    void (*const kernel)(SparseAccArgs<T>) = weighted ? sparse_accumulate_kernel<T, true> : sparse_accumulate_kernel<T, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)g.ntiles, (unsigned)nsplit, (unsigned)nb), dim3(256), SwizzledK<T>::LDS, u->stream, g);
    if (nsplit > 1)
        hipLaunchKernelGGL(strip_reduce_kernel<T>, dim3((unsigned)g.ntiles, 16, (unsigned)nb), dim3(256), 0, u->stream, g.C, g.R, g.ntri, g.Mt,
                           g.ntiles, (const T*)g.P, nsplit, 1.0, g.c_bstride, g.p_bstride);
    return GPHIP_OK;
}

// r = y - mu_s of the chunk for nb slots (mu_s from dPar); slot s's partial sums go to part + s pstride
template <typename T>
int sparse_queue_resid(gphip_sparse_ctx* h, int64_t c0, int64_t mc, int64_t mpad, double* part, int nb, long pstride) {
    hipLaunchKernelGGL(sparse_resid_kernel<T>, dim3((unsigned)((mpad + 255) / 256), (unsigned)nb), dim3(256), 0, h->u->stream,
                       (const T*)h->dY.p + c0, (int)mc, (int)mpad, (const double*)h->dPar.as<double>(), SPARSE_PAR, (T*)h->dRz.p, 16l * h->rcap, part,
                       pstride);
    return GPHIP_OK;
}

// The point-dependent mean and noise of a call (gphip_sparse_*_pw), a property of the group evaluation.  mean / nugget: the
// group's rows, row s = slot s, N values each; a null array is the constant of theta, broadcast.
struct SparsePw {
    const double *mean = nullptr, *nugget = nullptr;
    bool any() const { return mean || nugget; }
    SparsePw rows_from(int64_t s0, int64_t N) const { return SparsePw{mean ? mean + s0 * N : nullptr, nugget ? nugget + s0 * N : nullptr}; }
};

// r = y - m_i and the weight row 1 / nu_i of the chunk for nb slots from the group's arrays in dPwTrain (pw's null array: the
// slot's constant in dPar); slot s's partial sums of r^2 w, log nu and w go to part + s pstride + {0, 2 pn, 3 pn}
template <typename T>
int sparse_queue_resid_pw(gphip_sparse_ctx* h, const SparsePw& pw, int64_t c0, int64_t mc, int64_t mpad, double* part, int nb, long pstride,
                          long pn) {
    const double* dm = h->dPwTrain.as<double>() + c0;
    hipLaunchKernelGGL(sparse_resid_pw_kernel<T>, dim3((unsigned)((mpad + 255) / 256), (unsigned)nb), dim3(256), 0, h->u->stream,
                       (const T*)h->dY.p + c0, (int)mc, (int)mpad, (const double*)h->dPar.as<double>(), pw.mean ? dm : nullptr,
                       pw.nugget ? dm + (size_t)nb * h->N : nullptr, (long)h->N, (T*)h->dRz.p, 16l * h->rcap, (T*)h->dWz.p, (long)h->rcap, part,
                       pstride, pn);
    return GPHIP_OK;
}

// option "sparse_pw_fused" = 0: the chunk of V and the residual row of nb slots times sqrt(w) in place
template <typename T>
int sparse_queue_scale_rows(gphip_sparse_ctx* h, int64_t mpad, int nb) {
    gphip_ctx* u = h->u;
    hipLaunchKernelGGL(sparse_scale_rows_kernel<T>, dim3((unsigned)(mpad / 256 + 1), (unsigned)u->Npad + 1, (unsigned)nb), dim3(256), 0, u->stream,
                       (T*)u->dV.p, (long)mpad, (long)mpad * u->Npad, (int)u->Npad, (T*)h->dRz.p, 16l * h->rcap, (const T*)h->dWz.p, (long)h->rcap,
                       (int)mpad);
    return GPHIP_OK;
}

// per-block partial sums of k(x_i, x_i) of the chunk (u->dKss) for nb slots; weighted: of k(x_i, x_i) / nu_i
template <typename T>
int sparse_queue_kk(gphip_sparse_ctx* h, int64_t mc, int64_t mpad, double* part, int nb, long pstride, bool weighted) {
    hipLaunchKernelGGL(sparse_blocksum_kernel<T>, dim3((unsigned)((mpad + 255) / 256), (unsigned)nb), dim3(256), 0, h->u->stream,
                       h->u->dKss.as<double>(), (long)mpad, (int)mc, part, pstride, weighted ? (const T*)h->dWz.p : nullptr, (long)h->rcap);
    return GPHIP_OK;
}

// the trace and B = sn_s^2 I + V V^T of nb slots (sn_s^2 from dPar); slot s's trace goes to out[s ostride]
template <typename T>
int sparse_queue_diag(gphip_sparse_ctx* h, double* out, int nb = 1, long ostride = 0) {
    gphip_ctx* b = h->b;
    hipLaunchKernelGGL(sparse_diag_kernel<T>, dim3((unsigned)nb), dim3(256), 0, h->u->stream, (T*)b->dA.p, (long)b->slot_elems, (int)b->R,
                       (int)b->N, (int)b->Npad, (const double*)h->dPar.as<double>() + 1, SPARSE_PAR, out, ostride);
    return GPHIP_OK;
}

// queue_factor on nb slots of a context whose workspaces are ready (build: after queue_build), to the end of the call; want_w:
// it leaves the block inverses that forward substitutions with the factor use.  Slot s's info, as gphip_loglik's, is c->hInfo[s].
int sparse_factor(gphip_sparse_ctx* h, gphip_ctx* c, int nb, bool build, bool want_w, const char* what) {
    {
        FactorMode mode(c, want_w);
        c->theta_packed = false; c->fused_eval = false;
        if (build) DISPATCH(c, queue_build, c, nb);
        DISPATCH(c, queue_factor, c, nb);
    }
    c->abort_unread = what;
    const int rc = complete_call(c);
    return rc ? sfail(h, rc, c->err) : GPHIP_OK;
}

// prediction: the mpad rows of V1 of nb slots from u's dV into b's, the strip partials of |v1|^2 into u->dPart [slot][strip][mpad]
// on the way (sparse_handover_kernel, in the strips of the exact path's predict_strips), on u's stream
template <typename T>
int sparse_queue_handover(gphip_sparse_ctx* h, int64_t mpad, int nb, int* nstrips_out) {
    gphip_ctx *u = h->u, *b = h->b;
    int nstrips = 0;
    const int js = predict_strips(u, mpad, nb, &nstrips);
    HIPCHK(u->dPart.grow((size_t)nb * nstrips * mpad * 8));
    hipLaunchKernelGGL(sparse_handover_kernel<T>, dim3((unsigned)(mpad / TB), (unsigned)nstrips, (unsigned)nb), dim3(256), 0, u->stream,
                       (const T*)u->dV.p, (T*)b->dV.p, (long)mpad, (long)mpad * u->Npad, (int)u->N, (int)u->Npad, js, u->dPart.as<double>(),
                       nstrips);
    *nstrips_out = nstrips;
    return GPHIP_OK;
}

// The head of the data chunk [c0, c0 + mc) for nb slots, on u's stream: the chunk's points into u's test-point block, its mpad rows
// of V = L_u^-1 k(Z, X) into u->dV (queue_forward_slots: resident = slot 0 with the fitted factor, all_factored = its guard) and
// the residual rows into dRz -- with pw the weight rows into dWz as well.  Slot s's partial sums go to part + s pstride (pw: pn
// apart per sum).  The chunk loop of the group evaluator and the gradient's recomputed chunks both come through here, so a
// recomputed chunk's V, residual and weights are the evaluation's.
int sparse_chunk_head(gphip_sparse_ctx* h, int64_t c0, int64_t mc, int64_t mpad, int nb, bool resident, bool all_factored, const SparsePw& pw,
                      double* part, long pstride, long pn, SparsePhases& ph) {
    gphip_ctx* u = h->u;
    {
        SparseScope ps(ph, PH_CROSS, u->stream);
        if (const int rc = sparse_load_points(h, h->dXt.p, h->Npad, c0, mpad)) return rc;
        DISPATCH(u, queue_cross, u, mc, mpad, nb);
    }
    {
        SparseScope ps(ph, PH_FORWARD, u->stream);
        queue_forward_slots(u, mpad, nb, resident, all_factored);
    }
    if (pw.any()) return DISPATCH(h, sparse_queue_resid_pw, h, pw, c0, mc, mpad, part, nb, pstride, pn);
    return DISPATCH(h, sparse_queue_resid, h, c0, mc, mpad, part, nb, pstride);
}

// mean of k(z, z) over the inducing points of a run-time compiled kernel (the default jitter's scale) for the thetas of the
// first nb slots, which are on the device; out [nb]
int sparse_mean_kzz(gphip_sparse_ctx* h, int64_t rows, double* out, int nb = 1) {
    gphip_ctx* u = h->u;
    std::vector<double> k, s((size_t)nb, 0.0);
    for (int64_t c0 = 0; c0 < u->N; c0 += rows) {
        const int64_t mc = std::min(rows, u->N - c0), mpad = (mc + TB - 1) / TB * TB;
        int rc = sparse_load_points(h, u->dXt.p, u->Npad, c0, mpad);
        if (!rc) rc = queue_custom_kss(u, mc, mpad, nb);
        if (rc) return rc == GPHIP_ERR_HIP && !u->err.empty() ? sfail(h, rc, u->err) : rc;
        k.resize((size_t)nb * mpad);
        HIPCHK(hipMemcpyAsync(k.data(), u->dKss.p, k.size() * 8, hipMemcpyDeviceToHost, u->stream));
        HIPCHK(hipStreamSynchronize(u->stream));
        for (int q = 0; q < nb; ++q)
            for (int64_t t = 0; t < mc; ++t) s[(size_t)q] += k[(size_t)q * mpad + t];
    }
    for (int q = 0; q < nb; ++q) out[q] = s[(size_t)q] / (double)u->N;
    return GPHIP_OK;
}

// dZacc += scale x the column-wise contraction of the weight block W (nrows x u's columns, W(t, j) at W[j ldw + t]) whose rows are
// the points xr / xr2 (scaled by term 1 / term 2, [d][ldr]).  Strips: whole slabs of 32 rows, strips x column tiles ~ 2 per CU.
template <typename T>
int sparse_queue_zgrad(gphip_sparse_ctx* h, const void* W, long ldw, const void* xr, const void* xr2, int64_t ldr, int64_t nrows, double scale) {
    gphip_ctx* u = h->u;
    SparseZGradArgs<T> a{};
    a.W = (const T*)W; a.ldw = ldw;
    a.xr = (const T*)xr; a.xr2 = (const T*)xr2; a.ldr = (int)ldr;
    a.zs = (const T*)u->dXs.p; a.zs2 = (const T*)u->dXs2.p; a.ldz = (int)u->Npad;
    a.nrows = (int)nrows; a.ncols = (int)u->N; a.d = (int)u->d; a.d0 = 0;
    a.slotp = u->dSlotp.as<double>(); a.ks = u->ks;
    a.mpad = (int)u->Npad;
    const int Mt = (int)u->Nt, nterm = u->ks.op != 0 ? 2 : 1;
    const int64_t nslabs = (nrows + ZG_TR - 1) / ZG_TR;
    int64_t nstrips = std::min<int64_t>(nslabs, (2l * std::max(u->ncu, 1) + Mt - 1) / Mt);
    const int64_t strip_slabs = (nslabs + nstrips - 1) / nstrips;
    nstrips = (nslabs + strip_slabs - 1) / strip_slabs;
    a.strip_rows = (int)(strip_slabs * ZG_TR);
    const long md = (long)u->Npad * u->d;
    HIPCHK(h->dZpart.grow((size_t)(2 * nstrips * nterm) * md * 8));
    a.part = h->dZpart.as<double>();
    const dim3 grid((unsigned)Mt, (unsigned)nstrips);
    const int d = a.d;
#define ZG_LAUNCH(DW)                                                                                                            \
    do {                                                                                                                         \
        if (nterm == 2) hipLaunchKernelGGL((sparse_zgrad_kernel<T, DW, false, true>), grid, dim3(256), (sparse_zgrad_lds<T, DW, false>(2)), u->stream, a); \
        else hipLaunchKernelGGL((sparse_zgrad_kernel<T, DW, false, false>), grid, dim3(256), (sparse_zgrad_lds<T, DW, false>(1)), u->stream, a);           \
    } while (0)
    if (d <= 2) { ZG_LAUNCH(2); }
    else if (d <= 4) { ZG_LAUNCH(4); }
    else if (d <= 8) { ZG_LAUNCH(8); }
    else if (d <= 16) { ZG_LAUNCH(16); }
    else if (d <= KB_LDS_MAXD && nterm == 1)
        hipLaunchKernelGGL((sparse_zgrad_kernel<T, 32, false, false>), grid, dim3(256), (sparse_zgrad_lds<T, 32, false>(1)), u->stream, a);
    else                                       // (two terms beyond 16 dimensions: 2 x 32 accumulators would not stay in registers)
                                               // the points from global memory, one launch per window of 16 coordinates
        for (a.d0 = 0; a.d0 < d; a.d0 += 16) {
            if (nterm == 2) hipLaunchKernelGGL((sparse_zgrad_kernel<T, 16, true, true>), grid, dim3(256), (sparse_zgrad_lds<T, 16, true>(2)), u->stream, a);
            else hipLaunchKernelGGL((sparse_zgrad_kernel<T, 16, true, false>), grid, dim3(256), (sparse_zgrad_lds<T, 16, true>(1)), u->stream, a);
        }
#undef ZG_LAUNCH
    hipLaunchKernelGGL(sparse_zgrad_finish_kernel, dim3((unsigned)((md + 255) / 256)), dim3(256), 0, u->stream, (const double*)a.part,
                       (int)(2 * nstrips), nterm, md, d, (const double*)u->dInvEll.as<double>(),
                       (const double*)(nterm == 2 ? u->dInvEll2.as<double>() : nullptr), scale, h->dZacc.as<double>());
    return GPHIP_OK;
}

// what the evaluation hands on to the gradient phase
struct SparseGradIn {
    const double* theta;
    SparsePw pw;                               // the evaluation's arrays, for the head of a recomputed chunk (no entry point has a gradient with them yet)
    double sn2, mu, rtr, ctc, trvv, skk;
    int64_t rows, nchunks;
};

// The gradient of the bound after a successful evaluation (u and b factored, both streams idle; the call's single chunk of V
// still in u->dV when nchunks == 1).  grad: p derivatives in theta's layout (null: the reductions in theta are skipped);
// gradZ: row-major m x d derivatives in the inducing locations (null: not wanted).
template <typename T>
int sparse_grad_phase(gphip_sparse_ctx* h, const SparseGradIn& in, SparsePhases& ph, double* grad, double* gradZ) {
    gphip_ctx *u = h->u, *b = h->b;
    const int64_t mpm = b->Npad;                // padded inducing points
    const int Mt = (int)b->Nt;
    const double sn2 = in.sn2;
    int rc;
    const size_t nblk = (size_t)(h->Npad / 256 + in.nchunks + 1);
    HIPCHK(h->dS.grow((size_t)mpm * mpm * sizeof(T)));
    HIPCHK(h->dH.grow((size_t)mpm * mpm * sizeof(T)));
    HIPCHK(h->dGw.grow((2 + nblk + (size_t)in.rows * (1 + Mt)) * 8));
    double* d_tr = h->dGw.as<double>();
    double* d_ws = d_tr + 2;
    double* d_w = d_ws + nblk;
    double* d_vta = d_w + in.rows;
    // every backward substitution with L_u refines its diagonal solves (queue_backward_rows): G and H cancel in dF/dZ by up
    // to 6e7, and a bare product with the explicit 128-block inverses costs it four digits at cond(K_uu) = 2e11
    const int64_t rpad = std::max<int64_t>(mpm, (std::min<int64_t>(in.rows, h->N) + TB - 1) / TB * TB);
    HIPCHK(h->dLd.grow((size_t)u->Nt * TS * sizeof(T)));
    HIPCHK(h->dRes.grow((size_t)rpad * TB * sizeof(T)));
    const size_t nz = (size_t)mpm * h->d;
    if (gradZ) {
        HIPCHK(h->dZacc.grow(nz * 8));
        HIPCHK(hipMemsetAsync(h->dZacc.p, 0, nz * 8, u->stream));
    }
    // ---- b: a, B^-1, S and the inner matrix of H
    {
        SparseScope ps(ph, PH_GRAD_SMALL, b->stream);
        HIPCHK(b->dAlpha.grow((size_t)mpm * sizeof(T)));
        if ((rc = queue_alpha<T>(b))) return sfail(h, rc, b->err);
        int gx = (int)((mpm * mpm + 255) / 256);
        if (gx > 4096) gx = 4096;
        hipLaunchKernelGGL(identity_rows_kernel<T>, dim3(gx), dim3(256), 0, b->stream, (T*)b->dV.p, (long)mpm, (int)mpm, 0, (int)b->N);
        queue_forward_rows<T>(b, mpm, 1, 0, true);
        queue_backward_rows<T>(b, mpm);
        hipLaunchKernelGGL(sparse_small_kernel<T>, dim3(gx), dim3(256), 0, b->stream, (const T*)b->dV.p, (long)mpm, (const T*)b->dAlpha.p,
                           (const T*)h->dBc.p, (int)b->R, (int)b->N, (int)mpm, sn2, (T*)h->dS.p, (T*)h->dH.p);
        hipLaunchKernelGGL(sparse_trace_kernel<T>, dim3(1), dim3(256), 0, b->stream, (const T*)b->dV.p, (long)mpm, (const T*)b->dAlpha.p,
                           (int)b->N, d_tr);
    }
    if ((rc = complete_call(b))) return sfail(h, rc, b->err);
    // ---- u: H = L_u^-T [..] L_u^-1 by two backward substitutions (the inner matrix is symmetric), then the K_uu term
    HIPCHK(u->dAlpha.grow((size_t)u->Npad * sizeof(T)));
    HIPCHK(hipMemsetAsync(u->dAlpha.p, 0, (size_t)u->Npad * sizeof(T), u->stream));
    if ((rc = ensure_gacc(u))) return sfail(h, rc, u->err);
    HIPCHK(hipMemsetAsync(u->dGacc.p, 0, u->ngacc * 8, u->stream));
    {
        SparseScope ps(ph, PH_GRAD_SMALL, u->stream);
        if ((rc = queue_backward_rows<T>(u, mpm, h->dH.p, h->dLd.p, h->dRes.p))) return sfail(h, rc, u->err);
        hipLaunchKernelGGL(sparse_transpose_kernel<T>, dim3((unsigned)(mpm / 32), (unsigned)(mpm / 32)), dim3(256), 0, u->stream,
                           (const T*)h->dH.p, (long)mpm, (T*)b->dV.p, (long)mpm);
        if ((rc = queue_backward_rows<T>(u, mpm, b->dV.p, h->dLd.p, h->dRes.p))) return sfail(h, rc, u->err);
    }
    if (grad) {
        SparseScope ps(ph, PH_GRAD_REDUCE, u->stream);
        queue_grad_full<T>(u, b->dV.p, (long)mpm, nullptr);
    }
    if (gradZ) {                               // sum_l 2 H_lk dk(z_l, z_k)/dz_k: the rows are Z itself, nothing is halved
        SparseScope ps(ph, PH_GRAD_INDUCING, u->stream);
        if ((rc = sparse_queue_zgrad<T>(h, b->dV.p, (long)mpm, u->dXs.p, u->dXs2.p, mpm, u->N, 1.0))) return rc;
    }
    // ---- the chunks of data points, in the evaluation's order
    size_t used = 0;
    for (int64_t c0 = 0; c0 < h->N; c0 += in.rows) {
        const int64_t mc = std::min(in.rows, h->N - c0), mpad = (mc + TB - 1) / TB * TB;
        const unsigned nb = (unsigned)((mpad + 255) / 256);
        // (the evaluation's chunk again: mu is still in dPar, and its partial sums, which are not read again, go where chunk 0's went)
        if (in.nchunks > 1 && (rc = sparse_chunk_head(h, c0, mc, mpad, 1, true, true, in.pw, h->dSum.as<double>() + 1, 0l, (long)nblk, ph)))
            return rc;
        {
            SparseScope ps(ph, PH_GRAD_SMALL, u->stream);
            hipLaunchKernelGGL(sparse_vta_kernel<T>, dim3(nb, (unsigned)Mt), dim3(256), 0, u->stream, (const T*)u->dV.p, (long)mpad,
                               (const T*)b->dAlpha.p, (int)mpad, d_vta);
            hipLaunchKernelGGL(sparse_w_kernel<T>, dim3(nb), dim3(256), 0, u->stream, (const T*)h->dRz.p, (const double*)d_vta, Mt, (int)mc,
                               (int)mpad, sn2, d_w, d_ws + used);
        }
        {
            SparseScope ps(ph, PH_GRAD_WEIGHTS, u->stream);
            SparseWeightArgs<T> g{};
            g.V = (const T*)u->dV.p; g.ldv = (long)mpad;
            g.S = (const T*)h->dS.p; g.lds = (long)mpm;
            g.w = d_w; g.a = (const T*)b->dAlpha.p;
            g.out = (T*)b->dV.p; g.ldo = (long)mpad;
            g.mpad = (int)mpm; g.scale = -2.0;
            hipLaunchKernelGGL(sparse_weight_kernel<T>, dim3((unsigned)(mpad / TB), (unsigned)Mt), dim3(256), 0, u->stream, g);
        }
        {
            SparseScope ps(ph, PH_GRAD_BACKWARD, u->stream);
            if ((rc = queue_backward_rows<T>(u, mpad, b->dV.p, h->dLd.p, h->dRes.p))) return sfail(h, rc, u->err);
        }
        if (grad) {
            SparseScope ps(ph, PH_GRAD_REDUCE, u->stream);
            GradArgs<T> a = grad_args<T>(u, b->dV.p, (long)mpad, 0, mc);
            a.xr = (const T*)u->dXsS.p; a.xr2 = (const T*)u->dXsS2.p; a.npad_r = (int)mpad;
            launch_grad<T>(u, a, dim3((unsigned)(mpad / TB), (unsigned)u->Nt));
            if (h->custom) {                   // - sum_i dk(x_i, x_i) / (2 sn^2): the dual-number program on the chunk's own points
                GradArgs<T> dg = a;
                dg.diag = 1; dg.wdiag = -1.0 / sn2;
                launch_grad<T>(u, dg, dim3((unsigned)(mpad / TB), 1u));
            }
        }
        if (gradZ) {                           // sum_i G_ki dk(z_k, x_i)/dz_k from -2 G: halved
            SparseScope ps(ph, PH_GRAD_INDUCING, u->stream);
            if ((rc = sparse_queue_zgrad<T>(h, b->dV.p, (long)mpad, u->dXsS.p, u->dXsS2.p, mpad, mc, 0.5))) return rc;
        }
        used += nb;
    }
    std::vector<double> gacc(u->ngacc), hw(2 + used), zacc(gradZ ? nz : 0);
    HIPCHK(hipMemcpyAsync(gacc.data(), u->dGacc.p, gacc.size() * 8, hipMemcpyDeviceToHost, u->stream));
    HIPCHK(hipMemcpyAsync(hw.data(), h->dGw.p, hw.size() * 8, hipMemcpyDeviceToHost, u->stream));
    if (gradZ) HIPCHK(hipMemcpyAsync(zacc.data(), h->dZacc.p, nz * 8, hipMemcpyDeviceToHost, u->stream));
    if ((rc = complete_call(u))) return sfail(h, rc, u->err);
    if (gradZ) std::copy(zacc.begin(), zacc.begin() + (size_t)h->m * h->d, gradZ);
    if (!grad) return GPHIP_OK;
    // ---- host: the diagonal term of a stationary family in closed form (weight -1 / sn^2 per point on the reductions' accumulators,
    // every family is 1 at r = 0 and dg/dalpha is 0 there), the noise derivative, the chain rule, the mean
    const int64_t d = h->d;
    const double N = (double)h->N, m = (double)h->m;
    if (!h->custom) {
        const double* sp = u->hSlotp.as<double>();
        const int op = u->ks.op;
        const double wd = -N / sn2, k1 = sp[0], k2 = op != 0 ? sp[SP_SF2B] : 0.0;
        gacc[(size_t)d] += wd * (op == 2 ? k2 : 1.0) * k1;
        if (op != 0) gacc[(size_t)2 * d + 2] += wd * (op == 2 ? k1 : 1.0) * k2;
        gacc[(size_t)2 * d + 5] += wd;
    }
    const double trbinv = hw[0], ata = hw[1];
    const double dsn = -0.5 * (N - m + sn2 * trbinv) / sn2 + 0.5 * (in.rtr - in.ctc - sn2 * ata) / (sn2 * sn2) +
                       (in.skk - in.trvv) / (2.0 * sn2 * sn2);
    gacc[h->custom ? (size_t)u->ncp : (size_t)d + 1] = 2.0 * dsn;          // (the reductions' own diagonal slot was the jitter's derivative)
    const int o = grad_chain_rule(u, in.theta, gacc, grad);
    if (h->mean_id == GPHIP_MEAN_CONST) {
        double sw = 0.0;
        for (size_t k = 0; k < used; ++k) sw += hw[2 + k];
        grad[o] = sw;
    }
    return GPHIP_OK;
}

// theta's length and the jitter of an entry point (called under the object's lock: gphip_sparse_set_inducing replaces u)
int sparse_check_args(gphip_sparse_ctx* h, int p, double jitter) {
    if (p != h->u->p) return sfail(h, GPHIP_ERR_DIM, "theta has the wrong length for this kernel/mean");
    if (std::isnan(jitter) || std::isinf(jitter)) return sfail(h, GPHIP_ERR_ARG, "non-finite jitter");
    return GPHIP_OK;
}

// What a group evaluation is for (DESIGN.md sections 8f and 8h).  fit: a one-theta entry point -- the factors of u and b stay
// resident for the substitutions that follow (prediction, the gradient phase), u substitutes with queue_forward_fit, and a theta
// that cannot be evaluated ends the call before the chunk loop.  nothing: a batch -- every row keeps its slot whatever becomes of
// it, and no factor outlives the call.  group: a batch whose caller substitutes with the factors of every slot of u and b before
// the next group overwrites them (gphip_sparse_predict_samples) -- it differs from nothing in one thing: B factors with its
// block inverses.  The mode is the caller's, never the number of rows: a group of one row of a batch is a batch.
enum class SparseKeep { fit, nothing, group };

// one theta's slot of a group evaluation
struct SparseSlot {
    bool ok = false;                           // theta and its jitter are usable (else stand-in values were staged)
    bool evaluated = false;                    // B was factored and F formed (SparseKeep::fit stops before that on a failure)
    int info = 0, uinfo = 0;                   // the row's info as gphip_loglik's; that of K_uu's factorisation alone
    bool pw = false;                           // whitened by a point-dependent array: B = I + V W V^T and the sums below carry w = 1 / nu
    double sn2 = 0, mu = 0, kxx = 0, jit = 0;
    double sb2 = 0;                            // the sn^2 of B = sn^2 I + V V^T: theta's, or 1 when whitened
    double F = 0, logdet = 0, ctc = 0, rtr = 0, trvv = 0, skk = 0, slognu = 0;
    void put_parts(double* out) const { out[0] = logdet; out[1] = ctc; out[2] = rtr; out[3] = trvv; out[4] = skk; }
    // the six parts of the _pw calls, B = I + V W V^T: what a whitened slot holds; a constant slot's five converted
    void put_parts_pw(double* out, int64_t N, int64_t m) const {
        if (pw) { put_parts(out); out[5] = slognu; return; }
        out[0] = logdet - (double)m * std::log(sn2); out[1] = ctc / sn2; out[2] = rtr / sn2; out[3] = trvv / sn2; out[4] = skk / sn2;
        out[5] = (double)N * std::log(sn2);
    }
};

// a row of a point-dependent array is usable: every mean value finite, every noise variance finite and > 0
bool sparse_pw_row_ok(const SparsePw& pw, int s, int64_t N) {
    if (pw.mean)
        for (int64_t i = 0; i < N; ++i)
            if (!std::isfinite(pw.mean[(size_t)s * N + i])) return false;
    if (pw.nugget)
        for (int64_t i = 0; i < N; ++i) {
            const double v = pw.nugget[(size_t)s * N + i];
            if (!std::isfinite(v) || !(v > 0.0)) return false;
        }
    return true;
}

// The bound for the nb rows of Theta in slots 0 .. nb - 1 of u and b, `rows` data points per chunk (the callers size u's dV, dRz
// and dPar for nb slots of them).  u builds and factors nb K_uu at once; every chunk of data points is loaded once and crossed,
// substituted, reduced and accumulated for all nb slots by launches whose last grid index is the slot; b factors nb matrices B at
// once.  A row that fails keeps its slot (a non-finite theta is staged as stage_theta's stand-in values with a unit nugget, so
// its slot factors) and only its own res[s] tells -- unless keep says that it ends the call.  keepB (null: not wanted): slot
// 0's B before its factorisation overwrites it.
// pw (DESIGN.md section 8i): the group's rows of a point-dependent mean and noise.  The data are whitened by w = 1 / nu_i: the
// residual kernel's pw form leaves the weight row, the accumulation runs its weighted instantiation, and the slot's B is
// I + V W V^T -- sn^2 = 1 for sparse_diag_kernel, b's nugget and b's pivot tolerance.  A row whose arrays are unusable is staged
// with the stand-in arrays m = 0, nu = 1 and fails like a non-finite theta.
int sparse_group(gphip_sparse_ctx* h, const double* Theta, int nb, int p, double jitter, int64_t rows, SparseKeep keep, Buf* keepB,
                 const SparsePw& pw, SparsePhases& ph, SparseSlot* res) {
    gphip_ctx *u = h->u, *b = h->b;
    const bool resident = keep == SparseKeep::fit;
    int rc;
    double* par = h->hPar.as<double>();
    for (int s = 0; s < nb; ++s) {
        SparseSlot& r = res[s];
        r = SparseSlot{};
        r.ok = stage_theta(u, s, Theta + (size_t)s * p);
        const double* sp = u->hSlotp.as<double>() + (size_t)s * SLOTP;
        r.sn2 = sp[1]; r.mu = sp[2]; r.kxx = sp[SP_KXX]; r.jit = jitter;
        r.pw = pw.any();
        r.sb2 = r.pw ? 1.0 : r.sn2;
        double* ps = par + (size_t)SPARSE_PAR * s;
        ps[0] = r.mu; ps[1] = r.sb2; ps[2] = r.kxx; ps[SPARSE_PAR_NOISE] = r.sn2;
    }
    std::vector<char> pw_ok((size_t)nb, 1);
    if (pw.any())
        for (int s = 0; s < nb; ++s)
            if (!sparse_pw_row_ok(pw, s, h->N)) { pw_ok[(size_t)s] = 0; res[s].ok = false; }
    if (jitter < 0.0) {                        // default: joint_jitter_rel x the row's k(x, x) (run-time compiled kernels: its mean of k(z, z))
        std::vector<double> scale((size_t)nb);
        for (int s = 0; s < nb; ++s) scale[(size_t)s] = res[s].kxx;
        if (h->custom) {
            if ((rc = copy_theta(u, nb))) return sfail(h, rc, u->err);
            if ((rc = sparse_mean_kzz(h, rows, scale.data(), nb))) return rc;
        }
        for (int s = 0; s < nb; ++s) res[s].jit = joint_jitter_rel(u) * scale[(size_t)s];
    }
    for (int s = 0; s < nb; ++s) {
        SparseSlot& r = res[s];
        if (!std::isfinite(r.jit) || r.jit < 0.0) r.ok = false;
        if (!r.ok && resident) { r.info = GPHIP_INFO_NAN; return GPHIP_OK; }
        if (r.ok) h->last_jitter = r.jit;
        else r.jit = 1.0;                      // (the stand-in theta of a row that is given up: K_uu + I factors)
        // u: the nugget slot carries the jitter; the pivot tolerance follows it
        double* sp = u->hSlotp.as<double>() + (size_t)s * SLOTP;
        sp[1] = r.jit;
        sp[SP_MFMA] = 0.0;
        if (h->custom) sp[SP_SF2B] = r.jit;
        else sp[3] = pivot_tol_rel(u) * (std::fabs(r.kxx) + r.jit);
    }
    if ((rc = copy_theta(u, nb))) return sfail(h, rc, u->err);
    HIPCHK(hipMemsetAsync(u->dInfo.p, 0, (size_t)nb * 4, u->stream));
    if ((rc = sparse_copy_par(h, nb))) return rc;
    std::vector<double> standin;               // (outlives the uploads: the call ends with a synchronisation of u's stream)
    if (pw.any()) {                            // the group's rows, once: every chunk reads its slice
        HIPCHK(h->dPwTrain.grow((size_t)2 * nb * h->N * 8));
        HIPCHK(h->dWz.grow((size_t)h->rz_slots * h->rcap * h->es));
        const double* src[2] = {pw.mean, pw.nugget};
        for (int a = 0; a < 2; ++a) {
            if (!src[a]) continue;
            double* dst = h->dPwTrain.as<double>() + (size_t)a * nb * h->N;
            bool all = true;
            for (int s = 0; s < nb; ++s) all = all && pw_ok[(size_t)s];
            if (all) { HIPCHK(hipMemcpyAsync(dst, src[a], (size_t)nb * h->N * 8, hipMemcpyHostToDevice, u->stream)); continue; }
            standin.assign((size_t)2 * h->N, 0.0);
            std::fill(standin.begin() + h->N, standin.end(), 1.0);
            for (int s = 0; s < nb; ++s)
                HIPCHK(hipMemcpyAsync(dst + (size_t)s * h->N, pw_ok[(size_t)s] ? src[a] + (size_t)s * h->N : standin.data() + (size_t)a * h->N,
                                      (size_t)h->N * 8, hipMemcpyHostToDevice, u->stream));
        }
    }
    {
        SparseScope ps(ph, PH_KUU_FACTOR, u->stream);
        rc = sparse_factor(h, u, nb, true, true, "sparse GP: the factorisation of K_uu timed out (set option dataflow=0 and report)");
    }
    if (rc) return rc;
    bool all_factored = true;
    for (int s = 0; s < nb; ++s)
        if ((res[s].uinfo = u->hInfo.as<int>()[s]) != 0) all_factored = false;
    if (resident) {
        if (!all_factored) { res[0].info = res[0].uinfo; return GPHIP_OK; }
        record_fit(u, true, Theta, p, u->hRes.as<double>()[0]);       // (queue_forward_fit asks for it)
    }
    // b: empty bordered workspaces; the nugget scalar of slot s is sn_s^2, its pivot tolerance relative to sn_s^2 (B >= sn_s^2 I)
    for (int s = 0; s < nb; ++s) {
        const double sn2 = res[s].sb2, thb[3] = {1.0, 1.0, std::sqrt(sn2)};
        (void)stage_theta(b, s, thb);
        double* spb = b->hSlotp.as<double>() + (size_t)s * SLOTP;
        spb[1] = sn2; spb[3] = pivot_tol_rel(b) * sn2; spb[4] = 0.0; spb[SP_MFMA] = 0.0;
    }
    if ((rc = copy_theta(b, nb))) return sfail(h, rc, b->err);
    HIPCHK(hipMemsetAsync(b->dInfo.p, 0, (size_t)nb * 4, b->stream));
    HIPCHK(hipMemsetAsync(b->dA.p, 0, (size_t)nb * b->slot_elems * h->es, u->stream));
    // partial sums per slot: [0] the trace, then one per 256 data points of every chunk for r^2, then the same for k(x_i, x_i)
    const int64_t nchunks = (h->N + rows - 1) / rows;
    // (whitened: two more, for log nu_i and for w_i = 1 / nu_i, and the other two carry w)
    const size_t nblk = (size_t)(h->Npad / 256 + nchunks + 1), ss = 1 + (pw.any() ? 4 : 2) * nblk;
    HIPCHK(h->dSum.grow((size_t)nb * ss * 8));
    double* d_r2 = h->dSum.as<double>() + 1;
    double* d_kk = d_r2 + nblk;
    size_t used = 0;
    for (int64_t c0 = 0; c0 < h->N; c0 += rows) {
        const int64_t mc = std::min(rows, h->N - c0), mpad = (mc + TB - 1) / TB * TB;
        if ((rc = sparse_chunk_head(h, c0, mc, mpad, nb, resident, all_factored, pw, d_r2 + used, (long)ss, (long)nblk, ph))) return rc;
        if (h->custom) {                       // k(x_i, x_i) per point and slot (u->dXsT still holds the chunk)
            if ((rc = queue_custom_kss(u, mc, mpad, nb))) return sfail(h, rc, u->err);
            DISPATCH(h, sparse_queue_kk, h, mc, mpad, d_kk + used, nb, (long)ss, pw.any());
        }
        used += (size_t)((mpad + 255) / 256);
        {
            SparseScope ps(ph, PH_ACCUMULATE, u->stream);
            const bool fused = pw.any() && h->pw_fused;
            if (pw.any() && !fused) DISPATCH(h, sparse_queue_scale_rows, h, mpad, nb);
            if ((rc = DISPATCH(h, sparse_queue_accumulate, h, mpad, nb, fused))) return rc;
        }
    }
    // a slot without a factor of K_uu accumulated whatever its V held: B = sn^2 I in its place, so that b factors numbers
    for (int s = 0; s < nb; ++s)
        if (res[s].uinfo != 0)
            HIPCHK(hipMemsetAsync(static_cast<char*>(b->dA.p) + (size_t)s * b->slot_elems * h->es, 0, (size_t)b->slot_elems * h->es, u->stream));
    DISPATCH(h, sparse_queue_diag, h, h->dSum.as<double>(), nb, (long)ss);
    if (keepB) {
        HIPCHK(keepB->grow((size_t)b->slot_elems * h->es));
        HIPCHK(hipMemcpyAsync(keepB->p, b->dA.p, (size_t)b->slot_elems * h->es, hipMemcpyDeviceToDevice, u->stream));
    }
    h->hSum.assign((size_t)nb * ss, 0.0);
    HIPCHK(hipMemcpyAsync(h->hSum.data(), h->dSum.p, (size_t)nb * ss * 8, hipMemcpyDeviceToHost, u->stream));
    if ((rc = complete_call(u))) return sfail(h, rc, u->err);          // (the forward substitutions' abort word)
    {
        SparseScope ps(ph, PH_B_FACTOR, b->stream);    // (fit, group: substitutions with L_B follow, so it leaves its block inverses)
        rc = sparse_factor(h, b, nb, false, keep != SparseKeep::nothing, "sparse GP: the factorisation of B timed out (set option dataflow=0 and report)");
    }
    if (rc) return rc;
    for (int s = 0; s < nb; ++s) {
        SparseSlot& r = res[s];
        const double* hs = h->hSum.data() + (size_t)s * ss;
        r.logdet = b->hRes.as<double>()[2 * s]; r.ctc = b->hRes.as<double>()[2 * s + 1];
        for (size_t k = 0; k < used; ++k) r.rtr += hs[1 + k];
        double sw = 0.0;                       // whitened: sum_i log nu_i and sum_i w_i
        if (r.pw) for (size_t k = 0; k < used; ++k) { r.slognu += hs[1 + 2 * nblk + k]; sw += hs[1 + 3 * nblk + k]; }
        if (h->custom) for (size_t k = 0; k < used; ++k) r.skk += hs[1 + nblk + k];
        else r.skk = r.pw ? sw * r.kxx : (double)h->N * r.kxx;
        r.trvv = hs[0];
        // (whitened: log det Lambda in the place of (N - m) log sn^2 -- B = I + V W V^T carries no power of sn^2 -- and sb2 = 1)
        r.F = -0.5 * ((double)h->N * LOG_TWO_PI + (r.pw ? r.slognu : (double)(h->N - h->m) * std::log(r.sn2)) + r.logdet + (r.rtr - r.ctc) / r.sb2) -
              (r.skk - r.trvv) / (2.0 * r.sb2);
        r.info = r.uinfo != 0 ? r.uinfo : b->hInfo.as<int>()[s];        // (a failure of u comes first)
        if (!r.ok || (r.info == 0 && !std::isfinite(r.F))) r.info = GPHIP_INFO_NAN;
        r.evaluated = true;
    }
    if (resident) {
        const double thb[3] = {1.0, 1.0, std::sqrt(res[0].sb2)};
        record_fit(b, res[0].info == 0, thb, 3, res[0].logdet);
    }
    return GPHIP_OK;
}

// One evaluation: the group evaluator with one slot, the fit left resident.  out, parts: the bound (null = not wanted); grad
// (null = not wanted): the analytic gradient in theta; gradZ (null = not wanted): the analytic gradient in the inducing
// locations, row-major m x d.
// pw (the _pw calls; no gradient): point-dependent arrays of N values.  six: parts are the six of gphip_sparse_bound_pw.
int sparse_eval(gphip_sparse_ctx* h, const double* theta, int p, double jitter, double* out, double* parts, int* info,
                double* grad = nullptr, double* gradZ = nullptr, const SparsePw& pw = SparsePw{}, bool six = false) {
    gphip_ctx *u = h->u, *b = h->b;
    int rc = sparse_check_args(h, p, jitter);
    if (rc) return rc;
    const double qnan = std::nan("");
    auto give_up = [&](int inf) {
        *info = inf;
        if (out) *out = qnan;
        if (parts) for (int k = 0; k < (six ? 6 : 5); ++k) parts[k] = qnan;
        return GPHIP_OK;
    };
    if (grad) for (int k = 0; k < p; ++k) grad[k] = qnan;
    if (gradZ) for (int64_t k = 0; k < h->m * h->d; ++k) gradZ[k] = qnan;
    const bool wants_grad = grad || gradZ;
    h->fitted = false;
    sparse_reset_phases(h, PH_KUU_FACTOR, PH_JOINT_V);
    for (int k = 0; k < p; ++k)
        if (!std::isfinite(theta[k])) return give_up(GPHIP_INFO_NAN);
    HIPCHK(hipSetDevice(h->device));
    if ((rc = ensure_slots(u, 1))) return sfail(h, rc, u->err);
    if ((rc = ensure_slots(b, 1))) return sfail(h, rc, b->err);
    invalidate_fit(u);
    invalidate_fit(b);
    if (!stage_theta(u, 0, theta)) return give_up(GPHIP_INFO_NAN);     // (an unusable theta: before any buffer is sized; the group stages it again)
    // rows of V per pass: ensure_vchunk's rule (V within ~8 GiB, at least 2048 rows, halved while it does not fit) and the option
    int64_t rows = 0;
    const int64_t cap = h->chunk > 0 ? std::min<int64_t>(((int64_t)h->chunk + TB - 1) / TB * TB, h->Npad) : h->Npad;
    if ((rc = ensure_vchunk(u, cap, &rows))) { (void)hipGetLastError(); return sfail(h, rc, "no device memory for a chunk of V: " + u->err); }
    if (wants_grad) {
        // the second m x rows buffer (the weights T; also the scratch of the m x m work) is b's dV: the rows are halved while both do not fit
        rc = ensure_vbuf(b, std::max(rows, b->Npad));
        while (rc == GPHIP_ERR_HIP && rows > 2048) {
            (void)hipGetLastError();
            rows = (rows / 2 + TB - 1) / TB * TB;
            u->vcap = 0;                       // (u's V shrinks with it: ensure_vbuf frees and allocates again)
            if (!(rc = ensure_vbuf(u, rows))) rc = ensure_vbuf(b, std::max(rows, b->Npad));
        }
        if (rc) { (void)hipGetLastError(); return sfail(h, rc, "no device memory for the gradient's weights: " + b->err); }
    }
    h->last_chunk = (int)rows;
    if ((rc = sparse_ensure_rz(h, 1, rows))) return rc;
    if ((rc = sparse_ensure_par(h, 1))) return rc;
    SparsePhases ph(h);
    SparseSlot r;
    // (the gradient wants B itself, before its factorisation overwrites it: the B / (2 sn^2) term of H)
    if ((rc = sparse_group(h, theta, 1, p, jitter, rows, SparseKeep::fit, wants_grad ? &h->dBc : nullptr, pw, ph, &r))) return rc;
    if (!r.evaluated) return give_up(r.info);
    if (parts && six) r.put_parts_pw(parts, h->N, h->m);
    else if (parts) r.put_parts(parts);
    if (out) *out = r.F;
    *info = r.info;
    h->fitted = *info == 0;
    h->pw_fit = pw.any();
    h->sn2_fit = r.sn2; h->mu_fit = r.mu; h->kxx_fit = r.kxx; h->jit_fit = r.jit;
    if (wants_grad && *info == 0) {
        const SparseGradIn in{theta, pw, r.sn2, r.mu, r.rtr, r.ctc, r.trvv, r.skk, rows, (h->N + rows - 1) / rows};
        rc = DISPATCH(h, sparse_grad_phase, h, in, ph, grad, gradZ);
        if (rc && grad) for (int k = 0; k < p; ++k) grad[k] = qnan;
        if (rc && gradZ) for (int64_t k = 0; k < h->m * h->d; ++k) gradZ[k] = qnan;
    }
    return rc;
}

// m(x*) and nu(x*) of test points [m0, m0 + mc) for nb slots (pwt: rows of M values; a null array stays null) into dPwTest as
// [2][slot][mpad], on b's stream, for sparse_predict_finish_kernel.  The noise is not read for a latent prediction.
int sparse_stage_test_arrays(gphip_sparse_ctx* h, const SparsePw& pwt, int64_t M, int64_t m0, int64_t mc, int64_t mpad, int nb, int latent,
                             const double** d_mean, const double** d_nug) {
    *d_mean = *d_nug = nullptr;
    const double* src[2] = {pwt.mean, latent ? nullptr : pwt.nugget};
    if (!src[0] && !src[1]) return GPHIP_OK;
    HIPCHK(h->dPwTest.grow((size_t)2 * nb * mpad * 8));
    for (int a = 0; a < 2; ++a) {
        if (!src[a]) continue;
        double* dst = h->dPwTest.as<double>() + (size_t)a * nb * mpad;
        HIPCHK(hipMemcpy2DAsync(dst, (size_t)mpad * 8, src[a] + m0, (size_t)M * 8, (size_t)mc * 8, (size_t)nb, hipMemcpyHostToDevice, h->b->stream));
        (a == 0 ? *d_mean : *d_nug) = dst;
    }
    return GPHIP_OK;
}

// The group and chunk rule of the batched calls (gphip_sparse_bound_batch, gphip_sparse_predict_samples) for B rows: *G rows per
// group, *rows data points of V per slot and pass; u and b get their slots, u's dV, dRz and dPar their sizes.  Drops any fit.
int sparse_size_groups(gphip_sparse_ctx* h, int B, int* G_out, int64_t* rows_out) {
    gphip_ctx *u = h->u, *b = h->b;
    // ---- the group: as many rows as u and b give slots, as keep 2048 data points of V per slot within the ~8 GiB of a chunk
    const int64_t mpm = u->Npad;
    const double budget = 8.0 * (1 << 30);
    int want = (int)std::min<int64_t>(B, std::max<int64_t>(1, (int64_t)(budget / ((double)mpm * 2048 * h->es))));
    if (h->batch_slots > 0) want = std::min(want, h->batch_slots);
    int rc = ensure_slots(u, want);
    if (rc) return sfail(h, rc, u->err);
    if ((rc = ensure_slots(b, want))) return sfail(h, rc, b->err);
    invalidate_fit(u);
    invalidate_fit(b);
    int G = std::min(want, std::min(u->slots, b->slots));
    // rows of V per slot and pass: the chunk of all slots within the budget, at least 2048, at most the option / the data;
    // halved while the buffer does not fit, then the group is
    const int64_t cap = h->chunk > 0 ? std::min<int64_t>(((int64_t)h->chunk + TB - 1) / TB * TB, h->Npad) : h->Npad;
    int64_t rows = (int64_t)(budget / ((double)G * mpm * h->es)) / TB * TB;
    rows = std::min(std::max<int64_t>(rows, 2048), cap);
    rc = ensure_vbuf(u, (int64_t)G * rows);
    while (rc == GPHIP_ERR_HIP && (rows > 2048 || G > 1)) {
        (void)hipGetLastError();
        if (rows > 2048) rows = std::min(cap, std::max<int64_t>(2048, (rows / 2 + TB - 1) / TB * TB));
        else G = (G + 1) / 2;
        u->vcap = 0;
        rc = ensure_vbuf(u, (int64_t)G * rows);
    }
    if (rc) { (void)hipGetLastError(); return sfail(h, rc, "no device memory for a chunk of V: " + u->err); }
    h->last_chunk = (int)rows;
    if ((rc = sparse_ensure_rz(h, G, rows))) return rc;
    if ((rc = sparse_ensure_par(h, G))) return rc;
    *G_out = G; *rows_out = rows;
    return GPHIP_OK;
}

// gphip_sparse_bound_batch (DESIGN.md section 8f): the bound for the B rows of Theta, one theta per workspace slot, the group
// evaluator on group after group.  No fit is left resident; a row that fails has only its own info / out to show for it.
// pw: B x N point-dependent arrays, row s for row s of Theta.  six: parts are B x 6, those of gphip_sparse_bound_pw.
int sparse_eval_batch(gphip_sparse_ctx* h, const double* Theta, int B, int p, double jitter, double* out, double* parts, int* info,
                      const SparsePw& pw = SparsePw{}, bool six = false) {
    const double qnan = std::nan("");
    h->fitted = false;
    sparse_reset_phases(h, PH_KUU_FACTOR, PH_JOINT_V);
    HIPCHK(hipSetDevice(h->device));
    int G = 0;
    int64_t rows = 0;
    int rc = sparse_size_groups(h, B, &G, &rows);
    if (rc) return rc;
    SparsePhases ph(h);
    std::vector<SparseSlot> res((size_t)G);
    for (int s0 = 0; s0 < B; s0 += G) {
        const int nb = std::min(G, B - s0);
        h->last_slots = nb;
        if ((rc = sparse_group(h, Theta + (size_t)s0 * p, nb, p, jitter, rows, SparseKeep::nothing, nullptr, pw.rows_from(s0, h->N), ph, res.data())))
            return rc;
        const int np = six ? 6 : 5;
        for (int s = 0; s < nb; ++s) {
            const SparseSlot& r = res[(size_t)s];
            info[s0 + s] = r.info;
            out[s0 + s] = r.info == 0 ? r.F : qnan;
            if (parts) {
                double* ps = parts + (size_t)(s0 + s) * np;
                if (six) r.put_parts_pw(ps, h->N, h->m);
                else r.put_parts(ps);
                if (r.info != 0) for (int k = 0; k < np; ++k) ps[k] = qnan;
            }
        }
        ph.harvest();                          // (group by group: the events go back to the pool for the next one)
    }
    return GPHIP_OK;
}

// Gradients in the test inputs (gphip_sparse_predict_grad, DESIGN.md section 8j): what the prediction pass adds per chunk for the
// ONE slot of the resident fit.  dmean / dvar: the call's row-major M x d outputs (dvar null: not wanted).
struct SparseXGrad { double* dmean; double* dvar; };

// a_mu = L_u^-T L_B^-T c into u->dAlpha, once per call: b's single-vector backward launch (queue_alpha: c sits in b's rhs row), then
// u's on that vector (the row route where the launch is unavailable); b hands over through an event.
template <typename T>
int sparse_queue_amu(gphip_sparse_ctx* h) {
    gphip_ctx *u = h->u, *b = h->b;
    const int64_t mpm = u->Npad;
    int rc;
    HIPCHK(b->dAlpha.grow((size_t)mpm * sizeof(T)));
    HIPCHK(u->dAlpha.grow((size_t)mpm * sizeof(T)));
    if ((rc = queue_alpha<T>(b))) return sfail(h, rc, b->err);
    hipEvent_t e = get_event(u);
    const hipError_t e1 = hipEventRecord(e, b->stream), e2 = hipStreamWaitEvent(u->stream, e, 0);
    u->pool.push_back(e);                      // (the wait holds what was recorded)
    HIPCHK(e1);
    HIPCHK(e2);
    if (trsv_ok(u, 1)) {
        T *z = trsv_input<T>(u), *x = nullptr;
        HIPCHK(hipMemcpyAsync(z, b->dAlpha.p, (size_t)mpm * sizeof(T), hipMemcpyDeviceToDevice, u->stream));
        rc = queue_trsv_fill<T>(u, 1, 1);
        if (!rc) rc = queue_trsv<T>(u, z, 0, 1, true, &x);
        if (rc) return sfail(h, rc, u->err);
        HIPCHK(hipMemcpyAsync(u->dAlpha.p, x, (size_t)mpm * sizeof(T), hipMemcpyDeviceToDevice, u->stream));
        return GPHIP_OK;
    }
    HIPCHK(hipMemsetAsync(u->dV.p, 0, (size_t)TB * mpm * sizeof(T), u->stream));
    HIPCHK(hipMemcpy2DAsync(u->dV.p, (size_t)TB * sizeof(T), b->dAlpha.p, sizeof(T), sizeof(T), (size_t)mpm, hipMemcpyDeviceToDevice, u->stream));
    queue_backward_rows<T>(u, TB);
    HIPCHK(hipMemcpy2DAsync(u->dAlpha.p, sizeof(T), u->dV.p, (size_t)TB * sizeof(T), sizeof(T), (size_t)mpm, hipMemcpyDeviceToDevice, u->stream));
    return GPHIP_OK;
}

// One chunk of the gradients, after the pass has left V1 in u's dV and V2 in b's: b's stream takes V2 to L_B^-T V2 and forms
// V1 - sn^2 (that) in place, hands it to u through the event `back`, u's stream substitutes with L_u (W = L_u^-T (..), refined
// unless option "sparse_pgrad_refine" = 0), reduces against the scaled Z and downloads the chunk's rows.
template <typename T>
int sparse_queue_pgrad(gphip_sparse_ctx* h, const SparseXGrad& xg, int64_t m0, int64_t mc, int64_t mpad, hipEvent_t back, SparsePhases& ph) {
    gphip_ctx *u = h->u, *b = h->b;
    int rc;
    if (xg.dvar) {
        {
            SparseScope ps(ph, PH_PGRAD_BACKWARD, b->stream);
            if ((rc = queue_backward_rows<T>(b, mpad))) return sfail(h, rc, b->err);
            const long n = (long)mpad * u->Npad;
            hipLaunchKernelGGL(sparse_xgrad_combine_kernel<T>, dim3((unsigned)std::min<long>((n + 255) / 256, 4096)), dim3(256), 0, b->stream,
                               (const T*)u->dV.p, (T*)b->dV.p, n, h->sn2_fit);
        }
        HIPCHK(hipEventRecord(back, b->stream));
        HIPCHK(hipStreamWaitEvent(u->stream, back, 0));
        {
            SparseScope ps(ph, PH_PGRAD_BACKWARD, u->stream);
            rc = h->pgrad_refine ? queue_backward_rows<T>(u, mpad, b->dV.p, h->dLd.p, h->dRes.p) : queue_backward_rows<T>(u, mpad, b->dV.p);
            if (rc) return sfail(h, rc, u->err);
        }
    }
    {
        SparseScope ps(ph, PH_PGRAD_REDUCE, u->stream);
        if ((rc = queue_xgrad<T>(u, b->dV.p, u->dAlpha.p, mc, mpad, xg.dvar != nullptr, u->predict_grad_split, &u->predict_grad_nsplit)))
            return sfail(h, rc, u->err);
    }
    const int64_t d = u->d;
    const double* out = u->dXgOut.as<double>();
    HIPCHK(hipMemcpyAsync(xg.dmean + m0 * d, out, (size_t)(mc * d) * 8, hipMemcpyDeviceToHost, u->stream));
    if (xg.dvar) HIPCHK(hipMemcpyAsync(xg.dvar + m0 * d, out + mpad * d, (size_t)(mc * d) * 8, hipMemcpyDeviceToHost, u->stream));
    return GPHIP_OK;
}

// The prediction pass of gphip_sparse_predict[_pw] and gphip_sparse_predict_samples[_pw] (DESIGN.md section 8h): mean and variance
// at the M test points X for the nb slots whose factors u and b hold, MC points at a time, every launch with the slot as its last
// grid index:
//   u   stage_test_chunk (k_s(X*, Z) of all slots), the forward substitution of all slots, k_s(x*, x*) of a run-time compiled
//       kernel, the hand-over: V1 into b's dV and the strip partials of |v1|^2 (sparse_handover_kernel; option
//       "sparse_samples_handover" = 0: a copy and the exact path's partial launch on u, whose dots nobody reads)
//   b   (its stream waits for an event of u's, not the host) the forward substitution of all slots, the partial launch against c,
//       the finishing kernel
// and one staged download per chunk, which the host scatters: row s to mean / var + s stride.  resident: the factors are the fit's
// (one slot).  Else u_factored / b_factored: every slot has a factor there -- a launch that spin-waits (the dataflow substitution)
// runs on a context only then (queue_forward_slots).  pwt: nb rows of M values of m(x*) and nu(x*), which take the place of mu and
// sn^2 in the finishing kernel.  info (null: every row is good): a row whose info is not 0 gets NaN.  xg (gphip_sparse_predict_grad,
// the resident slot only): every chunk goes on to the gradients in its test points (sparse_queue_pgrad) before it is downloaded.
int sparse_predict_pass(gphip_sparse_ctx* h, const double* X, int64_t M, int64_t MC, int nb, bool resident, bool u_factored, bool b_factored,
                        const SparsePw& pwt, int latent, double* mean, double* var, int64_t stride, const int* info, SparsePhases& ph,
                        const SparseXGrad* xg = nullptr) {
    gphip_ctx *u = h->u, *b = h->b;
    const double qnan = std::nan("");
    const int64_t mpm = u->Npad;
    int rc = GPHIP_OK;
    std::vector<double> xt, hm, hv;
    struct Handed { gphip_ctx* u; hipEvent_t e; ~Handed() { if (e) u->pool.push_back(e); } } handed{u, get_event(u)}, back{u, xg ? get_event(u) : nullptr};
    for (int64_t m0 = 0; m0 < M; m0 += MC) {
        const int64_t mc = std::min(MC, M - m0);
        int64_t mpad = 0;
        int ns1 = 0, ns2 = 0;
        {
            SparseScope ps(ph, PH_SAMPLES_VU, u->stream);
            // (ranged = false: u builds k(x*, Z) with the direct form, kbuild_mfma = 0 -- no verdict of the MFMA kernel build to guard)
            mpad = stage_test_chunk(u, X, m0, mc, nb, 0, xt, &rc, false);
            if (rc) return sfail(h, rc, u->err);
            queue_forward_slots(u, mpad, nb, resident, u_factored);
            if (h->custom && (rc = queue_custom_kss(u, mc, mpad, nb))) return sfail(h, rc, u->err);
        }
        long p1_sstride = (long)mpad, p1_off = 0;
        {
            SparseScope ps(ph, PH_SAMPLES_HANDOVER, u->stream);
            if (h->samples_handover) {
                if ((rc = DISPATCH(h, sparse_queue_handover, h, mpad, nb, &ns1))) return rc;
            } else {                           // the two launches it replaces; the norm rows are the second of each strip's two
                HIPCHK(hipMemcpyAsync(b->dV.p, u->dV.p, (size_t)nb * mpad * mpm * h->es, hipMemcpyDeviceToDevice, u->stream));
                if ((rc = DISPATCH(u, queue_predict_partial, u, mpad, nb, false, &ns1))) return sfail(h, rc, u->err);
                p1_sstride = 2l * mpad; p1_off = (long)mpad;
            }
        }
        HIPCHK(hipEventRecord(handed.e, u->stream));
        HIPCHK(hipStreamWaitEvent(b->stream, handed.e, 0));
        {
            SparseScope ps(ph, PH_SAMPLES_VB, b->stream);
            queue_forward_slots(b, mpad, nb, resident, b_factored);
        }
        {
            SparseScope ps(ph, PH_SAMPLES_REDUCE, b->stream);
            if ((rc = DISPATCH(b, queue_predict_partial, b, mpad, nb, false, &ns2))) return sfail(h, rc, b->err);
            const double *d_mt = nullptr, *d_nt = nullptr;
            if ((rc = sparse_stage_test_arrays(h, pwt, M, m0, mc, mpad, nb, latent, &d_mt, &d_nt))) return rc;
            // (mu, B's sn^2, k(x, x) and the noise of every slot are in dPar since the evaluation)
            hipLaunchKernelGGL(sparse_predict_finish_kernel, dim3((unsigned)((mc + 255) / 256), (unsigned)nb), dim3(256), 0, b->stream,
                               u->dPart.as<double>() + p1_off, ns1, p1_sstride, (long)ns1 * p1_sstride, b->dPart.as<double>(), ns2,
                               (long)mpad, (int)mc, h->dPar.as<double>(), h->custom ? u->dKss.as<double>() : nullptr, latent ? 1 : 0,
                               d_mt, d_nt, b->dMean.as<double>(), b->dVar.as<double>());
        }
        hm.resize((size_t)nb * mpad);
        hv.resize((size_t)nb * mpad);
        HIPCHK(hipMemcpyAsync(hm.data(), b->dMean.p, hm.size() * 8, hipMemcpyDeviceToHost, b->stream));
        HIPCHK(hipMemcpyAsync(hv.data(), b->dVar.p, hv.size() * 8, hipMemcpyDeviceToHost, b->stream));
        if (xg && (rc = DISPATCH(h, sparse_queue_pgrad, h, *xg, m0, mc, mpad, back.e, ph))) return rc;
        if ((rc = complete_call(b))) return sfail(h, rc, b->err);      // (b's stream waited for u's: both are idle)
        if ((rc = complete_call(u))) return sfail(h, rc, u->err);      // (the abort word of u's substitution)
        for (int s = 0; s < nb; ++s) {
            const bool good = !info || info[s] == 0;
            double* ms = mean + (size_t)s * stride + m0;
            double* vs = var + (size_t)s * stride + m0;
            for (int64_t t = 0; t < mc; ++t) {
                ms[t] = good ? hm[(size_t)s * mpad + t] : qnan;
                vs[t] = good ? hv[(size_t)s * mpad + t] : qnan;
            }
        }
    }
    return GPHIP_OK;
}

// gphip_sparse_predict_samples (DESIGN.md section 8h): mean and variance at the M test points for the S rows of Thetas.  Group
// after group (sparse_eval_batch's rule) the group evaluator leaves the factors of every slot of u and b (SparseKeep::group) and
// the prediction pass substitutes with them.
// pw: S x N training arrays; pwt: S x M arrays of m(x*) and nu(x*).
int sparse_predict_samples(gphip_sparse_ctx* h, const double* Thetas, int S, int p, double jitter, const double* X, int64_t M, int latent,
                           double* mean, double* var, double* bound, int* info, const SparsePw& pw = SparsePw{}, const SparsePw& pwt = SparsePw{}) {
    gphip_ctx *u = h->u, *b = h->b;
    const double qnan = std::nan("");
    h->fitted = false;
    sparse_reset_phases(h, PH_KUU_FACTOR, PH_JOINT_V);
    sparse_reset_phases(h, PH_SAMPLES_VU, PH_COUNT);
    HIPCHK(hipSetDevice(h->device));
    int G = 0;
    int64_t rows = 0;
    int rc = sparse_size_groups(h, S, &G, &rows);
    if (rc) return rc;
    // test points per pass (gphip_predict_samples' rule): at most 2048, the group's V within the ~8 GiB budget in u's dV and in
    // b's, at most the option; halved while the two buffers do not fit
    const int64_t mpm = u->Npad;
    int64_t MC = (int64_t)((8.0 * (1 << 30)) / ((double)G * mpm * h->es)) / TB * TB;
    MC = std::min<int64_t>(std::max<int64_t>(MC, TB), 2048);
    MC = std::min(MC, (M + TB - 1) / TB * TB);
    if (h->samples_chunk > 0) MC = std::min(MC, ((int64_t)h->samples_chunk + TB - 1) / TB * TB);
    for (;;) {
        if (!(rc = ensure_vbuf(u, (int64_t)G * MC))) rc = ensure_vbuf(b, (int64_t)G * MC);
        if (rc != GPHIP_ERR_HIP || MC <= TB) break;
        (void)hipGetLastError();
        MC = (MC / 2 + TB - 1) / TB * TB;
    }
    if (rc) { (void)hipGetLastError(); return sfail(h, rc, "no device memory for the test points' V of a group"); }
    h->last_samples_chunk = (int)MC;
    SparsePhases ph(h);
    std::vector<SparseSlot> res((size_t)G);
    for (int s0 = 0; s0 < S; s0 += G) {
        const int nb = std::min(G, S - s0);
        h->last_slots = nb;
        if ((rc = sparse_group(h, Thetas + (size_t)s0 * p, nb, p, jitter, rows, SparseKeep::group, nullptr, pw.rows_from(s0, h->N), ph, res.data())))
            return rc;
        bool u_factored = true, b_factored = true;
        for (int s = 0; s < nb; ++s) {
            const SparseSlot& r = res[(size_t)s];
            info[s0 + s] = r.info;
            if (bound) bound[s0 + s] = r.info == 0 ? r.F : qnan;
            if (r.uinfo != 0) u_factored = false;
            if (b->hInfo.as<int>()[s] != 0) b_factored = false;
        }
        if ((rc = sparse_predict_pass(h, X, M, MC, nb, false, u_factored, b_factored, pwt.rows_from(s0, M), latent, mean + (size_t)s0 * M,
                                      var + (size_t)s0 * M, M, info + s0, ph)))
            return rc;
        ph.harvest();                          // (group by group: the events go back to the pool for the next one)
    }
    return GPHIP_OK;
}

int sparse_create(const void* X, const void* y, int64_t N, int64_t d, const void* Z, int64_t m, int kernel_id, const char* body, int ncp,
                  int mean_id, int dtype, int device, gphip_sparse_handle* out) {
    if (!out) return GPHIP_ERR_ARG;
    *out = nullptr;
    if (!X || !y || !Z) return GPHIP_ERR_ARG;
    if (N < 1 || d < 1 || m < 1 || m > SPARSE_MAX_M) return GPHIP_ERR_DIM;
    if (!body && kernel_id == GPHIP_KERNEL_NULL) return GPHIP_ERR_UNSUPPORTED;
    if (!body && kernel_id == GPHIP_KERNEL_CUSTOM) return GPHIP_ERR_ARG;
    gphip_sparse_ctx* h = new gphip_sparse_ctx;
    h->dtype = dtype; h->es = dtype == 64 ? 8 : 4;
    h->N = N; h->d = d; h->Npad = (N + TB - 1) / TB * TB;
    h->kernel_id = kernel_id; h->mean_id = mean_id; h->device = device;
    if (body) { h->custom = true; h->body = body; h->ncp = ncp; }
    auto bail = [&](int code) { gphip_sparse_destroy(h); return code; };
    int rc = sparse_make_children(h, static_cast<const double*>(Z), m);
    if (rc) {
        if (body) g_create_error = h->err;
        return bail(rc);
    }
    const double* Xd = static_cast<const double*>(X);
    const double* yd = static_cast<const double*>(y);
    std::vector<double> xt((size_t)d * h->Npad, 0.0), yp((size_t)h->Npad, 0.0);
    for (int64_t i = 0; i < N; ++i) {
        for (int64_t j = 0; j < d; ++j) xt[(size_t)j * h->Npad + i] = Xd[i * d + j];
        yp[(size_t)i] = yd[i];
    }
    if (hipSetDevice(h->device) != hipSuccess) return bail(GPHIP_ERR_HIP);
    if (h->dXt.grow(xt.size() * h->es) != hipSuccess || h->dY.grow(yp.size() * h->es) != hipSuccess) { (void)hipGetLastError(); return bail(GPHIP_ERR_HIP); }
    if (DISPATCH(h->u, upload, h->u, h->dXt.p, xt, h->u->stream) != GPHIP_OK) return bail(GPHIP_ERR_HIP);
    if (DISPATCH(h->u, upload, h->u, h->dY.p, yp, h->u->stream) != GPHIP_OK) return bail(GPHIP_ERR_HIP);
    if (DISPATCH(h, sparse_func_attrs, h) != GPHIP_OK) return bail(GPHIP_ERR_HIP);
    *out = h;
    return GPHIP_OK;
}


// ---- joint prediction (DESIGN.md section 8g)

int sparse_joint_dim_check(gphip_sparse_ctx* h, int64_t M) {
    if (M < 1) return sfail(h, GPHIP_ERR_DIM, "M < 1");
    if (M > JOINT_MAX_M) return sfail(h, GPHIP_ERR_DIM, "M above GPHIP_JOINT_MAX_M (all rows of V1 and V2 must be resident at once)");
    return GPHIP_OK;
}

int sparse_joint_state_check(gphip_sparse_ctx* h) {
    if (!h->fitted || !has_fit(h->u) || !has_fit(h->b)) return sfail(h, GPHIP_ERR_STATE, "joint prediction before a successful gphip_sparse_fit");
    if (h->pw_fit) return sfail(h, GPHIP_ERR_UNSUPPORTED, "no joint prediction after a fit with a point-dependent mean or noise");
    return GPHIP_OK;
}

// the rhs-row operand -c / sn^2 of the V2 segment: from b's rhs tile row into u's dJZ, on b's stream
template <typename T>
void sparse_queue_cblock(gphip_sparse_ctx* h, int64_t kseg) {
    gphip_ctx *u = h->u, *b = h->b;
    hipLaunchKernelGGL(joint_cblock_kernel<T>, dim3((unsigned)((kseg + 255) / 256)), dim3(256), 0, b->stream, (const T*)b->dA.p, (int)b->R,
                       (int)kseg, h->sn2_fit, (T*)u->dJZ.p, (long)kseg);
}

// the two-segment downdate of the child's workspace: Sigma = K(X*, X*) - V1^T V1 + sn^2 V2^T V2
template <typename T>
int sparse_queue_joint_downdate(gphip_sparse_ctx* h, int64_t mpad) {
    return queue_downdate_any<T, true>(h->u, h->u->joint, mpad, h->joint_split, &h->joint_nsplit, h->sn2_fit);
}

// Everything up to Sigma in the workspace of u's child: V1 on u, V2 and the rhs-row operand on b, then build + downdate on the
// child.  The child's diagonal carries k(x*, x*) + (noisy: sn^2) + (*jitter_io, which a negative value turns into the default).
int sparse_joint_sigma(gphip_sparse_ctx* h, const double* Xs, int64_t M, const double* ystar, bool noisy, double* jitter_io,
                       SparsePhases& ph) {
    gphip_ctx *u = h->u, *b = h->b;
    HIPCHK(hipSetDevice(h->device));
    sparse_reset_phases(h, PH_JOINT_V, PH_SAMPLES_VU);
    const int64_t mpad = (M + TB - 1) / TB * TB, kseg = u->Npad;
    const size_t seg_bytes = (size_t)mpad * kseg * h->es;
    int rc = ensure_vbuf(u, 2 * mpad);         // u's dV takes both segments: [V1 | V2], mpad x 2 kseg with ld mpad
    if (!rc) rc = ensure_vbuf(b, mpad);
    if (rc) { (void)hipGetLastError(); return sfail(h, GPHIP_ERR_HIP, "joint prediction: no device memory for all M rows of V1 and V2"); }
    HIPCHK(u->dJZ.grow((size_t)TB * 2 * kseg * h->es));
    HIPCHK(hipMemsetAsync(u->dJZ.p, 0, (size_t)TB * 2 * kseg * h->es, u->stream));
    std::vector<double> xt;
    {
        SparseScope ps(ph, PH_JOINT_V, u->stream);
        stage_test_chunk(u, Xs, 0, M, 1, 0, xt, &rc, false);      // all M rows as one chunk
        if (rc) return sfail(h, rc, u->err);
        queue_forward_fit(u, mpad);
    }
    double kss_mean = 0.0;                     // (run-time compiled kernels: k(x*, x*) is a function of the point)
    if (jitter_io && *jitter_io < 0.0 && h->custom && (rc = joint_mean_kss(u, M, mpad, &kss_mean))) return sfail(h, rc, u->err);
    if ((rc = complete_call(u))) return sfail(h, rc, u->err);
    {
        // V2 = L_B^-1 V1: the same rows through b's factor, then next to V1; the rhs-row operand from b's rhs row
        SparseScope ps(ph, PH_JOINT_V, b->stream);
        HIPCHK(hipMemcpyAsync(b->dV.p, u->dV.p, seg_bytes, hipMemcpyDeviceToDevice, b->stream));
        queue_forward_fit(b, mpad);
        HIPCHK(hipMemcpyAsync(static_cast<char*>(u->dV.p) + seg_bytes, b->dV.p, seg_bytes, hipMemcpyDeviceToDevice, b->stream));
        DISPATCH(h, sparse_queue_cblock, h, kseg);
    }
    if ((rc = complete_call(b))) return sfail(h, rc, b->err);
    if ((rc = joint_child(u, Xs, M, ystar))) return sfail(h, rc, u->err);
    gphip_ctx* c = u->joint;
    {
        SparseScope ps(ph, PH_JOINT_BUILD, c->stream);
        rc = joint_build(u, noisy, jitter_io, kss_mean);
    }
    if (rc) return sfail(h, rc, u->err);
    {
        SparseScope ps(ph, PH_JOINT_DOWNDATE, c->stream);
        rc = DISPATCH(h, sparse_queue_joint_downdate, h, mpad);
    }
    return rc ? sfail(h, rc, u->err) : GPHIP_OK;
}

// the event pair of the factorisation of Sigma while option "profile" is on
struct SparseFactorEvents {
    hipEvent_t ev[2];
    bool on;
    SparseFactorEvents(gphip_sparse_ctx* h) : on(h->profile > 0) {
        if (on) { ev[0] = get_event(h->u); ev[1] = get_event(h->u); }
    }
    hipEvent_t* get() { return on ? ev : nullptr; }
    void hand_over(SparsePhases& ph) {
        if (on) ph.recs.push_back(SparsePhase{PH_JOINT_FACTOR, ev[0], ev[1]});
    }
};

// One table for gphip_sparse_set_option / gphip_sparse_get_option (as option_slot is for the exact path): the object's own integer
// options -- OPT_NONNEG: a negative value is refused, OPT_FLAG: stored as 0 / 1 -- and, OPT_RESULT, the results of the last call,
// which can be read only (setting one goes where every name the object does not own goes: to u and b).
enum { OPT_NONNEG = 1, OPT_FLAG = 2, OPT_RESULT = 4 };
struct SparseOption { const char* name; int gphip_sparse_ctx::*field; int kind; };
const SparseOption* sparse_option(const char* name) {
    static const SparseOption table[] = {
        {"sparse_chunk", &gphip_sparse_ctx::chunk, OPT_NONNEG}, {"sparse_split", &gphip_sparse_ctx::split, OPT_NONNEG},
        {"profile", &gphip_sparse_ctx::profile, 0}, {"sparse_joint_split", &gphip_sparse_ctx::joint_split, OPT_NONNEG},
        {"sparse_batch_slots", &gphip_sparse_ctx::batch_slots, OPT_NONNEG}, {"sparse_samples_chunk", &gphip_sparse_ctx::samples_chunk, OPT_NONNEG},
        {"sparse_samples_handover", &gphip_sparse_ctx::samples_handover, OPT_FLAG}, {"sparse_pw_fused", &gphip_sparse_ctx::pw_fused, OPT_FLAG},
        {"sparse_pgrad_refine", &gphip_sparse_ctx::pgrad_refine, OPT_FLAG},
        {"grad_analytic", &gphip_sparse_ctx::grad_analytic, OPT_RESULT}, {"last_sparse_chunk", &gphip_sparse_ctx::last_chunk, OPT_RESULT},
        {"last_sparse_nsplit", &gphip_sparse_ctx::last_nsplit, OPT_RESULT}, {"last_sparse_slots", &gphip_sparse_ctx::last_slots, OPT_RESULT},
        {"last_sparse_samples_chunk", &gphip_sparse_ctx::last_samples_chunk, OPT_RESULT},
        {"last_sparse_joint_nsplit", &gphip_sparse_ctx::joint_nsplit, OPT_RESULT},
    };
    for (const SparseOption& o : table)
        if (!strcmp(name, o.name)) return &o;
    return nullptr;
}

}  // namespace

extern "C" {

int gphip_sparse_create(const void* X, const void* y, int64_t N, int64_t d, const void* Z, int64_t m, int kernel_id, int mean_id, int dtype,
                        int device, gphip_sparse_handle* out) {
    return sparse_create(X, y, N, d, Z, m, kernel_id, nullptr, 0, mean_id, dtype, device, out);
}

int gphip_sparse_create_custom(const void* X, const void* y, int64_t N, int64_t d, const void* Z, int64_t m, const char* body, int nparams,
                               int mean_id, int dtype, int device, gphip_sparse_handle* out) {
    g_create_error.clear();
    if (!out) return GPHIP_ERR_ARG;
    *out = nullptr;
    if (!body || !*body || nparams < 0 || nparams > 4096) { g_create_error = "null / empty function body or bad parameter count"; return GPHIP_ERR_ARG; }
    return sparse_create(X, y, N, d, Z, m, GPHIP_KERNEL_CUSTOM, body, nparams, mean_id, dtype, device, out);
}

int gphip_sparse_destroy(gphip_sparse_handle h) {
    if (!h) return GPHIP_OK;
    {
        std::lock_guard<std::recursive_mutex> lk(h->mu);
        if (h->u && h->u->paths_live > 0)
            return sfail(h, GPHIP_ERR_STATE, "gphip_sparse_destroy with live paths objects: gphip_paths_destroy them first");
    }
    if (h->u) {
        (void)hipSetDevice(h->u->device);
        (void)hipStreamSynchronize(h->u->stream);
    }
    if (h->b) (void)hipStreamSynchronize(h->b->stream);
    if (h->u) gphip_destroy(h->u);
    if (h->b) gphip_destroy(h->b);
    (void)hipSetDevice(h->device);
    delete h;                                  // (the buffers free themselves)
    return GPHIP_OK;
}

int gphip_sparse_set_inducing(gphip_sparse_handle h, const void* Z, int64_t m) {
    if (!h || !Z) return sfail(h, GPHIP_ERR_ARG, "null argument");
    if (m < 1 || m > SPARSE_MAX_M) return sfail(h, GPHIP_ERR_DIM, "m < 1 or above GPHIP_SPARSE_MAX_M");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (m != h->m) {                           // (new contexts: a paths object borrows the old one of K_uu)
        if (h->u->paths_live > 0)
            return sfail(h, GPHIP_ERR_STATE, "gphip_sparse_set_inducing with another m and live paths objects: gphip_paths_destroy them first");
        return sparse_make_children(h, static_cast<const double*>(Z), m);
    }
    // the same number of inducing points: both contexts keep their buffers, streams, options and compiled programs; the points
    // and what create_ctx derives from them are replaced, the fit is dropped
    h->fitted = false;
    for (gphip_ctx* c : {h->u, h->b})
        if (const int rc = ctx_replace_points(c, static_cast<const double*>(Z))) return sfail(h, rc, "replacing the inducing points failed: " + c->err);
    return GPHIP_OK;
}

int gphip_sparse_num_params(gphip_sparse_handle h, int* p) {
    if (!h || !p) return GPHIP_ERR_ARG;
    *p = h->u->p;
    return GPHIP_OK;
}

int gphip_sparse_bound(gphip_sparse_handle h, const double* theta, int p, double jitter, double* out, double* parts, int* info) {
    if (!h || !theta || !out || !info) return sfail(h, GPHIP_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    return sparse_eval(h, theta, p, jitter, out, parts, info);
}

int gphip_sparse_bound_batch(gphip_sparse_handle h, const double* Theta, int B, int p, double jitter, double* out, double* parts,
                             int* info) {
    if (!h || !Theta || !out || !info) return sfail(h, GPHIP_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (const int rc = sparse_check_args(h, p, jitter)) return rc;
    if (B <= 0) return GPHIP_OK;
    return sparse_eval_batch(h, Theta, B, p, jitter, out, parts, info);
}

int gphip_sparse_bound_pw(gphip_sparse_handle h, const double* theta, int p, double jitter, const double* mean_train,
                          const double* nugget_train, double* out, double* parts, int* info) {
    if (!h || !theta || !out || !info) return sfail(h, GPHIP_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    // (no array: the constant call itself -- the same bytes in out and info -- with its five parts converted on the host)
    return sparse_eval(h, theta, p, jitter, out, parts, info, nullptr, nullptr, SparsePw{mean_train, nugget_train}, true);
}

int gphip_sparse_bound_batch_pw(gphip_sparse_handle h, const double* Theta, int B, int p, double jitter, const double* mean_train,
                                const double* nugget_train, double* out, double* parts, int* info) {
    if (!h || !Theta || !out || !info) return sfail(h, GPHIP_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (const int rc = sparse_check_args(h, p, jitter)) return rc;
    if (B <= 0) return GPHIP_OK;
    return sparse_eval_batch(h, Theta, B, p, jitter, out, parts, info, SparsePw{mean_train, nugget_train}, true);
}

int gphip_sparse_fit_pw(gphip_sparse_handle h, const double* theta, int p, double jitter, const double* mean_train, const double* nugget_train,
                        int* info) {
    if (!h || !theta || !info) return sfail(h, GPHIP_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    return sparse_eval(h, theta, p, jitter, nullptr, nullptr, info, nullptr, nullptr, SparsePw{mean_train, nugget_train});
}

int gphip_sparse_nested_sampling(gphip_sparse_handle h, double jitter, const double* box, const int* prior_kind, gphip_logprior_fn logprior,
                                 void* user, const gphip_ns_options* opts, const double* start, int64_t cap, double* points, double* loglik,
                                 double* logprior_out, double* accept_rate, int64_t* n_samples, double* log_evidence, int64_t* n_evals) {
    if (!h) return GPHIP_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (const int rc = sparse_check_args(h, h->u->p, jitter)) return rc;
    return ns_run(h->u->p,
                  [&](const double* Theta, int B, int p, double* out, int* info) {
                      return gphip_sparse_bound_batch(h, Theta, B, p, jitter, out, nullptr, info);
                  },
                  [&](int code, const char* msg) { return sfail(h, code, msg); }, box, prior_kind, logprior, user, opts, start, cap, points,
                  loglik, logprior_out, accept_rate, n_samples, log_evidence, n_evals);
}

int gphip_sparse_bound_grad(gphip_sparse_handle h, const double* theta, int p, double jitter, double* out, double* grad, double* parts,
                            int* info) {
    if (!h || !theta || !out || !grad || !info) return sfail(h, GPHIP_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    gphip_ctx* u = h->u;
    if (const int rc = sparse_check_args(h, p, jitter)) return rc;
    h->grad_analytic = 0;
    if (h->custom) {
        if (const int rc = ensure_custom_grad(u)) return sfail(h, rc, u->err);
    }
    if (!h->custom || (u->custom_grad && u->cgrad_state == 1)) {
        const int rc = sparse_eval(h, theta, p, jitter, out, parts, info, grad);
        if (!rc && *info == 0) h->grad_analytic = 1;
        return rc;
    }
    // No dual-number program (it does not compile, more than 64 parameters, option custom_grad = 0): central differences of the
    // bound with gphip_loglik_grad's step, the jitter held at the unperturbed call's value.  The unperturbed evaluation comes last
    // so that its fit stays resident; a default jitter (< 0) has to be found by an evaluation of its own first.
    const double qnan = std::nan("");
    for (int k = 0; k < p; ++k) grad[k] = qnan;
    double jit = jitter;
    int rc = GPHIP_OK;
    if (jit < 0.0) {
        if ((rc = sparse_eval(h, theta, p, jitter, out, nullptr, info))) return rc;
        if (*info != 0) { if (parts) for (int k = 0; k < 5; ++k) parts[k] = qnan; return GPHIP_OK; }
        jit = h->last_jitter;
    }
    std::vector<double> th(theta, theta + p), g((size_t)p, qnan);
    for (int k = 0; k < p; ++k) {
        const double step = fd_step(u, theta[k]);
        double fp = 0.0, fm = 0.0;
        int ip = 0, im = 0;
        th[(size_t)k] = theta[k] + step;
        if ((rc = sparse_eval(h, th.data(), p, jit, &fp, nullptr, &ip))) return rc;
        th[(size_t)k] = theta[k] - step;
        if ((rc = sparse_eval(h, th.data(), p, jit, &fm, nullptr, &im))) return rc;
        th[(size_t)k] = theta[k];
        if (ip == 0 && im == 0) g[(size_t)k] = (fp - fm) / (2.0 * step);
    }
    if ((rc = sparse_eval(h, theta, p, jitter, out, parts, info))) return rc;
    if (*info == 0) for (int k = 0; k < p; ++k) grad[k] = g[(size_t)k];
    return GPHIP_OK;
}

int gphip_sparse_bound_grad_inducing(gphip_sparse_handle h, const double* theta, int p, double jitter, double* out, double* grad,
                                     double* gradZ, double* parts, int* info) {
    if (!h || !theta || !out || !gradZ || !info) return sfail(h, GPHIP_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (const int rc = sparse_check_args(h, p, jitter)) return rc;
    // (a run-time compiled function would need its dual-number program seeded in the coordinates: not built)
    if (h->custom) return sfail(h, GPHIP_ERR_UNSUPPORTED, "no gradient in the inducing locations for a run-time compiled covariance function");
    h->grad_analytic = 0;
    const int rc = sparse_eval(h, theta, p, jitter, out, parts, info, grad, gradZ);
    if (!rc && *info == 0 && grad) h->grad_analytic = 1;
    return rc;
}

int gphip_sparse_fit(gphip_sparse_handle h, const double* theta, int p, double jitter, int* info) {
    if (!h || !theta || !info) return sfail(h, GPHIP_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    return sparse_eval(h, theta, p, jitter, nullptr, nullptr, info);
}

int gphip_sparse_predict(gphip_sparse_handle h, const void* Xs, int64_t M, int latent, double* mean, double* var) {
    return gphip_sparse_predict_pw(h, Xs, M, latent, nullptr, nullptr, mean, var);
}

int gphip_sparse_predict_pw(gphip_sparse_handle h, const void* Xs, int64_t M, int latent, const double* mean_test, const double* nugget_test,
                            double* mean, double* var) {
    if (!h || !Xs || !mean || !var) return sfail(h, GPHIP_ERR_ARG, "null argument");
    if (M < 1) return sfail(h, GPHIP_ERR_DIM, "M < 1");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    gphip_ctx *u = h->u, *b = h->b;
    if (!h->fitted || !has_fit(u) || !has_fit(b)) return sfail(h, GPHIP_ERR_STATE, "gphip_sparse_predict before a successful gphip_sparse_fit");
    HIPCHK(hipSetDevice(h->device));
    // test points per pass: ensure_vchunk's rule on u up to 32768, at most the option; b's dV takes the same rows
    int64_t MC = std::min<int64_t>(32768, (M + TB - 1) / TB * TB);
    if (h->samples_chunk > 0) MC = std::min(MC, ((int64_t)h->samples_chunk + TB - 1) / TB * TB);
    int rc = ensure_vchunk(u, MC, &MC);
    if (rc) { (void)hipGetLastError(); return sfail(h, rc, "no device memory for the test points' V: " + u->err); }
    if ((rc = ensure_vbuf(b, MC))) { (void)hipGetLastError(); return sfail(h, rc, "no device memory for the test points' V: " + b->err); }
    h->last_samples_chunk = (int)MC;
    sparse_reset_phases(h, PH_SAMPLES_VU, PH_COUNT);
    SparsePhases ph(h);
    // (the fit's one slot: mu, B's sn^2, k(x, x) and the noise of the fit are slot 0 of dPar since the evaluation)
    return sparse_predict_pass(h, static_cast<const double*>(Xs), M, MC, 1, true, true, true, SparsePw{mean_test, nugget_test}, latent, mean, var,
                               M, nullptr, ph);
}

int gphip_sparse_predict_grad(gphip_sparse_handle h, const void* Xs, int64_t M, double* mean, double* var, double* dmean, double* dvar) {
    if (!h || !Xs || !dmean) return sfail(h, GPHIP_ERR_ARG, "null argument");
    if (M < 1) return sfail(h, GPHIP_ERR_DIM, "M < 1");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    gphip_ctx *u = h->u, *b = h->b;
    if (!h->fitted || !has_fit(u) || !has_fit(b)) return sfail(h, GPHIP_ERR_STATE, "gphip_sparse_predict_grad before a successful gphip_sparse_fit");
    if (h->custom) return sfail(h, GPHIP_ERR_UNSUPPORTED, "no gradient in the test inputs for a run-time compiled covariance function");
    if (h->pw_fit) return sfail(h, GPHIP_ERR_UNSUPPORTED, "gphip_sparse_predict_grad after a fit with a point-dependent nugget / mean array");
    HIPCHK(hipSetDevice(h->device));
    int64_t MC = 0;                            // the exact call's chunk rule on u; b's dV takes the same rows
    int rc = xgrad_chunk(u, M, &MC);
    if (rc) { (void)hipGetLastError(); return sfail(h, rc, "no device memory for the test points' V: " + u->err); }
    if ((rc = ensure_vbuf(b, MC))) { (void)hipGetLastError(); return sfail(h, rc, "no device memory for the test points' V: " + b->err); }
    h->last_samples_chunk = (int)MC;
    HIPCHK(h->dLd.grow((size_t)u->Nt * TS * h->es));
    HIPCHK(h->dRes.grow((size_t)MC * TB * h->es));
    sparse_reset_phases(h, PH_SAMPLES_VU, PH_COUNT);
    SparsePhases ph(h);
    if ((rc = DISPATCH(h, sparse_queue_amu, h))) return rc;
    std::vector<double> own_mean, own_var;     // (the pass always downloads both)
    if (!mean) { own_mean.resize((size_t)M); mean = own_mean.data(); }
    if (!var) { own_var.resize((size_t)M); var = own_var.data(); }
    const SparseXGrad xg{dmean, dvar};
    return sparse_predict_pass(h, static_cast<const double*>(Xs), M, MC, 1, true, true, true, SparsePw{}, 0, mean, var, M, nullptr, ph, &xg);
}

int gphip_sparse_predict_samples(gphip_sparse_handle h, const double* Thetas, int S, int p, double jitter, const void* Xs, int64_t M,
                                 int latent, double* mean, double* var, double* bound, int* info) {
    if (!h || !Thetas || !Xs || !mean || !var || !info) return sfail(h, GPHIP_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (const int rc = sparse_check_args(h, p, jitter)) return rc;
    if (S < 1 || M < 1) return sfail(h, GPHIP_ERR_DIM, "S < 1 or M < 1");
    return sparse_predict_samples(h, Thetas, S, p, jitter, static_cast<const double*>(Xs), M, latent, mean, var, bound, info);
}

int gphip_sparse_predict_samples_pw(gphip_sparse_handle h, const double* Thetas, int S, int p, double jitter, const double* mean_train,
                                    const double* nugget_train, const void* Xs, int64_t M, int latent, const double* mean_test,
                                    const double* nugget_test, double* mean, double* var, double* bound, int* info) {
    if (!h || !Thetas || !Xs || !mean || !var || !info) return sfail(h, GPHIP_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (const int rc = sparse_check_args(h, p, jitter)) return rc;
    if (S < 1 || M < 1) return sfail(h, GPHIP_ERR_DIM, "S < 1 or M < 1");
    return sparse_predict_samples(h, Thetas, S, p, jitter, static_cast<const double*>(Xs), M, latent, mean, var, bound, info,
                                  SparsePw{mean_train, nugget_train}, SparsePw{mean_test, nugget_test});
}

int gphip_sparse_predict_cov(gphip_sparse_handle h, const void* Xs, int64_t M, int latent, double* mean, double* cov) {
    if (!h || !Xs || !mean || !cov) return sfail(h, GPHIP_ERR_ARG, "null argument");
    if (int rc = sparse_joint_dim_check(h, M)) return rc;
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (int rc = sparse_joint_state_check(h)) return rc;
    SparsePhases ph(h);
    int rc = sparse_joint_sigma(h, static_cast<const double*>(Xs), M, nullptr, !latent, nullptr, ph);
    if (!rc && (rc = joint_cov_tail(h->u, M, mean, cov))) (void)sfail(h, rc, h->u->err);
    return rc;
}

int gphip_sparse_predict_draws(gphip_sparse_handle h, const void* Xs, int64_t M, int latent, int S, uint64_t seed, const double* z,
                               double jitter, double* out, int* info) {
    if (!h || !Xs || !out || !info) return sfail(h, GPHIP_ERR_ARG, "null argument");
    if (!std::isfinite(jitter)) return sfail(h, GPHIP_ERR_ARG, "non-finite jitter");
    if (int rc = sparse_joint_dim_check(h, M)) return rc;
    if (S < 1) return sfail(h, GPHIP_ERR_DIM, "S < 1");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (int rc = sparse_joint_state_check(h)) return rc;
    *info = GPHIP_INFO_OK;
    SparsePhases ph(h);
    SparseFactorEvents fev(h);
    double jit = jitter;
    int rc = sparse_joint_sigma(h, static_cast<const double*>(Xs), M, nullptr, !latent, &jit, ph);
    if (!rc && (rc = joint_draws_tail(h->u, M, S, seed, z, out, info, fev.get()))) (void)sfail(h, rc, h->u->err);
    fev.hand_over(ph);
    return rc;
}

int gphip_sparse_predict_logpdf(gphip_sparse_handle h, const void* Xs, int64_t M, const double* ystar, double* out, int* info) {
    if (!h || !Xs || !ystar || !out || !info) return sfail(h, GPHIP_ERR_ARG, "null argument");
    if (int rc = sparse_joint_dim_check(h, M)) return rc;
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (int rc = sparse_joint_state_check(h)) return rc;
    for (int64_t j = 0; j < M; ++j)
        if (!std::isfinite(ystar[j])) { *out = NAN; *info = GPHIP_INFO_NAN; return GPHIP_OK; }
    SparsePhases ph(h);
    SparseFactorEvents fev(h);
    int rc = sparse_joint_sigma(h, static_cast<const double*>(Xs), M, ystar, true, nullptr, ph);
    if (!rc && (rc = joint_logpdf_tail(h->u, M, out, info, fev.get()))) (void)sfail(h, rc, h->u->err);
    fev.hand_over(ph);
    return rc;
}

int gphip_sparse_set_option(gphip_sparse_handle h, const char* name, double value) {
    if (!h || !name) return GPHIP_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    const int v = (int)value;
    const SparseOption* o = sparse_option(name);
    if (o && !(o->kind & OPT_RESULT)) {
        if ((o->kind & OPT_NONNEG) && v < 0) return sfail(h, GPHIP_ERR_ARG, std::string(name) + " < 0");
        h->*(o->field) = (o->kind & OPT_FLAG) ? (v != 0) : v;
        return GPHIP_OK;
    }
    int rc = gphip_set_option(h->u, name, value);
    if (!rc) rc = gphip_set_option(h->b, name, value);
    if (rc) return sfail(h, rc, "unknown option");
    h->u->kbuild_mfma = 0;
    for (auto& o : h->forwarded)
        if (o.first == name) { o.second = value; return GPHIP_OK; }
    h->forwarded.emplace_back(name, value);
    return GPHIP_OK;
}

int gphip_sparse_get_option(gphip_sparse_handle h, const char* name, double* value) {
    if (!h || !name || !value) return GPHIP_ERR_ARG;
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    for (int k = 0; k < PH_COUNT; ++k)
        if (!strcmp(name, SPARSE_PHASE_OPTION[k])) { *value = h->ms[k]; return GPHIP_OK; }
    if (const SparseOption* o = sparse_option(name)) { *value = h->*(o->field); return GPHIP_OK; }
    if (!strcmp(name, "last_jitter")) { *value = h->last_jitter; return GPHIP_OK; }         // (the one result that is no integer)
    const int rc = gphip_get_option(h->u, name, value);
    return rc ? sfail(h, rc, "unknown option") : GPHIP_OK;
}

const char* gphip_sparse_last_error(gphip_sparse_handle h) { return h ? h->err.c_str() : "null handle"; }

}  // extern "C"
