// gphip_paths_mix.inc -- the mixture paths object (include/gphip.h: gphip_paths_create_samples / gphip_paths_rows /
// gphip_paths_get_table; DESIGN.md section 8q): pathwise draws over R hyper-parameter rows in ONE object, created in one call and
// evaluated by gphip_paths_eval / gphip_paths_eval_own through one launch sequence.  Included by gphip.hip behind
// gphip_paths.inc.  For the exact object; out of scope: the sparse object, run-time compiled covariance functions,
// point-dependent fits, dealing rows to several devices, device-resident inputs and outputs.
//
//   create   host: row_of / start; gphip_rff_table(theta_r, F, seeds[r]) per row -> Omega_r, b_r, a_r
//            paths_mix_weights_kernel                  w and a_r w for all draws
//            paths_mix_kernel<GenFeature>, shared      f~_s(x_i) at the training points for all draws: one launch
//            per GROUP of rows with draws (as many as fit the workspace slots; option paths_mix_slots):
//              eval_chunk under FactorMode(h, true)    K(theta_r) of the group built and factored together, factors kept
//              paths_mix_resid_kernel                  y - m_r - f~ - sn_r eps into each slot's rows of the vector block, the
//                                                      counts padded to a common whole number of 128-row tiles
//              queue_forward_slots + queue_backward_rows(nslots)   both substitutions for all slots at once
//              paths_mix_gather_kernel                 the slots' rows into the object's [Npad][Spad] block
//            paths_mix_finite_kernel, paths_mix_poison_kernel      info per row; NaN into the draws of a failed row
//   eval / eval_own   per chunk of points: paths_mix_kernel over the features, then over the training points,
//            paths_mix_finish_kernel, one download.  eval is the shared-points form of the same kernel: the same bytes as
//            eval_own on the points broadcast to every draw.
// The forward substitution of a group always takes the batched GEMM route (queue_forward_slots with all_factored = false): the
// one-launch dataflow route needs every slot factored, and which route runs must not depend on whether SOME row failed -- the
// other rows' bytes do not change when a row fails.
#include "gp_paths_mix.h"

namespace {

constexpr int64_t PATHS_MIX_MAX_TAB = (int64_t)1 << 27;      // R x Ftot x d doubles: 1 GiB of per-row tables

// One contraction of the E pairs (pair e = s mc + t; shared: at point column e % mc of xt [d][ldt], else at column e) against
// the features (kernel = false) or the training points of the mixture object q, into part (grown here): ncomp = 1 or 1 + d
// components per pair and strip.  The strips follow from the pairs alone, as in queue_paths_own.
template <typename T>
int queue_paths_mix(gphip_paths* q, bool kernel, bool grad, bool shared, const double* xt, long ldt, int64_t E, int64_t mc, Buf& part,
                    int split, int* nstrips_out) {
    gphip_ctx* h = q->h;
    const int d = (int)q->d;
    PathsMixArgs<T> o{};
    o.a = paths_side<T>(q, kernel, xt, ldt, E);
    PathsArgs<T>& a = o.a;
    const long epad = (long)((E + PO_P - 1) / PO_P * PO_P);
    a.mpad = epad;
    a.ncomp = grad ? d + 1 : 1;
    o.mc = (int)mc;
    o.span = (int)std::min<int64_t>(q->S, (PO_P - 1) / mc + 2);
    o.shared = shared ? 1 : 0;
    o.row_of = q->dRowOf.as<int>();
    o.con_rs = kernel ? 0l : (long)q->d * (long)q->Ftot;
    o.ph_rs = kernel ? 0l : (long)q->Ftot;
    o.ie_rs = d; o.sp_rs = SLOTP;
    const bool global_form = d > KB_LDS_MAXD;
    const int dw = d <= 8 ? 8 : (d <= 16 ? 16 : 32);
    const size_t row_bytes = kernel ? (size_t)(2 * dw + SLOTP) * 8 : (size_t)(dw + 1) * PC_TJ * 8;
    int rows = global_form ? 0 : (int)std::min<size_t>((size_t)std::min(q->R, o.span), (size_t)PM_ROW_LDS / row_bytes);
    if (h->paths_mix_stage >= 0) rows = std::min(rows, h->paths_mix_stage);
    o.rows_lds = rows;
    const unsigned gx = (unsigned)(epad / PO_P);
    // the strip rule counts 256-thread workgroups: two of this kernel's count as one
    const int nstrips = paths_strips(h, ((long)gx + 1) / 2, a.ncon, split, &a.strip_slabs);
    *nstrips_out = nstrips;
    HIPCHK(part.grow((size_t)nstrips * a.ncomp * epad * 8));
    a.part = part.as<double>();
    const dim3 grid(gx, (unsigned)nstrips, (unsigned)(grad && global_form ? (d + PO_GW - 1) / PO_GW : 1));
    // profile class 6 (prediction epilogue): flops = the FMAs of the dot products; bytes = the weight slabs once per workgroup
    ProfScope ps(h, 6, 2.0 * a.ncomp * (double)E * a.ncon, (double)sizeof(T) * gx * a.ncon * o.span);
#define PATHS_MIX_GO(GEN, FEAT, GRAD, DW) \
    hipLaunchKernelGGL((paths_mix_kernel<T, GEN, GRAD, DW>), grid, dim3(PO_P), (paths_mix_lds<T, FEAT, DW>(o.span, o.rows_lds)), h->stream, o)
#define PATHS_MIX_DW(GEN, FEAT, GRAD)                                    \
    do {                                                                 \
        if (d <= 8) PATHS_MIX_GO(GEN, FEAT, GRAD, 8);                    \
        else if (d <= 16) PATHS_MIX_GO(GEN, FEAT, GRAD, 16);             \
        else if (!global_form) PATHS_MIX_GO(GEN, FEAT, GRAD, 32);        \
        else PATHS_MIX_GO(GEN, FEAT, GRAD, 0);                           \
    } while (0)
    if (kernel) { if (grad) PATHS_MIX_DW(GenKernel, false, true); else PATHS_MIX_DW(GenKernel, false, false); }
    else { if (grad) PATHS_MIX_DW(GenFeature, true, true); else PATHS_MIX_DW(GenFeature, true, false); }
#undef PATHS_MIX_DW
#undef PATHS_MIX_GO
    return GPHIP_OK;
}

// gphip_paths_eval (shared) and gphip_paths_eval_own on a mixture object: the chunks of paths_own_chunk_rows, per chunk both
// contractions, the finish kernel and one download
template <typename T>
int paths_mix_eval_device(gphip_paths* q, const double* X, int64_t M, bool shared, double* out, double* dout) {
    gphip_ctx* h = q->h;
    const int64_t d = q->d;
    const int S = q->S;
    HIPCHK(hipSetDevice(h->device));
    const int64_t MC = paths_own_chunk_rows(q, M);
    const int64_t EPAD = ((int64_t)S * MC + PO_P - 1) / PO_P * PO_P;
    HIPCHK(q->dXs.grow((size_t)d * (shared ? (MC + PC_TP - 1) / PC_TP * PC_TP : EPAD) * 8));
    HIPCHK(q->dOut.grow((size_t)S * MC * 8));
    if (dout) HIPCHK(q->dDout.grow((size_t)S * MC * d * 8));
    std::vector<double> xt, ho, hd;
    hipStream_t st = h->stream;
    const bool grad = dout != nullptr;
    for (int64_t m0 = 0; m0 < M; m0 += MC) {
        const int64_t mc = std::min<int64_t>(MC, M - m0), E = (int64_t)S * mc, epad = (E + PO_P - 1) / PO_P * PO_P;
        const int64_t ldt = shared ? (mc + PC_TP - 1) / PC_TP * PC_TP : epad;
        xt.assign((size_t)d * ldt, 0.0);
        if (shared) {
            for (int64_t i = 0; i < mc; ++i)
                for (int64_t c = 0; c < d; ++c) xt[(size_t)c * ldt + i] = X[(m0 + i) * d + c];
        } else {
            for (int64_t s = 0; s < S; ++s)
                for (int64_t i = 0; i < mc; ++i)
                    for (int64_t c = 0; c < d; ++c) xt[(size_t)c * ldt + s * mc + i] = X[((int64_t)s * M + m0 + i) * d + c];
        }
        HIPCHK(hipMemcpyAsync(q->dXs.p, xt.data(), xt.size() * 8, hipMemcpyHostToDevice, st));
        int nsf = 0, nsk = 0;
        if (int rc = queue_paths_mix<T>(q, false, grad, shared, q->dXs.as<double>(), (long)ldt, E, mc, q->dPartF, h->paths_split, &nsf)) return rc;
        if (int rc = queue_paths_mix<T>(q, true, grad, shared, q->dXs.as<double>(), (long)ldt, E, mc, q->dPartK, h->paths_split, &nsk)) return rc;
        if (shared) h->paths_nsplit = nsk;
        else h->paths_own_nsplit = nsk;
        const int ncomp = grad ? (int)d + 1 : 1;
        const long nf = (long)E * ncomp;
        hipLaunchKernelGGL(paths_mix_finish_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, (const double*)q->dPartF.p, nsf,
                           (const double*)q->dPartK.p, nsk, ncomp, (long)epad, (long)E, (long)mc, (const int*)q->dRowOf.as<int>(),
                           (const double*)q->dMu.as<double>(), q->dOut.as<double>(), grad ? q->dDout.as<double>() : nullptr);
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

int paths_mix_eval(gphip_paths* q, const double* X, int64_t M, bool shared, double* out, double* dout) {
    gphip_ctx* h = q->h;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = DISPATCH(h, paths_mix_eval_device, q, X, M, shared, out, dout);
    (shared ? h->paths_eval_us : h->paths_own_us) = paths_us(t0);
    return rc;
}

// the device part of gphip_paths_create_samples (h->mu held).  active: the rows with draws, ascending; start / counts: the rows'
// first draw and number of draws; info: filled for the active rows; bad[r] != 0 on return: row r failed.
template <typename T>
int paths_mix_create_device(gphip_paths* q, const double* Thetas, int p, const std::vector<int>& active, const std::vector<int>& start,
                            const int* counts, const uint64_t* seeds, int* info, std::vector<int>& bad) {
    gphip_ctx* h = q->h;
    const int64_t N = q->N, Npad = q->Npad, d = q->d, Ftot = q->Ftot, Spad = q->Spad;
    const int S = q->S, R = q->R, na = (int)active.size();
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(q->dXt.grow((size_t)d * Npad * 8));
    HIPCHK(q->dIe1.grow((size_t)R * d * 8));
    HIPCHK(q->dIe2.grow((size_t)R * d * 8));
    HIPCHK(q->dSlotp.grow((size_t)R * SLOTP * 8));
    HIPCHK(q->dMu.grow((size_t)R * 8));
    HIPCHK(q->dRowOf.grow((size_t)S * 4));
    HIPCHK(q->dOmT.grow((size_t)R * d * Ftot * 8));
    HIPCHK(q->dPhase.grow((size_t)R * Ftot * 8));
    HIPCHK(q->dWa.grow((size_t)Ftot * Spad * sizeof(T)));
    HIPCHK(q->dW.grow((size_t)S * Ftot * 8));
    HIPCHK(q->dEps.grow((size_t)S * N * 8));
    HIPCHK(q->dV.grow((size_t)Npad * Spad * sizeof(T)));
    // scratch of the call in dFlag: [R Ftot] a_r, [Npad] y, [R] sn, [R] eps keys, [R] seeds, then the ints start, count, rows
    // (the active rows), bad, flag, R each
    const size_t n8 = (size_t)R * Ftot + (size_t)Npad + 3 * (size_t)R;
    HIPCHK(q->dFlag.grow(n8 * 8 + 5 * (size_t)R * 4));
    double* dAmp = q->dFlag.as<double>();
    double* dY = dAmp + (size_t)R * Ftot;
    double* dSn = dY + Npad;
    uint64_t* dKeys = reinterpret_cast<uint64_t*>(dSn + R);
    uint64_t* dSeeds = dKeys + R;
    int* dStart = reinterpret_cast<int*>(dSeeds + R);
    int *dCount = dStart + R, *dRows = dCount + R, *dBad = dRows + R, *dRowFlag = dBad + R;
    // the host's share: inputs, the rows' tables (Omega transposed per row), noise scales and keys
    std::vector<double> xt((size_t)d * Npad, 0.0), y((size_t)Npad, 0.0), omt((size_t)R * d * Ftot, 0.0), sn((size_t)R, 0.0);
    std::vector<uint64_t> keys((size_t)R), sd(seeds, seeds + R);
    std::vector<int> rows_pad((size_t)R, 0);
    for (int64_t i = 0; i < N; ++i) {
        for (int64_t c = 0; c < d; ++c) xt[(size_t)c * Npad + i] = h->hostX[(size_t)i * d + c];
        y[(size_t)i] = h->hostY[(size_t)i];
    }
    q->omega.assign((size_t)R * Ftot * d, 0.0); q->phase.assign((size_t)R * Ftot, 0.0); q->amp.assign((size_t)R * Ftot, 0.0);
    for (int r = 0; r < R; ++r) {
        const double* th = Thetas + (size_t)r * p;
        double* om = q->omega.data() + (size_t)r * Ftot * d;
        int64_t ft = 0;
        // (a theta without a table, non-finite or a zero length scale, does not factor either: eval_chunk says so below)
        if (gphip_rff_table(h->kernel_id, h->d, th, p, q->F, seeds[r], &ft, om, q->phase.data() + (size_t)r * Ftot, q->amp.data() + (size_t)r * Ftot)) {
            std::fill(om, om + (size_t)Ftot * d, 0.0);
            std::fill(q->phase.begin() + (size_t)r * Ftot, q->phase.begin() + (size_t)(r + 1) * Ftot, 0.0);
            std::fill(q->amp.begin() + (size_t)r * Ftot, q->amp.begin() + (size_t)(r + 1) * Ftot, 0.0);
            if (counts[r] > 0) bad[(size_t)r] = 1;
        }
        for (int64_t j = 0; j < Ftot; ++j)
            for (int64_t c = 0; c < d; ++c) omt[((size_t)r * d + c) * Ftot + j] = om[(size_t)j * d + c];
        const double s = std::fabs(th[(size_t)p - 1 - (h->mean_id == GPHIP_MEAN_CONST ? 1 : 0)]);
        sn[(size_t)r] = std::isfinite(s) ? s : 0.0;
        keys[(size_t)r] = rff_key(seeds[r], RFF_TAG_EPS);
        // m_r: theta's last entry under the constant mean (what stage_theta puts into the slot scalar [2]), else 0
        const double m = h->mean_id == GPHIP_MEAN_CONST ? th[(size_t)p - 1] : 0.0;
        q->mu_r[(size_t)r] = std::isfinite(m) ? m : 0.0;
    }
    std::copy(active.begin(), active.end(), rows_pad.begin());
    hipStream_t st = h->stream;
    HIPCHK(hipMemcpyAsync(q->dXt.p, xt.data(), xt.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(q->dOmT.p, omt.data(), omt.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(q->dPhase.p, q->phase.data(), (size_t)R * Ftot * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(q->dRowOf.p, q->row_of.data(), (size_t)S * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dAmp, q->amp.data(), (size_t)R * Ftot * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dY, y.data(), (size_t)Npad * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dSn, sn.data(), (size_t)R * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(q->dMu.p, q->mu_r.data(), (size_t)R * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dKeys, keys.data(), (size_t)R * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dSeeds, sd.data(), (size_t)R * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dStart, start.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dCount, counts, (size_t)R * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dRows, rows_pad.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(dRowFlag, 0, (size_t)R * 4, st));
    HIPCHK(hipMemsetAsync(q->dWa.p, 0, (size_t)Ftot * Spad * sizeof(T), st));
    HIPCHK(hipMemsetAsync(q->dV.p, 0, (size_t)Npad * Spad * sizeof(T), st));
    const long nw = (long)S * Ftot;
    hipLaunchKernelGGL(paths_mix_weights_kernel<T>, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, q->dW.as<double>(), (T*)q->dWa.p,
                       (const double*)dAmp, (const int*)q->dRowOf.as<int>(), (const int*)dStart, (const uint64_t*)dSeeds, S, (long)Ftot,
                       (long)Spad);
    // f~ of every draw at the training points: the shared-points form, pair s N + i
    int nsf = 0;
    const int64_t EF = (int64_t)S * N, epadF = (EF + PO_P - 1) / PO_P * PO_P;
    if (int rc = queue_paths_mix<T>(q, false, false, true, q->dXt.as<double>(), (long)Npad, EF, N, q->dPartF, h->paths_split, &nsf)) return rc;
    HIPCHK(hipStreamSynchronize(st));                          // (the copies have read the host vectors)
    // groups of rows that fit the slots
    if (int rc = ensure_slots(h, na)) return rc;
    invalidate_fit(h);
    const int G = std::max(1, h->paths_mix_slots > 0 ? std::min(h->paths_mix_slots, h->slots) : h->slots);
    h->paths_mix_slots_last = std::min(G, na);
    h->paths_mix_groups = (na + G - 1) / G;
    std::vector<double> ie1((size_t)R * d, 1.0), ie2((size_t)R * d, 1.0), slotp((size_t)R * SLOTP, 0.0), tg, ll;
    std::vector<int> inf;
    for (int g0 = 0; g0 < na; g0 += G) {
        const int nb = std::min(G, na - g0);
        tg.resize((size_t)nb * p); ll.resize((size_t)nb); inf.assign((size_t)nb, 0);
        int cmax = 1;
        for (int k = 0; k < nb; ++k) {
            const int r = active[(size_t)(g0 + k)];
            memcpy(tg.data() + (size_t)k * p, Thetas + (size_t)r * p, (size_t)p * 8);
            cmax = std::max(cmax, counts[r]);
        }
        int rc;
        {
            FactorMode mode(h, true);          // the substitutions below use the 128-block inverses
            rc = eval_chunk(h, tg.data(), nb, ll.data(), nullptr, inf.data());      // build + factor, kept
        }
        if (rc) return rc;
        for (int k = 0; k < nb; ++k) {           // the slots' staged hyper-parameters, as the build kernels read them
            const int r = active[(size_t)(g0 + k)];
            memcpy(ie1.data() + (size_t)r * d, h->hInvEll.as<double>() + (size_t)k * d, (size_t)d * 8);
            if (q->two) memcpy(ie2.data() + (size_t)r * d, h->hInvEll2.as<double>() + (size_t)k * d, (size_t)d * 8);
            memcpy(slotp.data() + (size_t)r * SLOTP, h->hSlotp.as<double>() + (size_t)k * SLOTP, (size_t)SLOTP * 8);
            info[r] = inf[(size_t)k];
            if (inf[(size_t)k] != GPHIP_INFO_OK) bad[(size_t)r] = 1;
        }
        const int64_t mpad = ((int64_t)cmax + TB - 1) / TB * TB;
        if ((rc = ensure_vbuf(h, (int64_t)nb * mpad))) return rc;
        const long nv = (long)Npad * mpad, vs = nv;
        const dim3 grid((unsigned)((nv + 255) / 256), (unsigned)nb);
        hipLaunchKernelGGL(paths_mix_resid_kernel<T>, grid, dim3(256), 0, st, (const double*)q->dPartF.p, nsf, (long)epadF, (long)N, (long)Npad,
                           (const double*)dY, (const int*)(dRows + g0), (const int*)dStart, (const int*)dCount, (const double*)q->dMu.as<double>(),
                           (const double*)dSn, (const uint64_t*)dKeys, q->dEps.as<double>(), (T*)h->dV.p, (long)mpad, vs);
        queue_forward_slots(h, mpad, nb, false, false);
        if ((rc = queue_backward_rows<T>(h, mpad, nullptr, nullptr, nullptr, nb))) return rc;
        hipLaunchKernelGGL(paths_mix_gather_kernel<T>, grid, dim3(256), 0, st, (const T*)h->dV.p, (long)mpad, vs, (long)Npad,
                           (const int*)(dRows + g0), (const int*)dStart, (const int*)dCount, (T*)q->dV.p, (long)Spad);
        if ((rc = complete_call(h))) return rc;
    }
    // what the evaluations read per row, the rows' verdicts, NaN into the failed rows' draws
    HIPCHK(hipMemcpyAsync(q->dIe1.p, ie1.data(), ie1.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(q->dIe2.p, ie2.data(), ie2.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(q->dSlotp.p, slotp.data(), slotp.size() * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(paths_mix_finite_kernel<T>, dim3(1024), dim3(256), 0, st, (const T*)q->dV.p, (long)N, (long)Spad, S,
                       (const int*)q->dRowOf.as<int>(), dRowFlag);
    std::vector<int> flag((size_t)R, 0);
    HIPCHK(hipMemcpyAsync(flag.data(), dRowFlag, (size_t)R * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int r = 0; r < R; ++r)
        if (counts[r] > 0 && (flag[(size_t)r] || bad[(size_t)r])) {
            bad[(size_t)r] = 1;
            if (info[r] == GPHIP_INFO_OK) info[r] = GPHIP_INFO_NAN;
        }
    HIPCHK(hipMemcpyAsync(dBad, bad.data(), (size_t)R * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(paths_mix_poison_kernel<T>, dim3(1024), dim3(256), 0, st, (T*)q->dV.p, (long)N, (long)Spad, S,
                       (const int*)q->dRowOf.as<int>(), (const int*)dBad);
    if (int rc = complete_call(h)) return rc;
    q->dPartF.release();                                        // (S N-sized: an evaluation sizes its own)
    q->dFlag.release();
    return GPHIP_OK;
}

}  // namespace

extern "C" {

int gphip_paths_create_samples(gphip_handle h, const double* Thetas, int R, int p, const int* counts, const uint64_t* seeds, int F,
                               gphip_paths_handle* out, int* info) {
    if (out) *out = nullptr;
    if (!h || !Thetas || !counts || !seeds || !out || !info) return fail(h, GPHIP_ERR_ARG, "null argument");
    if (p != h->p) return fail(h, GPHIP_ERR_DIM, "theta has the wrong length");
    if (R < 1 || F < 1) return fail(h, GPHIP_ERR_DIM, "R < 1 or F < 1");
    int64_t S = 0;
    for (int r = 0; r < R; ++r) {
        if (counts[r] < 0) return fail(h, GPHIP_ERR_DIM, "a negative count");
        S += counts[r];
    }
    if (S < 1 || S > PATHS_MAX_S) return fail(h, GPHIP_ERR_DIM, "the counts add up to less than 1 or more than 2048 draws");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (h->custom) return fail(h, GPHIP_ERR_UNSUPPORTED, "no spectral law is known for a run-time compiled covariance function");
    if (h->pw_mean_host || h->pw_nug_host) return fail(h, GPHIP_ERR_UNSUPPORTED, "gphip_paths_create_samples with a point-dependent nugget / mean");
    const bool null_k = h->kernel_id == GPHIP_KERNEL_NULL;
    int64_t Ftot = 0;
    if (!null_k) {
        if (gphip_rff_table(h->kernel_id, h->d, nullptr, p, F, 0, &Ftot, nullptr, nullptr, nullptr))
            return fail(h, GPHIP_ERR_DIM, "no feature table for this kernel");
        if (Ftot * S > PATHS_MAX_FS) return fail(h, GPHIP_ERR_DIM, "Ftot x S above 2^26");
        if ((int64_t)R * Ftot * h->d > PATHS_MIX_MAX_TAB) return fail(h, GPHIP_ERR_DIM, "R x Ftot x d above 2^27");
        if (S * h->N > (int64_t)INT32_MAX - PO_P) return fail(h, GPHIP_ERR_DIM, "S x N above 2^31");
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < R; ++r) info[r] = GPHIP_INFO_OK;
    gphip_paths* q = new gphip_paths;
    q->h = h; q->S = (int)S; q->F = F; q->mix = true; q->R = R; q->Ftot = Ftot;
    q->N = h->N; q->Npad = h->Npad; q->d = h->d; q->Spad = (S + TB - 1) / TB * TB;
    q->row_of.resize((size_t)S); q->mu_r.assign((size_t)R, 0.0);
    std::vector<int> active, start((size_t)R, 0), bad((size_t)R, 0);
    {
        int s = 0;
        for (int r = 0; r < R; ++r) {
            start[(size_t)r] = s;
            if (counts[r] > 0) active.push_back(r);
            for (int k = 0; k < counts[r]; ++k) q->row_of[(size_t)s++] = r;
        }
    }
    if (null_k) {                                  // null kernel: f = m_r, answered on the host
        q->null_k = true;
        bool any = false;
        for (int r : active) {
            double mu = 0.0;
            info[r] = null_theta_info(h, Thetas + (size_t)r * p, &mu);
            q->mu_r[(size_t)r] = info[r] == GPHIP_INFO_OK ? mu : std::nan("");
            any = any || info[r] == GPHIP_INFO_OK;
        }
        if (!any) { delete q; return GPHIP_OK; }
        ++h->paths_live;
        *out = q;
        return GPHIP_OK;
    }
    q->ks = h->ks; q->two = h->ks.op != 0;
    const int rc = DISPATCH(h, paths_mix_create_device, q, Thetas, p, active, start, counts, seeds, info, bad);
    bool any = false;
    for (int r : active) any = any || !bad[(size_t)r];
    if (rc || !any) {
        (void)hipSetDevice(h->device);
        delete q;
        return rc;
    }
    ++h->paths_live;
    *out = q;
    h->paths_mix_create_us = paths_us(t0);
    return GPHIP_OK;
}

int gphip_paths_rows(gphip_paths_handle q, int* R, int* row_of_draw) {
    if (!q) return GPHIP_ERR_ARG;
    if (R) *R = q->R;
    if (row_of_draw)
        for (int s = 0; s < q->S; ++s) row_of_draw[s] = q->mix ? q->row_of[(size_t)s] : 0;
    return GPHIP_OK;
}

int gphip_paths_get_table(gphip_paths_handle q, int r, double* omega, double* phase, double* amp) {
    if (!q) return GPHIP_ERR_ARG;
    gphip_ctx* h = q->h;
    PathsLock lk(q);
    if (r < 0 || r >= q->R) return paths_ret(q, fail(h, GPHIP_ERR_DIM, "no such row"));
    if (q->null_k) return GPHIP_OK;                 // no features: nothing to copy (Ftot = 0)
    const size_t ft = (size_t)q->Ftot;
    if (omega) memcpy(omega, q->omega.data() + (size_t)r * ft * q->d, ft * q->d * 8);
    if (phase) memcpy(phase, q->phase.data() + (size_t)r * ft, ft * 8);
    if (amp) memcpy(amp, q->amp.data() + (size_t)r * ft, ft * 8);
    return GPHIP_OK;
}

}  // extern "C"
