// gphip_gradbatch.inc -- the likelihood gradient for a batch of theta (include/gphip.h: gphip_loglik_grad_batch; DESIGN.md §8l).
// Included at the end of gphip.hip.
//
// One gradient is a chain of latency-bound launches (factor, U = L^-T, alpha, K^-1 = U U^T, reduction, finish).  Here the rows
// are evaluated in GROUPS, one theta per workspace slot as gphip_predict_samples does, and every link of the chain is ONE
// launch (or one chain of launches) for the whole group:
//   eval_batch_local under FactorMode       the G factors with their 128-block inverses
//   identity_rows_kernel + queue_forward_rows   U_s = L_s^-T for all slots, G slabs of Npad x Npad in dV (the multi-kernel route of
//                                           "grad_potri" = 2, which carries the slot count; the dataflow inverse launch does not)
//   gather_rhs_row / utri_gemv_partial / utri_gemv_finish   alpha_s = U_s z_s, slot = blockIdx.z
//   launch_gemm, nslots = G                 the lower tiles of K_s^-1 = U_s U_s^T into the slabs of dKinvB
//   launch_grad, G slots                    grad_reduce_*_slots_kernel (slot = blockIdx.z), grad_finish_kernel per slot
//   one download of the accumulators and the alphas, grad_from_acc per row on the host
// Nothing in the chain waits on another workgroup and no sum uses atomics: a slot whose K did not factor computes garbage in
// its own slabs, which nobody reads, and every row's bytes depend on its theta and on the size of its group only.
//
// Group rule (gradbatch_group): G = as many rows as the context gives workspace slots, as keep what is still missing of the
// 2 (Npad + GRAD_LD_PAD) Npad es bytes of scratch per slot within a quarter of the free device memory (the rule of
// claim_inverse_scratch), and as "grad_batch_slots" allows.  Fewer than two, "grad_potri" = 0, a point-dependent nugget / mean
// or a run-time compiled function without a gradient program: the rows go one by one through gphip_loglik_grad.  So do the rows
// of a handle with more than "grad_batch_max_n" training points (default 7168): there one theta fills the device, the one-theta
// call has the faster single-launch U, and the batch measured 2 % behind the loop at (N, B) = (8192, 4) (DESIGN.md section 8l).

namespace {

// rows per group for a call with B rows; 0: the per-row loop.  Leaves the slots, dV and dKinvB allocated for that many.
int gradbatch_group(gphip_ctx* h, int B, int* G) {
    *G = 0;
    const int limit = h->grad_batch_slots > 0 ? std::min(h->grad_batch_slots, h->max_slots) : h->max_slots;
    if (limit < 2 || h->grad_potri == 0 || (h->grad_batch_max_n > 0 && h->N > h->grad_batch_max_n)) return GPHIP_OK;
    int rc = ensure_slots(h, std::min(B, limit));
    if (rc) return rc;
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    const size_t row = (size_t)h->Npad * h->es, slab = (size_t)h->Npad * row;
    int g = std::min(std::min(B, limit), h->slots);
    for (; g >= 1; --g) {
        const size_t vrows = (size_t)g * h->Npad + GRAD_LD_PAD;
        const size_t missing = (vrows > (size_t)h->vcap ? (vrows - (size_t)h->vcap) * row : 0) +
                               ((size_t)g * slab > h->dKinvB.bytes ? (size_t)g * slab - h->dKinvB.bytes : 0);
        if (missing == 0 || missing <= fr / 4) break;
    }
    if (g < 1 || (g < 2 && B > 1)) return GPHIP_OK;
    if (ensure_vbuf(h, (int64_t)g * h->Npad + GRAD_LD_PAD) != GPHIP_OK || h->dKinvB.grow((size_t)g * slab) != hipSuccess ||
        h->dAlpha.grow((size_t)g * row) != hipSuccess) {
        (void)hipGetLastError();
        h->err.clear();
        return GPHIP_OK;
    }
    if ((rc = ensure_gacc(h))) return rc;
    HIPCHK(h->dGacc.grow((size_t)g * h->ngacc * 8));
    *G = g;
    return GPHIP_OK;
}

// behind the factorisation of G slots: everything up to the accumulators (dGacc: [G][ngacc]) and the alphas (dAlpha: [G][Npad])
template <typename T>
int gradbatch_queue(gphip_ctx* h, int G) {
    const long npad = h->Npad, slab = npad * npad;
    const int nt = (int)h->Nt, chunk = 128, nch = (int)((npad + chunk - 1) / chunk);
    const unsigned g = (unsigned)G, gv = (unsigned)((npad + 255) / 256);
    T *U = (T*)h->dV.p, *Kb = (T*)h->dKinvB.p;
    int gx = (int)((slab + 255) / 256);
    if (gx > 4096) gx = 4096;
    hipLaunchKernelGGL(identity_rows_kernel<T>, dim3((unsigned)gx, g), dim3(256), 0, h->stream, U, npad, (int)npad, 0, (int)h->N, slab);
    queue_forward_rows<T>(h, npad, G, 0, true);
    // alpha_s = U_s z_s; scratch: the head of slot s's K^-1 slab (z, then the per-chunk partial sums), as queue_alpha_from_u
    const long part_off = (long)((((size_t)npad * sizeof(T) + 255) / 256) * 256), part_bs = slab * (long)sizeof(T) / 8;
    double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(Kb) + part_off);
    hipLaunchKernelGGL(gather_rhs_row_kernel<T>, dim3(gv, 1, g), dim3(256), 0, h->stream, (const T*)h->dA.p, (int)h->R, 0, (int)npad, Kb, 1l,
                       0, (long)h->slot_elems, slab);
    hipLaunchKernelGGL(utri_gemv_partial_kernel<T>, dim3((unsigned)nt, (unsigned)nch, g), dim3(TB), 0, h->stream, (const T*)U, npad,
                       (const T*)Kb, (int)npad, chunk, part, slab, slab, part_bs);
    hipLaunchKernelGGL(utri_gemv_finish_kernel<T>, dim3(gv, 1, g), dim3(256), 0, h->stream, (const double*)part, nch, (int)npad,
                       (T*)h->dAlpha.p, part_bs, npad);
    HIPCHK(hipMemsetAsync(h->dGacc.p, 0, (size_t)G * h->ngacc * 8, h->stream));
    // the lower tiles of K_s^-1 = U_s U_s^T: one triangular launch, tile (i, j) contracts k >= 128 i only (queue_kinv), slot = grid.y
    launch_gemm<T>(h, 2, cm<T>(Kb, npad, slab), cm<T>(U, npad, slab), cm<T>(U, npad, slab), (int)npad, 0, nt, 0, nt, 1, G, 1, 1);
    GradArgs<T> a = grad_args<T>(h, Kb, npad, 0, h->N);
    a.tri = 1;
    GradStride st{slab, npad, (long)h->d * npad, (long)SLOTP, (long)h->ngacc, 0l};
    launch_grad<T>(h, a, dim3((unsigned)nt, (unsigned)nt), G, &st);
    return GPHIP_OK;
}

// one group: rows [0, G) of Theta through the chain above
int gradbatch_rows(gphip_ctx* h, const double* Theta, int G, int p, double* out, double* grad, int* info) {
    int rc = GPHIP_OK;
    {
        FactorMode mode(h, true);              // the substitutions below use the 128-block inverses
        rc = eval_batch_local(h, Theta, G, p, out, nullptr, info);
    }
    if (rc) return rc;
    bool any = false;
    for (int s = 0; s < G; ++s) {
        for (int i = 0; i < p; ++i) grad[(size_t)s * p + i] = std::nan("");
        any = any || info[s] == 0;
    }
    if (!any) return GPHIP_OK;
    if ((rc = DISPATCH(h, gradbatch_queue, h, G))) return rc;
    const size_t np = h->ngacc, N = (size_t)h->N, Npad = (size_t)h->Npad;
    std::vector<double> gacc((size_t)G * np), alpha;
    HIPCHK(hipMemcpyAsync(gacc.data(), h->dGacc.p, gacc.size() * 8, hipMemcpyDeviceToHost, h->stream));
    rc = complete_call(h, [&] { return DISPATCH(h, download, h, alpha, h->dAlpha.p, (size_t)G * Npad, h->stream); });
    if (rc) return rc;
    for (int s = 0; s < G; ++s) {
        if (info[s] != 0) continue;
        const std::vector<double> gs(gacc.begin() + (size_t)s * np, gacc.begin() + (size_t)(s + 1) * np);
        const std::vector<double> as(alpha.begin() + (size_t)s * Npad, alpha.begin() + (size_t)s * Npad + N);
        grad_from_acc(h, Theta + (size_t)s * p, gs, as, grad + (size_t)s * p);
    }
    return GPHIP_OK;
}

}  // namespace

extern "C" {

int gphip_loglik_grad_batch(gphip_handle h, const double* Theta, int B, int p, double* out, double* grad, int* info) {
    if (!h || !Theta || !out || !grad || !info) return fail(h, GPHIP_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(h->mu);
    if (p != h->p) return fail(h, GPHIP_ERR_DIM, "theta has the wrong length for this kernel/mean");
    if (B <= 0) return GPHIP_OK;
    HIPCHK(hipSetDevice(h->device));
    if (h->kernel_id == GPHIP_KERNEL_NULL) return null_kernel_batch(h, Theta, B, out, nullptr, info, grad);
    h->grad_batch_route = 0;
    h->grad_batch_last = 0;
    int G = 0, rc = GPHIP_OK;
    if (h->custom && (rc = ensure_custom_grad(h))) return rc;
    const bool loop = h->pw_mean_host || h->pw_nug_host || (h->custom && !(h->custom_grad && h->cgrad_state == 1));
    if (!loop && (rc = gradbatch_group(h, B, &G))) return rc;
    if (G == 0) {                              // the rows one by one through the one-theta call: bit-identical to the host's loop
        for (int s = 0; s < B; ++s)
            if ((rc = gphip_loglik_grad(h, Theta + (size_t)s * p, p, out + s, grad + (size_t)s * p, info + s))) return rc;
        invalidate_fit(h);                     // (no row's factor stays resident, as on the batched route)
        return GPHIP_OK;
    }
    h->grad_analytic = 0;
    h->grad_batch_route = 1;
    for (int s0 = 0; s0 < B; s0 += G) {
        const int nb = std::min(G, B - s0);
        if ((rc = gradbatch_rows(h, Theta + (size_t)s0 * p, nb, p, out + s0, grad + (size_t)s0 * p, info + s0))) return rc;
        h->grad_batch_last = nb;
    }
    return GPHIP_OK;
}

}  // extern "C"
