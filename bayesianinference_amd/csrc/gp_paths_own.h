// gp_paths_own.h -- device side of gphip_paths_eval_own (include/gphip.h): every draw of a paths object at
// ITS OWN points.  Included by gphip_paths.inc behind gp_paths.h, whose generator policies (GenFeature / GenKernel) it uses as
// they are.  It sees only what a paths object holds (contraction points, tables, weights) and never the fit: the contraction
// points need not be the training points.
//
//   paths_own_kernel           part[e] = sum_j G(x_e, j) W(s(e), j) and, in the GRAD form, sum_j dG/dx_c W(s(e), j) for every c
//   paths_own_finish_kernel    the mean and the strips of both generators added in a fixed order
//
// paths_contract_kernel shares a generated tile G(t, j) among up to 128 draws through the MFMA.  Here a point belongs to one draw:
// there is nothing to share and the product is a dot product per pair -- the shape of predict_xgrad_kernel (gp_xgrad.h), and this
// kernel is its sibling.  A thread owns ONE (draw, point) pair: the pairs are flattened draw-major, e = s mc + t (mc points per
// draw in the chunk), and a workgroup takes PO_P consecutive pairs, so one point for each of 2048 draws fills the lanes as 2048
// points of one draw do.  The thread holds its point's coordinates, one fp64 value accumulator and the fp64 gradient accumulators
// in registers.  A workgroup spans at most span = min(S, (PO_P - 1) / mc + 2) consecutive draws; per slab of PC_TJ contraction
// indices it stages in LDS the slab's coordinates [DW][PC_TJ] and phases, and the weights W(s, j) of its draw range as
// Ws[j][span] (W[j ldw + s] has s contiguous: coalesced loads).  All lanes work on the same j at the same time: coordinate and
// phase reads are LDS broadcasts, a lane reads its own draw's weight from the slab row -- consecutive draws on consecutive banks,
// equal draws a broadcast.  The generator runs ONCE per pair and j and feeds the value and all gradient components.
// Coordinates, phases and kernel values are fp64 whatever T is, the weights are read as T, every accumulation is fp64 (there is
// no matrix pipe to feed).  No atomics, every sum in a fixed order: two calls return the same bytes.  The value is summed in the
// same order, by the same FMAs on the same generated value, in the GRAD and the value-only form.
// DW > 0: the pair's coordinates in registers, the slab's in LDS (d <= DW <= KB_LDS_MAXD), the gradient complete in one launch.
// DW = 0: coordinates from global memory; the GRAD form takes a window of PO_GW coordinates per blockIdx.z (the value from z = 0).
// Partials: part[((strip ncomp + comp) mpad + e], comp = 0 the value, 1 + c the gradient in coordinate c (ncomp = 1 or 1 + d).
// grid = (mpad / PO_P, strips, windows), PO_P threads.
#pragma once
#include "gp_paths.h"

namespace gphip {

constexpr int PO_P = 128;                      // pairs per workgroup
constexpr int PO_GW = 8;                       // coordinates per gradient window of the global-memory form

template <typename T>
struct PathsOwnArgs {
    PathsArgs<T> a;                            // xt: the pairs' coordinates [d][ldt], pair e at column e; ntest = the pairs; mpad = ldt
    int mc;                                    // points per draw: pair e belongs to draw e / mc
    int span;                                  // draws a workgroup can span: the row length of the weight slab
};

template <typename T, int DW> __host__ __device__ constexpr size_t paths_own_lds(int span) {
    constexpr int DS = DW > 0 ? DW : 1;
    return (size_t)(DS * PC_TJ + PC_TJ + 2 * DS) * 8 + (size_t)PC_TJ * span * sizeof(T);
}

template <typename T, class Gen, bool GRAD, int DW>
__global__ __launch_bounds__(PO_P) void paths_own_kernel(PathsOwnArgs<T> o) {
    constexpr int DS = DW > 0 ? DW : 1, NG = GRAD ? (DW > 0 ? DW : PO_GW) : 1;
    const PathsArgs<T>& a = o.a;
    extern __shared__ double lds_raw[];
    double* con_s = lds_raw;                     // [DS][PC_TJ] the slab's coordinates
    double* ph_s = con_s + DS * PC_TJ;           // [PC_TJ] its phases
    double* ie1_s = ph_s + PC_TJ;                // [DS] 1 / l, zero from d on
    double* ie2_s = ie1_s + DS;
    T* Ws = reinterpret_cast<T*>(ie2_s + DS);    // [PC_TJ][span] the slab's weights of the workgroup's draws
    const int tid = threadIdx.x, d = a.d, span = o.span;
    const long e0 = (long)blockIdx.x * PO_P, e = e0 + tid;               // < ldt: the grid covers the padded pairs
    const bool live = e < a.ntest;
    const long elast = e0 + PO_P <= a.ntest ? e0 + PO_P - 1 : (long)a.ntest - 1;
    const int s_lo = (int)(e0 / o.mc), ns = (int)(elast / o.mc) - s_lo + 1;       // the workgroup's draws (uniform), ns <= span
    const int sl = live ? (int)(e / o.mc) - s_lo : 0;
    const int c0 = (GRAD && DW == 0) ? (int)blockIdx.z * PO_GW : 0;
    double xr[DS], xw[NG];
#pragma unroll
    for (int q = 0; q < DS; ++q) xr[q] = (DW > 0 && live && q < d) ? a.xt[(long)q * a.ldt + e] : 0.0;
#pragma unroll
    for (int w = 0; w < NG; ++w) xw[w] = (GRAD && DW == 0 && live && c0 + w < d) ? a.xt[(long)(c0 + w) * a.ldt + e] : 0.0;
    if (DW > 0 && tid < DW) {
        ie1_s[tid] = (a.ie1 && tid < d) ? a.ie1[tid] : 0.0;
        ie2_s[tid] = (a.ie2 && tid < d) ? a.ie2[tid] : 0.0;
    }
    double acc = 0.0, ag[NG];
#pragma unroll
    for (int w = 0; w < NG; ++w) ag[w] = 0.0;
    const long jbeg = (long)blockIdx.y * a.strip_slabs * PC_TJ;
    const long jend = jbeg + (long)a.strip_slabs * PC_TJ < a.ncon ? jbeg + (long)a.strip_slabs * PC_TJ : a.ncon;
    for (long js = jbeg; js < jend; js += PC_TJ) {
        __syncthreads();                         // (the previous slab has been read)
        for (int idx = tid; idx < PC_TJ * ns; idx += PO_P) {
            const int jl = idx / ns, k = idx % ns;
            Ws[jl * span + k] = js + jl < jend ? a.W[(js + jl) * a.ldw + s_lo + k] : (T)0;
        }
        if (tid < PC_TJ) ph_s[tid] = (a.phase && js + tid < jend) ? a.phase[js + tid] : 0.0;
        if (DW > 0)
            for (int idx = tid; idx < DW * PC_TJ; idx += PO_P) {
                const int c = idx / PC_TJ, jl = idx % PC_TJ;
                con_s[idx] = (c < d && js + jl < jend) ? a.con[(long)c * a.ldc + js + jl] : 0.0;
            }
        __syncthreads();
        const int nj = (int)(jend - js < PC_TJ ? jend - js : PC_TJ);
        if (!live) continue;
        for (int jl = 0; jl < nj; ++jl) {
            const long j = js + jl;
            Gen g(a);
            g.begin(ph_s[jl]);
            if (DW > 0) {
#pragma unroll
                for (int q = 0; q < DS; ++q) g.coord(xr[q], con_s[q * PC_TJ + jl], ie1_s[q], ie2_s[q]);
            } else {
                for (int c = 0; c < d; ++c)
                    g.coord(a.xt[(long)c * a.ldt + e], a.con[(long)c * a.ldc + j], a.ie1 ? a.ie1[c] : 0.0, a.ie2 ? a.ie2[c] : 0.0);
            }
            const double val = g.template finish<GRAD>();
            const double wt = (double)Ws[jl * span + sl];
            acc = __builtin_fma(wt, val, acc);
            if constexpr (GRAD) {
                if constexpr (DW > 0) {          // (coordinates from d on: the slab holds zeros there and so does xr, the term is zero)
#pragma unroll
                    for (int q = 0; q < DW; ++q) ag[q] = __builtin_fma(wt, g.dcoord(xr[q], con_s[q * PC_TJ + jl], ie1_s[q], ie2_s[q]), ag[q]);
                } else {
#pragma unroll
                    for (int w = 0; w < NG; ++w) {
                        const int c = c0 + w;
                        if (c < d)
                            ag[w] = __builtin_fma(wt, g.dcoord(xw[w], a.con[(long)c * a.ldc + j], a.ie1 ? a.ie1[c] : 0.0, a.ie2 ? a.ie2[c] : 0.0), ag[w]);
                    }
                }
            }
        }
    }
    if (!live) return;
    double* p = a.part + (long)blockIdx.y * a.ncomp * a.mpad + e;
    if (!GRAD || DW > 0 || blockIdx.z == 0) p[0] = acc;
    if (GRAD) {
#pragma unroll
        for (int w = 0; w < NG; ++w)
            if (c0 + w < d) p[(long)(1 + c0 + w) * a.mpad] = ag[w];
    }
}

// out[e] = mu + (feature strips in order) + (kernel strips in order) for comp = 0, dout[e][c] = the same sums without mu for
// comp = 1 + c; E pairs, one thread per (pair, comp).  dout may be null when ncomp = 1.
__global__ __launch_bounds__(256) void paths_own_finish_kernel(const double* __restrict__ pf, int nsf, const double* __restrict__ pk, int nsk,
                                                               int ncomp, long mpad, long E, double mu, double* __restrict__ out,
                                                               double* __restrict__ dout) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= E * ncomp) return;
    const int comp = (int)(idx % ncomp);
    const long e = idx / ncomp;
    double f = 0.0, k = 0.0;
    for (int q = 0; q < nsf; ++q) f += pf[((long)q * ncomp + comp) * mpad + e];
    for (int q = 0; q < nsk; ++q) k += pk[((long)q * ncomp + comp) * mpad + e];
    if (comp == 0) out[e] = mu + f + k;
    else dout[e * (ncomp - 1) + comp - 1] = f + k;
}

}  // namespace gphip
