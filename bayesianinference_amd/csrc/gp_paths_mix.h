// gp_paths_mix.h -- device side of the mixture paths object (include/gphip.h: gphip_paths_create_samples):
// a paths object whose S draws each belong to one of R hyper-parameter rows.  Included by gphip_paths_mix.inc behind gp_paths.h
// and gp_paths_own.h, whose generator policies (GenFeature / GenKernel) and constants it uses as they are.  Out of scope: the
// sparse object (the contraction points are addressed per row through con_rs, so a per-row Z can come later), run-time compiled
// covariance functions, point-dependent fits, dealing rows to several devices.
//
//   paths_mix_kernel           part[e] = sum_j G_r(x_e, j) W(s(e), j), r = row_of[s(e)], and in the GRAD form the d derivatives
//   paths_mix_finish_kernel    m_r and the strips of both generators added in a fixed order
//   paths_mix_weights_kernel   w_sj = philox_normal(seed_r, q, j), Wa = a_rj w_sj            (q = the draw's number within its row)
//   paths_mix_resid_kernel     y - m_r - f~ - sn_r eps into each slot's rows of the vector block of the substitutions
//   paths_mix_gather_kernel    the slots' rows into the object's [Npad][Spad] block
//   paths_mix_finite_kernel / paths_mix_poison_kernel   a per-row finiteness flag; NaN into the draws of a failed row
//
// paths_mix_kernel is a sibling of paths_own_kernel (gp_paths_own.h), not a change to it: a thread owns ONE (draw, point) pair,
// pairs are flattened draw-major (e = s mc + t), a workgroup takes PO_P consecutive pairs, every sum is fp64 and runs in the order
// of the contraction index, strips leave partials that the finish kernel adds in a fixed order (no atomics: two calls return the
// same bytes, and the value is summed by the same FMAs in the GRAD and the value-only form).  What is new: everything that
// depends on theta is PER ROW -- Omega_r and b_r on the feature side (GenFeature); 1 / l_r of both terms and the slot scalars on
// the kernel side (GenKernel); m_r in the finish kernel.  The generators see their row through a row-adjusted copy of the
// arguments.  Draws are ordered by row, so a workgroup's draws cover the contiguous rows r_lo .. r_hi.
// shared = 1 (the shared-points form): pair e reads point column e % mc of xt -- all draws at the same mc points
// (gphip_paths_eval, the feature pass of the creation at the training points) without uploading the points S times.
//
// Staging rule.  Per slab of PC_TJ contraction indices a workgroup stages in LDS the weights of its draws (as paths_own_kernel)
// and, on the kernel side, the slab of training points, which all rows share.  What depends on the row is staged in LDS while
// the workgroup's rows fit: nrows = r_hi - r_lo + 1 <= rows_lds, where the host sets rows_lds = PM_ROW_LDS (16 KiB) / the bytes
// of one row: (DW + 1) PC_TJ doubles per slab on the feature side (Omega_r's slab and b_r's: 7 / 3 / 1 rows at DW = 8 / 16 / 32),
// 2 DW + SLOTP doubles once on the kernel side (64 / 42 / 25 rows).  A workgroup that spans more rows (one point per draw and
// one draw per row is 128 rows) reads its row's data from global memory through L1 / L2 instead: lanes of the same row read the
// same address.  The decision is uniform in the workgroup; both forms run the same arithmetic on the same numbers: the same bytes.
// With 32 KiB of weights at most (span = 128 fp64) and 8.25 KiB of shared slab the launch stays under 64 KiB of LDS.
// DW > 0: the pair's coordinates in registers (d <= DW <= KB_LDS_MAXD), the gradient complete in one launch.  DW = 0: nothing
// row-dependent is staged, coordinates come from global memory, the GRAD form takes a window of PO_GW coordinates per blockIdx.z.
// Partials: part[(strip ncomp + comp) mpad + e], comp = 0 the value, 1 + c the gradient in coordinate c.
// grid = (mpad / PO_P, strips, windows), PO_P threads.
#pragma once
#include <type_traits>
#include "gp_paths_own.h"

namespace gphip {

constexpr int PM_ROW_LDS = 16 * 1024;          // bytes of LDS for what a workgroup stages per row

template <typename T>
struct PathsMixArgs {
    PathsArgs<T> a;                            // row 0's view: xt [d][ldt]; ntest = the pairs; mpad = the pairs padded to PO_P
    int mc;                                    // points per draw: pair e belongs to draw e / mc
    int span;                                  // draws a workgroup can span: the row length of the weight slab
    int shared;                                // 1: pair e reads point column e % mc; 0: column e
    const int* row_of;                         // [S] the row of a draw, non-decreasing
    long con_rs, ph_rs;                        // elements between the rows' contraction points / phases (0: all rows share them)
    int ie_rs, sp_rs;                          // elements between the rows' 1 / l and slot scalars
    int rows_lds;                              // rows a workgroup stages in LDS (0: none)
};

template <bool FEAT, int DW> __host__ __device__ constexpr size_t paths_mix_row_bytes() {
    return FEAT ? (size_t)(DW + 1) * PC_TJ * 8 : (size_t)(2 * DW + SLOTP) * 8;
}

template <typename T, bool FEAT, int DW> __host__ __device__ constexpr size_t paths_mix_lds(int span, int rows_lds) {
    constexpr int DS = DW > 0 ? DW : 1;
    return (FEAT ? 0 : (size_t)DS * PC_TJ * 8) + (DW > 0 ? (size_t)rows_lds * paths_mix_row_bytes<FEAT, DS>() : 0) +
           (size_t)PC_TJ * span * sizeof(T);
}

template <typename T, class Gen, bool GRAD, int DW>
__global__ __launch_bounds__(PO_P) void paths_mix_kernel(PathsMixArgs<T> o) {
    constexpr bool FEAT = std::is_same<Gen, GenFeature>::value;
    constexpr int DS = DW > 0 ? DW : 1, NG = GRAD ? (DW > 0 ? DW : PO_GW) : 1;
    const PathsArgs<T>& a = o.a;
    const int RL = DW > 0 ? o.rows_lds : 0;
    extern __shared__ double lds_raw[];
    // feature side: [RL][DS][PC_TJ] Omega_r's slab, [RL][PC_TJ] b_r's; kernel side: [DS][PC_TJ] the training points' slab, then
    // [RL][DS] 1 / l of both terms (zero from d on) and [RL][SLOTP] the slot scalars
    double* con_s = lds_raw;
    double* ph_s = con_s + (FEAT ? RL : 1) * DS * PC_TJ;
    double* ie1_s = ph_s + (FEAT ? RL * PC_TJ : 0);
    double* ie2_s = ie1_s + (FEAT ? 0 : RL * DS);
    double* sp_s = ie2_s + (FEAT ? 0 : RL * DS);
    T* Ws = reinterpret_cast<T*>(sp_s + (FEAT ? 0 : RL * SLOTP));      // [PC_TJ][span] the slab's weights of the workgroup's draws
    const int tid = threadIdx.x, d = a.d, span = o.span;
    const long e0 = (long)blockIdx.x * PO_P, e = e0 + tid;               // < mpad: the grid covers the padded pairs
    const bool live = e < a.ntest;
    const long elast = e0 + PO_P <= a.ntest ? e0 + PO_P - 1 : (long)a.ntest - 1;
    const int s_lo = (int)(e0 / o.mc), ns = (int)(elast / o.mc) - s_lo + 1;       // the workgroup's draws (uniform), ns <= span
    const int sl = live ? (int)(e / o.mc) - s_lo : 0;
    const int r_lo = o.row_of[s_lo], nrows = o.row_of[s_lo + ns - 1] - r_lo + 1;  // its rows (uniform)
    const int r = o.row_of[s_lo + sl], rl = r - r_lo;
    const bool stg = DW > 0 && nrows <= RL;                                        // the staging rule (uniform)
    const long col = live ? (o.shared ? e % o.mc : e) : 0;
    const int c0 = (GRAD && DW == 0) ? (int)blockIdx.z * PO_GW : 0;
    // this pair's row in global memory
    const double* gcon = a.con + (long)r * o.con_rs;
    const double* gph = a.phase ? a.phase + (long)r * o.ph_rs : nullptr;
    const double* gie1 = a.ie1 ? a.ie1 + (long)r * o.ie_rs : nullptr;
    const double* gie2 = a.ie2 ? a.ie2 + (long)r * o.ie_rs : nullptr;
    double xr[DS], xw[NG];
#pragma unroll
    for (int q = 0; q < DS; ++q) xr[q] = (DW > 0 && live && q < d) ? a.xt[(long)q * a.ldt + col] : 0.0;
#pragma unroll
    for (int w = 0; w < NG; ++w) xw[w] = (GRAD && DW == 0 && live && c0 + w < d) ? a.xt[(long)(c0 + w) * a.ldt + col] : 0.0;
    if (!FEAT && stg) {
        for (int idx = tid; idx < nrows * DS; idx += PO_P) {
            const int rr = idx / DS, c = idx % DS;
            ie1_s[idx] = (a.ie1 && c < d) ? a.ie1[(long)(r_lo + rr) * o.ie_rs + c] : 0.0;
            ie2_s[idx] = (a.ie2 && c < d) ? a.ie2[(long)(r_lo + rr) * o.ie_rs + c] : 0.0;
        }
        for (int idx = tid; idx < nrows * SLOTP; idx += PO_P) sp_s[idx] = a.slotp[(long)(r_lo + idx / SLOTP) * o.sp_rs + idx % SLOTP];
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
        if (FEAT && stg) {
            for (int idx = tid; idx < nrows * DS * PC_TJ; idx += PO_P) {
                const int rr = idx / (DS * PC_TJ), c = (idx / PC_TJ) % DS, jl = idx % PC_TJ;
                con_s[idx] = (c < d && js + jl < jend) ? a.con[(long)(r_lo + rr) * o.con_rs + (long)c * a.ldc + js + jl] : 0.0;
            }
            for (int idx = tid; idx < nrows * PC_TJ; idx += PO_P) {
                const int rr = idx / PC_TJ, jl = idx % PC_TJ;
                ph_s[idx] = js + jl < jend ? a.phase[(long)(r_lo + rr) * o.ph_rs + js + jl] : 0.0;
            }
        }
        if (!FEAT && DW > 0)
            for (int idx = tid; idx < DW * PC_TJ; idx += PO_P) {
                const int c = idx / PC_TJ, jl = idx % PC_TJ;
                con_s[idx] = (c < d && js + jl < jend) ? a.con[(long)c * a.ldc + js + jl] : 0.0;
            }
        __syncthreads();
        const int nj = (int)(jend - js < PC_TJ ? jend - js : PC_TJ);
        if (!live) continue;
        // one slab for this pair; STG (a compile-time copy of stg): the row's data from LDS, else from global memory
        auto slab = [&](auto stg_c) {
            constexpr bool STG = decltype(stg_c)::value;
            PathsArgs<T> ar = a;                 // the generator's view of this pair's row
            if (!FEAT) ar.slotp = STG ? sp_s + rl * SLOTP : a.slotp + (long)r * o.sp_rs;
            auto con_at = [&](int q, int jl, long j) -> double {
                if (!FEAT) return con_s[q * PC_TJ + jl];
                if (STG) return con_s[(rl * DS + q) * PC_TJ + jl];
                return q < d ? gcon[(long)q * a.ldc + j] : 0.0;
            };
            auto ie1_at = [&](int q) -> double { return FEAT ? 0.0 : (STG ? ie1_s[rl * DS + q] : ((gie1 && q < d) ? gie1[q] : 0.0)); };
            auto ie2_at = [&](int q) -> double { return FEAT ? 0.0 : (STG ? ie2_s[rl * DS + q] : ((gie2 && q < d) ? gie2[q] : 0.0)); };
            for (int jl = 0; jl < nj; ++jl) {
                const long j = js + jl;
                Gen g(ar);
                g.begin(FEAT ? (STG ? ph_s[rl * PC_TJ + jl] : gph[j]) : 0.0);
                if constexpr (DW > 0) {
#pragma unroll
                    for (int q = 0; q < DS; ++q) g.coord(xr[q], con_at(q, jl, j), ie1_at(q), ie2_at(q));
                } else {
                    for (int c = 0; c < d; ++c)
                        g.coord(a.xt[(long)c * a.ldt + col], gcon[(long)c * a.ldc + j], gie1 ? gie1[c] : 0.0, gie2 ? gie2[c] : 0.0);
                }
                const double val = g.template finish<GRAD>();
                const double wt = (double)Ws[jl * span + sl];
                acc = __builtin_fma(wt, val, acc);
                if constexpr (GRAD) {
                    if constexpr (DW > 0) {      // (coordinates from d on: the contraction side reads zero there and so does xr, the term is zero)
#pragma unroll
                        for (int q = 0; q < DW; ++q) ag[q] = __builtin_fma(wt, g.dcoord(xr[q], con_at(q, jl, j), ie1_at(q), ie2_at(q)), ag[q]);
                    } else {
#pragma unroll
                        for (int w = 0; w < NG; ++w) {
                            const int c = c0 + w;
                            if (c < d)
                                ag[w] = __builtin_fma(wt, g.dcoord(xw[w], gcon[(long)c * a.ldc + j], gie1 ? gie1[c] : 0.0, gie2 ? gie2[c] : 0.0), ag[w]);
                        }
                    }
                }
            }
        };
        if (stg) slab(std::true_type{});
        else slab(std::false_type{});
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

// out[e] = m_r + (feature strips in order) + (kernel strips in order) for comp = 0, dout[e][c] = the same sums without m_r for
// comp = 1 + c; E pairs of mc points per draw, r = row_of[e / mc]; one thread per (pair, comp).  dout may be null when ncomp = 1.
__global__ __launch_bounds__(256) void paths_mix_finish_kernel(const double* __restrict__ pf, int nsf, const double* __restrict__ pk, int nsk,
                                                               int ncomp, long mpad, long E, long mc, const int* __restrict__ row_of,
                                                               const double* __restrict__ mu, double* __restrict__ out,
                                                               double* __restrict__ dout) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= E * ncomp) return;
    const int comp = (int)(idx % ncomp);
    const long e = idx / ncomp;
    double f = 0.0, k = 0.0;
    for (int q = 0; q < nsf; ++q) f += pf[((long)q * ncomp + comp) * mpad + e];
    for (int q = 0; q < nsk; ++q) k += pk[((long)q * ncomp + comp) * mpad + e];
    if (comp == 0) out[e] = mu[row_of[e / mc]] + f + k;
    else dout[e * (ncomp - 1) + comp - 1] = f + k;
}

// w[s][j] = philox_normal(seeds[r], s - start[r], j) (fp64, kept) and Wa(s, j) = amp[r][j] w_sj at Wa[j ldw + s], r = row_of[s]:
// draw number s - start[r] of row r has the weights of that draw of gphip_paths_create(.., seeds[r])
template <typename T>
__global__ __launch_bounds__(256) void paths_mix_weights_kernel(double* __restrict__ w, T* __restrict__ Wa, const double* __restrict__ amp,
                                                                const int* __restrict__ row_of, const int* __restrict__ start,
                                                                const uint64_t* __restrict__ seeds, int S, long Ftot, long ldw) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)S * Ftot) return;
    const int s = (int)(e / Ftot);
    const long j = e % Ftot;
    const int r = row_of[s];
    const double z = philox_normal(seeds[r], (uint32_t)(s - start[r]), (uint32_t)j);
    w[e] = z;
    Wa[j * ldw + s] = (T)(amp[(long)r * Ftot + j] * z);
}

// The right-hand sides of a group of rows in the vector block of the substitutions, slot = blockIdx.y, row r = rows[slot]:
// V(t, i) = (y_i - m_r) - f~_s(x_i) - eps_si at V[slot vs + i mpad + t] for the row's draws t < count[r] (s = start[r] + t), zero
// for the padding; f~ = the feature pass's strips (pair s N + i) added in order, eps_si = sn_r philox_normal(keys[r], t, i) (kept).
template <typename T>
__global__ __launch_bounds__(256) void paths_mix_resid_kernel(const double* __restrict__ part, int nstrips, long epad, long N, long Npad,
                                                              const double* __restrict__ y, const int* __restrict__ rows,
                                                              const int* __restrict__ start, const int* __restrict__ count,
                                                              const double* __restrict__ mu, const double* __restrict__ sn,
                                                              const uint64_t* __restrict__ keys, double* __restrict__ eps, T* __restrict__ V,
                                                              long mpad, long vs) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= Npad * mpad) return;
    const long i = e / mpad;
    const int t = (int)(e % mpad), r = rows[blockIdx.y];
    T* Vs = V + (long)blockIdx.y * vs;
    if (i >= N || t >= count[r]) { Vs[e] = (T)0; return; }
    const long s = start[r] + t;
    double f = 0.0;
    for (int q = 0; q < nstrips; ++q) f += part[(long)q * epad + s * N + i];
    const double ep = sn[r] * philox_normal(keys[r], (uint32_t)t, (uint32_t)i);
    eps[s * N + i] = ep;
    Vs[e] = (T)((y[i] - mu[r]) - f - ep);
}

// the substituted rows of a group back into the object's block: v(s, i) at out[i spad + s]
template <typename T>
__global__ __launch_bounds__(256) void paths_mix_gather_kernel(const T* __restrict__ V, long mpad, long vs, long Npad, const int* __restrict__ rows,
                                                               const int* __restrict__ start, const int* __restrict__ count,
                                                               T* __restrict__ out, long spad) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= Npad * mpad) return;
    const long i = e / mpad;
    const int t = (int)(e % mpad), r = rows[blockIdx.y];
    if (t < count[r]) out[i * spad + start[r] + t] = V[(long)blockIdx.y * vs + e];
}

// flag[row_of[s]] = 1 when a v(s, i), s < S, i < N, is not finite (every thread that finds one stores the same word)
template <typename T>
__global__ __launch_bounds__(256) void paths_mix_finite_kernel(const T* __restrict__ v, long N, long spad, int S, const int* __restrict__ row_of,
                                                               int* __restrict__ flag) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < N * spad; e += (long)gridDim.x * 256) {
        const int s = (int)(e % spad);
        if (s < S && !isfinite((double)v[e])) flag[row_of[s]] = 1;
    }
}

// v(s, i) = NaN for the draws of the rows with bad[r] != 0: they evaluate to NaN, values and gradients
template <typename T>
__global__ __launch_bounds__(256) void paths_mix_poison_kernel(T* __restrict__ v, long N, long spad, int S, const int* __restrict__ row_of,
                                                               const int* __restrict__ bad) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < N * spad; e += (long)gridDim.x * 256) {
        const int s = (int)(e % spad);
        if (s < S && bad[row_of[s]]) v[e] = (T)__builtin_nan("");
    }
}

}  // namespace gphip
