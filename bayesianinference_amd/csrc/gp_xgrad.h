// gp_xgrad.h -- device side of the gradients of the predictive mean and variance in the TEST inputs (include/gphip.h
// gphip_predict_grad, gphip_sparse_predict_grad).  Included by gphip_xgrad.inc.  Written for the exact
// object; the sparse object runs the same kernel with a = a_mu, W = L_u^-T (V1 - sn^2 L_B^-T V2) and the inducing points as p_j.
//
//     dmu /dx*_c  =      sum_j a_j     dk(x*, p_j)/dx*_c          a = alpha = K^-1 (y - m)        (a broadcast vector)
//     dvar/dx*_c  = -2   sum_j W(t, j) dk(x*, p_j)/dx*_c          W(t, .) = K^-1 k(X, x*_t)       (a matrix entry per pair)
//     dk(x*, p)/dx*_c = -(dk/dk_s) sf_s^2 m2dg_s(r_s^2) u_sc / l_sc,   u_sc = (x*_c - p_c) / l_sc     per term s (kfamily's m2dg)
// The kernel leaves A_s(t, c) = sum_j w (dk/dk_s) sf_s^2 m2dg_s u_sc for both weights; the finish kernel adds the strips in order,
// divides by l_sc and applies the signs (-1 for the mean, +2 for the variance).
//
// The outputs are the test points, the contraction runs over the points p_j (training points).  W is what the backward
// substitution leaves in the V block: W(t, j) at W[j ldw + t], the test index contiguous -- the transpose of what
// sparse_zgrad_kernel faces.  So a thread owns ONE test point: the lanes read their weights coalesced straight from global memory,
// the slab of contraction points and of the broadcast weights is an LDS broadcast (all lanes read the same j), the thread's own
// coordinates and its accumulators stay in registers.  kfamily is evaluated once per pair and feeds both accumulator sets.
// fp64 accumulation whatever T is; contracting with the differences u and not with sum f x* - x* sum f keeps the cancellation out
// (see sparse_zgrad_kernel).  No atomics, every sum in a fixed order: two calls return the same bytes.
//
// DW = coordinates held per term (zero-filled from d to DW).  GLB: more than KB_LDS_MAXD dimensions (two terms: more than 16) --
// the points come from global memory and one launch covers the window [d0, d0 + DW) of coordinates.  TWO: the covariance form
// has a second term.  VAR: the matrix-weighted accumulators exist (dvar was asked for).
// Partials: part[((strip nterm + s) nv + which) mpad d + t d + c], nv = VAR ? 2 : 1, which = 0 mean / 1 variance.
// grid = (mpad / 128, strips), 128 threads.
#pragma once

namespace gphip {

template <typename T>
struct XGradArgs {
    const T* W; long ldw;                      // W(t, j) at W[j ldw + t] (VAR only)
    const T* a;                                // the broadcast weights [ncon]
    const T* xt; const T* xt2; int ldt;        // scaled test points [d][ldt] of term 1 / term 2
    const T* xc; const T* xc2; int ldc;        // scaled contraction points [d][ldc]
    int ntest, ncon, d, d0;
    int strip_cols;                            // contraction points per strip (multiple of XG_TS)
    const double* slotp; KSpec ks;
    double* part; int mpad;
};

constexpr int XG_TS = 64;                      // contraction points per slab

template <typename T, int DW, bool GLB> __host__ __device__ constexpr size_t predict_xgrad_lds(int nterm) {
    return (XG_TS + (GLB ? 0 : (size_t)nterm * DW * XG_TS)) * sizeof(T);
}

template <typename T, int DW, bool GLB, bool TWO, bool VAR>
__global__ __launch_bounds__(128) void predict_xgrad_kernel(XGradArgs<T> a) {
    extern __shared__ double lds_raw[];
    constexpr bool two = TWO;
    constexpr int DW2 = TWO ? DW : 1, DWV = VAR ? DW : 1, DWV2 = (VAR && TWO) ? DW : 1;
    T* aw = reinterpret_cast<T*>(lds_raw);       // [64] broadcast weights of the slab
    T* cj1 = aw + XG_TS;                         // [DW][64] slab points of term 1, then of term 2
    T* cj2 = cj1 + DW * XG_TS;
    const int tid = threadIdx.x, t = blockIdx.x * TB + tid;
    const int d = a.d, d0 = GLB ? a.d0 : 0;
    const bool live = t < a.ntest;
    const long j0 = (long)blockIdx.y * a.strip_cols;
    const long j1 = j0 + a.strip_cols < a.ncon ? j0 + a.strip_cols : a.ncon;
    const double* sp = a.slotp;
    const double sf2a = sp[0], sf2b = two ? sp[SP_SF2B] : 0.0;
    const T al1 = (T)sp[SP_ALPHA1], al2 = (T)sp[SP_ALPHA2];
    T x1[DW], x2[DW2];                           // the thread's own point (the window's coordinates when GLB)
#pragma unroll
    for (int q = 0; q < DW; ++q) {
        const bool in = d0 + q < d;
        x1[q] = in ? a.xt[(long)(d0 + q) * a.ldt + t] : (T)0;
        if (two) x2[q] = in ? a.xt2[(long)(d0 + q) * a.ldt + t] : (T)0;
    }
    double am1[DW], am2[DW2], av1[DWV], av2[DWV2];
#pragma unroll
    for (int q = 0; q < DW; ++q) am1[q] = 0.0;
#pragma unroll
    for (int q = 0; q < DW2; ++q) am2[q] = 0.0;
#pragma unroll
    for (int q = 0; q < DWV; ++q) av1[q] = 0.0;
#pragma unroll
    for (int q = 0; q < DWV2; ++q) av2[q] = 0.0;
    for (long js = j0; js < j1; js += XG_TS) {
        __syncthreads();                         // (the previous slab has been read)
        if (tid < XG_TS) aw[tid] = js + tid < j1 ? a.a[js + tid] : (T)0;
        if (!GLB)
            for (int idx = tid; idx < DW * XG_TS; idx += TB) {
                const int c = idx / XG_TS, q = idx % XG_TS;
                const bool in = c < d && js + q < j1;
                cj1[idx] = in ? a.xc[(long)c * a.ldc + js + q] : (T)0;
                if (two) cj2[idx] = in ? a.xc2[(long)c * a.ldc + js + q] : (T)0;
            }
        __syncthreads();
        const int nj = (int)(j1 - js < XG_TS ? j1 - js : XG_TS);
        if (!live) continue;
        for (int jl = 0; jl < nj; ++jl) {
            const long j = js + jl;
            T u1[DW], u2[DW2];
            T r2a = (T)0, r2b = (T)0;
            if (GLB) {
                for (int c = 0; c < d; ++c) {
                    const T u = a.xt[(long)c * a.ldt + t] - a.xc[(long)c * a.ldc + j];
                    r2a += u * u;
                }
                if (two)
                    for (int c = 0; c < d; ++c) {
                        const T u = a.xt2[(long)c * a.ldt + t] - a.xc2[(long)c * a.ldc + j];
                        r2b += u * u;
                    }
#pragma unroll
                for (int q = 0; q < DW; ++q) {
                    const bool in = d0 + q < d;
                    u1[q] = in ? x1[q] - a.xc[(long)(d0 + q) * a.ldc + j] : (T)0;
                    if (two) u2[q] = in ? x2[q] - a.xc2[(long)(d0 + q) * a.ldc + j] : (T)0;
                }
            } else {
#pragma unroll
                for (int q = 0; q < DW; ++q) {
                    u1[q] = x1[q] - cj1[q * XG_TS + jl];
                    r2a += u1[q] * u1[q];
                }
                if (two) {
#pragma unroll
                    for (int q = 0; q < DW; ++q) {
                        u2[q] = x2[q] - cj2[q * XG_TS + jl];
                        r2b += u2[q] * u2[q];
                    }
                }
            }
            T g1, m1, da1, g2 = (T)0, m2 = (T)0, da2 = (T)0;
            kfamily<T>(a.ks.fam1, r2a, al1, g1, m1, da1);
            if (two) kfamily<T>(a.ks.fam2, r2b, al2, g2, m2, da2);
            const double k1 = sf2a * (double)g1, k2 = sf2b * (double)g2;
            const double dk1 = (a.ks.op == 2) ? k2 : 1.0, dk2 = (a.ks.op == 2) ? k1 : 1.0;       // dk/dk1, dk/dk2
            const double f1 = dk1 * sf2a * (double)m1, f2 = dk2 * sf2b * (double)m2;
            const double wm = (double)aw[jl];
            const double fm1 = wm * f1, fm2 = wm * f2;
#pragma unroll
            for (int q = 0; q < DW; ++q) am1[q] = __builtin_fma(fm1, (double)u1[q], am1[q]);
            if (two) {
#pragma unroll
                for (int q = 0; q < DW; ++q) am2[q] = __builtin_fma(fm2, (double)u2[q], am2[q]);
            }
            if constexpr (VAR) {
                const double wv = (double)a.W[j * a.ldw + t];
                const double fv1 = wv * f1, fv2 = wv * f2;
#pragma unroll
                for (int q = 0; q < DW; ++q) av1[q] = __builtin_fma(fv1, (double)u1[q], av1[q]);
                if constexpr (TWO) {
#pragma unroll
                    for (int q = 0; q < DW; ++q) av2[q] = __builtin_fma(fv2, (double)u2[q], av2[q]);
                }
            }
        }
    }
    if (!live) return;
    constexpr int nterm = TWO ? 2 : 1, nv = VAR ? 2 : 1;
    const long md = (long)a.mpad * d;
    double* p = a.part + (long)blockIdx.y * nterm * nv * md + (long)t * d + d0;
#pragma unroll
    for (int q = 0; q < DW; ++q)
        if (d0 + q < d) {
            p[q] = am1[q];
            if constexpr (VAR) p[md + q] = av1[q];
            if constexpr (TWO) {
                p[nv * md + q] = am2[q];
                if constexpr (VAR) p[(nv + 1) * md + q] = av2[q];
            }
        }
}

// dmean(t, c) = -sum_s (sum over the strips of A_s mean) / l_sc,  dvar(t, c) = +2 sum_s (.. A_s variance) / l_sc, strips in order.
// ie1 / ie2: 1 / l of the two terms [d]; n = ntest x d entries of the row-major outputs; dvar: null without the variance.
__global__ __launch_bounds__(256) void predict_xgrad_finish_kernel(const double* __restrict__ part, int nstrips, int nterm, int nv, long md, long n,
                                                                   int d, const double* __restrict__ ie1, const double* __restrict__ ie2,
                                                                   double* __restrict__ dmean, double* __restrict__ dvar) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % d);
    for (int which = 0; which < nv; ++which) {
        double s1 = 0.0, s2 = 0.0;
        for (int q = 0; q < nstrips; ++q) {
            s1 += part[((long)q * nterm * nv + which) * md + idx];
            if (nterm == 2) s2 += part[(((long)q * nterm + 1) * nv + which) * md + idx];
        }
        double v = s1 * ie1[c];
        if (nterm == 2) v += s2 * ie2[c];
        if (which == 0) dmean[idx] = -v;
        else dvar[idx] = 2.0 * v;
    }
}

// the sparse object's weights before the substitution with L_u: X <- V1 - s X (X = L_B^-T V2 on entry), n elements
template <typename T>
__global__ void sparse_xgrad_combine_kernel(const T* __restrict__ V1, T* __restrict__ X, long n, double s) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        X[i] = (T)((double)V1[i] - s * (double)X[i]);
}

}  // namespace gphip
