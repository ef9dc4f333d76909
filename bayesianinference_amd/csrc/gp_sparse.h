// gp_sparse.h -- device kernels of the sparse inducing-point GP (include/gphip.h: gphip_sparse_*, gphip_sparse.inc).
//
//   sparse_accumulate_kernel     C += V^T V and the rhs row += r^T V on the lower tiles of b's workspace (the hot path; gp_contract.h)
//   (the first four kernels and strip_reduce_kernel carry a slot dimension for gphip_sparse_bound_batch: one theta per workspace
//    slot, slot = the grid's last index, every operand addressed as slot-0 base + slot x stride; the one-theta calls run them with one slot)
//   sparse_resid_kernel          r = y - mu of a chunk into row 0 of the rhs operand + per-block partial sums of r^2
//   sparse_resid_pw_kernel       point-dependent mean and noise: r = y - m_i, the weight row w = 1 / nu_i, partial sums of r^2 w, log nu, w
//   sparse_scale_rows_kernel     option "sparse_pw_fused" = 0 (the default): V(t, .) and r_t times sqrt(w_t) in place, ahead of the unweighted accumulation
//   sparse_blocksum_kernel       per-block partial sums of a double vector (k(x_i, x_i) of a run-time compiled kernel)
//   sparse_diag_kernel           tr(V V^T) from C's diagonal, then + sn^2 on it (identity on the pad)
//   sparse_predict_finish_kernel mean and variance of a chunk of test points from the strip partials of v1 and v2, per slot
//   sparse_handover_kernel       gphip_sparse_predict_samples: V1 of every slot from u's dV into b's + the strip partials of |v1|^2
//   sparse_small / _trace / _vta / _w / _weight / _transpose_kernel   the gradient of the bound, see the second half of this file
//   sparse_zgrad_kernel / sparse_zgrad_finish_kernel   the gradient of the bound in the inducing LOCATIONS, see the end of this file
#pragma once
#include "gp_contract.h"

namespace gphip {

constexpr int SPARSE_PAR = 4;                  // doubles per slot of the sparse object's own scalars: mu, sn^2 of B, k(x, x), the noise of theta
constexpr int SPARSE_PAR_NOISE = 3;            // (par[1] is the sn^2 of B = sn^2 I + V V^T: 1 once the data are whitened by 1 / nu_i)

// ---------------------------------------------------------------------------------------------
// Accumulation: strip_contract (gp_contract.h) with the contiguous-k operands.  V is the chunk of L_u^-1 k(Z, X) the forward
// substitution leaves: column-major, V(t, k) at V[t + k ldv], t = data point of the chunk, k = inducing index.  Output tile
// (ti, tj) of b's tile-major workspace takes
//     C(k1, k2) += sum_t V(t, k1) V(t, k2),      rhs tile row: row 0 += sum_t r_t V(t, k)
// so the contraction index t is the contiguous one of both operands.  The rhs operand is 16 rows x ldr (row 0 = r of the chunk,
// rows 1 .. 15 zero).  One workgroup = one output tile x one strip of the chunk's rows x one slot.
// ---------------------------------------------------------------------------------------------
// Weighted form (point-dependent noise): C(k1, k2) += sum_t V(t, k1) w_t V(t, k2), rhs row 0 +=
// sum_t r_t w_t V(t, k), w = 1 / nu the weight row of the chunk (W: one row of ldw elements per slot, zero on the pad).  The weight
// is the J-scale policy of the one contraction, chosen at compile time: the constant form's instantiation does not know of it.
// (Option "sparse_pw_fused" = 1; the default is the scaling pass of sparse_scale_rows_kernel, see the measurement in DESIGN.md 8i.)
template <typename T>
struct SparseAccArgs : ContractArgs<T> {
    long ldr;                    // leading dimension of the rhs operand Z
    const T* W; long ldw;        // weighted form: the weight rows
};

template <typename T, bool WEIGHTED>
__device__ __forceinline__ auto sparse_jscale(const SparseAccArgs<T>& g) {
    if constexpr (WEIGHTED) return JWeight<T, SwizzledK<T>::GK>(g.W + (long)blockIdx.z * g.ldw, (long)blockIdx.y * g.kstrip, g.K);
    else return JIdentity<T>{};
}

template <typename T, bool WEIGHTED>
__global__ __launch_bounds__(256, 2) void sparse_accumulate_kernel(SparseAccArgs<T> g) {
    strip_contract<T>(g, SwizzledK<T>{g.ldr}, sparse_jscale<T, WEIGHTED>(g));
}

// fixed-order sum of the 256 values of a workgroup (one per thread); the result is valid in thread 0
__device__ __forceinline__ double sparse_block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    return red[0];
}

// rz[t] = y[t] - mu for t < n, 0 for n <= t < npad (the residual in the handle's arithmetic type), part[block] = sum of the
// block's rz^2 in fp64.  grid = (ceil(npad / 256), slots): slot s subtracts mu[s mu_stride] and writes rz + s r_bstride,
// part + s p_bstride.
template <typename T>
__global__ __launch_bounds__(256) void sparse_resid_kernel(const T* __restrict__ y, int n, int npad, const double* __restrict__ muv,
                                                           int mu_stride, T* __restrict__ rz, long r_bstride, double* __restrict__ part,
                                                           long p_bstride) {
    __shared__ double red[256];
    const int t = blockIdx.x * 256 + threadIdx.x;
    const double mu = muv[(long)blockIdx.y * mu_stride];
    rz += (long)blockIdx.y * r_bstride;
    part += (long)blockIdx.y * p_bstride;
    const T r = t < n ? (T)(y[t] - (T)mu) : (T)0;
    if (t < npad) rz[t] = r;
    const double s = sparse_block_sum((double)r * (double)r, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// The point-dependent form of sparse_resid_kernel.  mean / nug: this chunk's slice of the group's arrays (fp64, slot s at
// + s a_bstride); a null array is the slot's constant par[0] (mu) / par[SPARSE_PAR_NOISE] (sn^2), broadcast.
//   rz[t] = y[t] - m_t, wz[t] = 1 / nu_t for t < n, both 0 for n <= t < npad (the handle's arithmetic type)
//   part[block], part[2 pn + block], part[3 pn + block] = the block's sums of r^2 w, log nu and w in fp64 (w as the kernel uses it;
//   part[pn + block] is sparse_blocksum_kernel's)
// grid = (ceil(npad / 256), slots).
template <typename T>
__global__ __launch_bounds__(256) void sparse_resid_pw_kernel(const T* __restrict__ y, int n, int npad, const double* __restrict__ par,
                                                              const double* __restrict__ mean, const double* __restrict__ nug, long a_bstride,
                                                              T* __restrict__ rz, long r_bstride, T* __restrict__ wz, long w_bstride,
                                                              double* __restrict__ part, long p_bstride, long pn) {
    __shared__ double red[256];
    const int t = blockIdx.x * 256 + threadIdx.x;
    const long slot = blockIdx.y;
    par += SPARSE_PAR * slot;
    rz += slot * r_bstride;
    wz += slot * w_bstride;
    part += slot * p_bstride;
    T r = (T)0, w = (T)0;
    double lognu = 0.0;
    if (t < n) {
        const double m = mean ? mean[slot * a_bstride + t] : par[0];
        const double nu = nug ? nug[slot * a_bstride + t] : par[SPARSE_PAR_NOISE];
        r = (T)(y[t] - (T)m);
        w = (T)(1.0 / nu);
        lognu = log(nu);
    }
    if (t < npad) { rz[t] = r; wz[t] = w; }
    double s = sparse_block_sum((double)r * (double)r * (double)w, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
    __syncthreads();
    s = sparse_block_sum(lognu, red);
    if (threadIdx.x == 0) part[2 * pn + blockIdx.x] = s;
    __syncthreads();
    s = sparse_block_sum((double)w, red);
    if (threadIdx.x == 0) part[3 * pn + blockIdx.x] = s;
}

// V(t, k) *= sqrt(w_t) for the npad rows x ncols columns of every slot's chunk, and r_t *= sqrt(w_t): after it the unweighted
// accumulation gives the weighted sums.  grid = (npad / 256, ncols + 1, slots); column ncols is the residual row.
template <typename T>
__global__ __launch_bounds__(256) void sparse_scale_rows_kernel(T* __restrict__ V, long ldv, long v_bstride, int ncols, T* __restrict__ rz,
                                                                long r_bstride, const T* __restrict__ wz, long w_bstride, int npad) {
    const int t = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    const long slot = blockIdx.z;
    if (t >= npad) return;
    const T s = (T)sqrt((double)wz[slot * w_bstride + t]);
    T* p = k < ncols ? V + slot * v_bstride + (long)k * ldv + t : rz + slot * r_bstride + t;
    *p *= s;
}

// part[block] = sum of v[t] (w: v[t] w[t]), t < n, over the block's 256 entries.  grid = (blocks, slots): slot s reads
// v + s v_bstride and w + s w_bstride
template <typename W>
__global__ __launch_bounds__(256) void sparse_blocksum_kernel(const double* __restrict__ v, long v_bstride, int n, double* __restrict__ part,
                                                              long p_bstride, const W* __restrict__ w, long w_bstride) {
    __shared__ double red[256];
    const int t = blockIdx.x * 256 + threadIdx.x;
    v += (long)blockIdx.y * v_bstride;
    part += (long)blockIdx.y * p_bstride;
    double x = t < n ? v[t] : 0.0;
    if (w && t < n) x *= (double)w[(long)blockIdx.y * w_bstride + t];
    const double s = sparse_block_sum(x, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// The diagonal of the accumulated V V^T in b's workspace: out[0] = its sum over the m inducing points (fixed order), then
// C(k, k) += sn2 for k < m and C(k, k) = 1 on the pad (k < 128 Mt).  One workgroup per slot: slot s works on C + s c_bstride
// with sn2 = sn2v[s sn2_stride] and writes out[s o_bstride].
template <typename T>
__global__ __launch_bounds__(256) void sparse_diag_kernel(T* __restrict__ C, long c_bstride, int R, int m, int mpad,
                                                          const double* __restrict__ sn2v, int sn2_stride, double* __restrict__ out,
                                                          long o_bstride) {
    __shared__ double red[256];
    const double sn2 = sn2v[(long)blockIdx.x * sn2_stride];
    C += (long)blockIdx.x * c_bstride;
    out += (long)blockIdx.x * o_bstride;
    double s = 0.0;
    for (int k = threadIdx.x; k < mpad; k += 256) {
        T* p = C + tile_index(k >> 7, k >> 7, R) * TS + (long)(k & 127) * (TB + 1);
        if (k < m) {
            const double v = (double)*p;
            s += v;
            *p = (T)(v + sn2);
        } else {
            *p = (T)1;
        }
    }
    s = sparse_block_sum(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

// Prediction epilogue, one slot per blockIdx.y (the one-theta call: one slot).  part1: strip partials of |v1|^2, v1 = L_u^-1 k(Z, x*),
// strip s of slot q at part1[q p1_bstride + s p1_sstride + t] (predict_partial_kernel's norm rows of u, or what
// sparse_handover_kernel leaves); part2: predict_partial_kernel's [slot][strip][2][mpad] for v2 = L_B^-1 v1 against c (dots and
// norms).  par: [slot][SPARSE_PAR] = mu, sn^2 and the scalar k(x, x) of the slot's theta; kss [slot][mpad] (run-time compiled
// kernels): k(x*, x*) per point in its place.  mean, var: [slot][mpad].  par[1] is the sn^2 of B = sn^2 I + V V^T (1 for a whitened
// fit), par[3] the noise variance at a test point; mean_t / nug_t ([slot][mpad] or null): m(x*) / nu(x*) per point in their place.
//     mean = mu + v2^T c        var = k(x*, x*) [+ noise] - |v1|^2 + sn2 |v2|^2
__global__ void sparse_predict_finish_kernel(const double* __restrict__ part1, int nstrips1, long p1_sstride, long p1_bstride,
                                             const double* __restrict__ part2, int nstrips2, long mpad, int mc,
                                             const double* __restrict__ par, const double* __restrict__ kss, int latent,
                                             const double* __restrict__ mean_t, const double* __restrict__ nug_t,
                                             double* __restrict__ mean, double* __restrict__ var) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int slot = blockIdx.y;
    if (t >= mc) return;
    const double mu = par[SPARSE_PAR * slot], sn2 = par[SPARSE_PAR * slot + 1];
    part1 += (long)slot * p1_bstride;
    part2 += (long)slot * nstrips2 * 2 * mpad;
    double n1 = 0.0, dot = 0.0, n2 = 0.0;
    for (int s = 0; s < nstrips1; ++s) n1 += part1[(long)s * p1_sstride + t];
    for (int s = 0; s < nstrips2; ++s) {
        dot += part2[((long)s * 2 + 0) * mpad + t];
        n2 += part2[((long)s * 2 + 1) * mpad + t];
    }
    const long o = (long)slot * mpad + t;
    const double noise = nug_t ? nug_t[o] : par[SPARSE_PAR * slot + SPARSE_PAR_NOISE];
    mean[o] = (mean_t ? mean_t[o] : mu) + dot;
    var[o] = (kss ? kss[o] : par[SPARSE_PAR * slot + 2]) + (latent ? 0.0 : noise) - n1 + sn2 * n2;
}

// gphip_sparse_predict_samples: V1 = L_u^-1 k(Z, X*) of every slot of a group goes from u's dV into b's, and the norms |v1|^2 are
// taken on the way -- ONE pass that reads V1 once (the one-theta call copies device to device and then runs
// predict_partial_kernel on u: two reads, one write).  predict_partial_kernel's access pattern: one workgroup per 128 test points
// x strip of js columns x slot, wave w takes columns w, w + 4, .. of the strip, a lane moves 2 adjacent test points per column
// (fp64: one 16-byte load and store), four columns in flight per wave, fp64 partial sums that meet in LDS in a fixed order.
// Columns [ncols, ncols_pad) are the pad of the inducing points: copied (b substitutes over whole tiles), not summed.
// grid = (mpad / 128, nstrips, nslots); V (both): V(t, j) at V[slot bstride + t + j ldv]; part: [slot][strip][mpad].
template <typename T>
__global__ __launch_bounds__(256) void sparse_handover_kernel(const T* __restrict__ V, T* __restrict__ out, long ldv, long bstride,
                                                              int ncols, int ncols_pad, int js, double* __restrict__ part, int nstrips) {
    __shared__ double red[4 * TB];
    typedef typename Num<T>::pair_t pair_t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tb = blockIdx.x, strip = blockIdx.y, slot = blockIdx.z;
    const int j0 = strip * js;
    const int jn = (ncols - j0 < js) ? (ncols - j0) : js;           // columns of this strip that are summed (<= 0: none)
    const int jc = (ncols_pad - j0 < js) ? (ncols_pad - j0) : js;   // columns of this strip that are copied
    const long base = (long)slot * bstride + (long)tb * TB + 2 * lane;
    V += base;
    out += base;
    double n0 = 0.0, n1 = 0.0;
    int j = wave;
    for (; j + 12 < jn; j += 16) {                // four independent 16-byte loads in flight per lane
        pair_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const pair_t*>(V + (long)(j0 + j + 4 * u) * ldv);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            *reinterpret_cast<pair_t*>(out + (long)(j0 + j + 4 * u) * ldv) = v[u];
            const double a = (double)v[u].x, b = (double)v[u].y;
            n0 = __builtin_fma(a, a, n0); n1 = __builtin_fma(b, b, n1);
        }
    }
    for (; j < jn; j += 4) {
        const pair_t v = *reinterpret_cast<const pair_t*>(V + (long)(j0 + j) * ldv);
        *reinterpret_cast<pair_t*>(out + (long)(j0 + j) * ldv) = v;
        const double a = (double)v.x, b = (double)v.y;
        n0 = __builtin_fma(a, a, n0); n1 = __builtin_fma(b, b, n1);
    }
    for (; j < jc; j += 4)
        *reinterpret_cast<pair_t*>(out + (long)(j0 + j) * ldv) = *reinterpret_cast<const pair_t*>(V + (long)(j0 + j) * ldv);
    red[wave * TB + 2 * lane] = n0; red[wave * TB + 2 * lane + 1] = n1;
    __syncthreads();
    if (tid < TB) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) s += red[w * TB + tid];
        part[((long)slot * nstrips + strip) * ldv + (long)tb * TB + tid] = s;
    }
}

// ---------------------------------------------------------------------------------------------
// The gradient of the bound (gphip_sparse_bound_grad).  With a = L_B^-T c, w = (r - V^T a) / sn^2 and
// D = I / sn^2 - B^-1 the weights of d k(Z, X) are G = L_u^-T (D V + a w^T), those of d k(Z, Z) are
// H = L_u^-T [I - sn^2 B^-1 / 2 - a a^T / 2 - B / (2 sn^2)] L_u^-1; both reach the gradient reductions of gp_kernels.h as the
// "K^-1" operand scaled by -2 (their weight is -Kinv and the chain rule halves the sums).
//
//   sparse_small_kernel          S = D and Hm = -2 [..] (dense, symmetric, zero on the pad) from B^-1, a and the saved B
//   sparse_trace_kernel          tr B^-1 and a^T a over the m inducing points
//   sparse_vta_kernel            strip partials of V^T a for a chunk
//   sparse_w_kernel              w of a chunk (fp64) + per-block partial sums of w
//   sparse_weight_kernel         T = scale (V S + w a^T) on the matrix pipe (the hot path)
//   sparse_transpose_kernel      out = in^T of a square column-major matrix
// ---------------------------------------------------------------------------------------------

// Binv: B^-1, column-major with leading dimension ld (= mpad; its lower triangle is read); a [mpad]; Bt: the tile-major lower tiles
// of B = sn^2 I + V V^T as they were before the factorisation (R tile rows).  S and Hm: column-major, leading dimension mpad.
template <typename T>
__global__ __launch_bounds__(256) void sparse_small_kernel(const T* __restrict__ Binv, long ld, const T* __restrict__ a, const T* __restrict__ Bt,
                                                           int R, int m, int mpad, double sn2, T* __restrict__ S, T* __restrict__ Hm) {
    const long total = (long)mpad * mpad;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int i = (int)(idx % mpad), j = (int)(idx / mpad);
        double s = 0.0, hm = 0.0;
        if (i < m && j < m) {
            const int lo = i < j ? i : j, hi = i < j ? j : i;              // element (hi, lo) of the lower triangle
            const double binv = (double)Binv[(long)lo * ld + hi];
            const double b = (double)Bt[tile_index(hi >> 7, lo >> 7, R) * TS + (long)(lo & 127) * TB + (hi & 127)];
            const double eye = i == j ? 1.0 : 0.0;
            s = eye / sn2 - binv;
            hm = -2.0 * (eye - 0.5 * sn2 * binv - 0.5 * (double)a[i] * (double)a[j] - b / (2.0 * sn2));
        }
        S[idx] = (T)s;
        Hm[idx] = (T)hm;
    }
}

// out[0] = tr B^-1, out[1] = a^T a, both over k < m in a fixed order.  One workgroup.
template <typename T>
__global__ __launch_bounds__(256) void sparse_trace_kernel(const T* __restrict__ Binv, long ld, const T* __restrict__ a, int m,
                                                           double* __restrict__ out) {
    __shared__ double red[256];
    double s = 0.0, q = 0.0;
    for (int k = threadIdx.x; k < m; k += 256) {
        s += (double)Binv[(long)k * ld + k];
        q += (double)a[k] * (double)a[k];
    }
    s = sparse_block_sum(s, red);
    __syncthreads();
    q = sparse_block_sum(q, red);
    if (threadIdx.x == 0) { out[0] = s; out[1] = q; }
}

// part[strip][t] = sum over the strip's 128 inducing indices of V(t, k) a_k.  grid = (npad_t / 256, Mt).
template <typename T>
__global__ __launch_bounds__(256) void sparse_vta_kernel(const T* __restrict__ V, long ldv, const T* __restrict__ a, int npad_t,
                                                         double* __restrict__ part) {
    __shared__ double as[TB];
    const int t = blockIdx.x * 256 + threadIdx.x, k0 = blockIdx.y * TB;
    if (threadIdx.x < TB) as[threadIdx.x] = (double)a[k0 + threadIdx.x];
    __syncthreads();
    if (t >= npad_t) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const T* v = V + (long)k0 * ldv + t;
#pragma unroll 2
    for (int k = 0; k < TB; k += 4) {
        s0 = __builtin_fma((double)v[(long)k * ldv], as[k], s0);
        s1 = __builtin_fma((double)v[(long)(k + 1) * ldv], as[k + 1], s1);
        s2 = __builtin_fma((double)v[(long)(k + 2) * ldv], as[k + 2], s2);
        s3 = __builtin_fma((double)v[(long)(k + 3) * ldv], as[k + 3], s3);
    }
    part[(long)blockIdx.y * npad_t + t] = (s0 + s1) + (s2 + s3);
}

// w[t] = (r_t - sum_strips part[strip][t]) / sn2 for t < n, 0 on the pad; wsum[block] = the block's sum of w.  grid = npad_t / 256.
template <typename T>
__global__ __launch_bounds__(256) void sparse_w_kernel(const T* __restrict__ rz, const double* __restrict__ part, int nstrips, int n,
                                                       int npad_t, double sn2, double* __restrict__ w, double* __restrict__ wsum) {
    __shared__ double red[256];
    const int t = blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (t < n) {
        double s = 0.0;
        for (int q = 0; q < nstrips; ++q) s += part[(long)q * npad_t + t];
        v = ((double)rz[t] - s) / sn2;
    }
    if (t < npad_t) w[t] = v;
    const double tot = sparse_block_sum(v, red);
    if (threadIdx.x == 0) wsum[blockIdx.x] = tot;
}

// ---------------------------------------------------------------------------------------------
// T(t, k) = scale (sum_k' V(t, k') S(k', k) + w_t a_k) for a chunk: V(t, k') at V[t + k' ldv] as the forward substitution leaves it,
// S the symmetric m x m matrix of sparse_small_kernel (column-major, leading dimension lds_), out(t, k) at out[t + k ldo] -- the
// layout queue_backward_rows and the gradient reductions read.  The contraction runs over the INDUCING index k', the strided one
// of V (downdate_kernel's orientation, not sparse_accumulate_kernel's): for one k' both operands are contiguous in their output
// index (V in t; S, being symmetric, in k), so a stage is KC rows of 128 contiguous elements per operand.
// One workgroup = one 128 (t) x 128 (k) output tile, 2 x 2 waves of 64 x 64, 4 x 4 accumulators of v_mfma_*_16x16x4 per wave
// (the accumulator layout of sparse_accumulate_kernel: i = t contiguous in the output, j = k).  Staging goes through registers
// into two LDS stages of KC = 8 rows per operand: global loads of stage s + 1 are issued before the MFMAs of stage s and stored
// after them, one barrier per stage.  An MFMA operand is one element per lane, row l & 15 at contraction index l >> 4: the 16
// lanes of one l >> 4 read 16 consecutive elements of one LDS row, and the row stride of 144 elements (= 16 mod 32 doubles,
// = 16 mod 64 floats) puts the rows of the lane groups that are served together on different banks: with 64 banks of 4 bytes the
// four groups of an fp32 read start at banks 0 / 16 / 32 / 48; an fp64 read is served half a wave at a time, and the two groups of
// a half start at banks 0 / 32 (groups 0 and 2 share banks, but not a half).  This follows from the layout; no bank-conflict
// counter has been read for it.  The kernel runs at 0.85 of the fp64 matrix-pipe figure at m = 8192.
// Pad rows of V (t beyond the chunk) and pad rows / columns of S are zeros, w_t is zero on the pad and a_k is zero for k >= m, so
// the pad of T comes out as exact zeros.  grid = (npad_t / 128, mpad / 128).
// ---------------------------------------------------------------------------------------------
template <typename T>
struct SparseWeightArgs {
    const T* V; long ldv;        // V(t, k') at V[t + k' ldv]
    const T* S; long lds;        // S(k', k) at S[k + k' lds] (symmetric)
    const double* w;             // [npad_t]
    const T* a;                  // [mpad]
    T* out; long ldo;            // out(t, k) at out[t + k ldo]
    int mpad;                    // padded inducing points: the contraction length (multiple of 128)
    double scale;
};

constexpr int SPW_KC = 8;                      // contraction indices per stage
constexpr int SPW_STR = 144;                   // elements between consecutive rows of a stage image

template <typename T>
__global__ __launch_bounds__(256, 2) void sparse_weight_kernel(SparseWeightArgs<T> g) {
    constexpr int FI = 4, FJ = 4;
    typedef typename Num<T>::acc_t acc_t;
    typedef T v4 __attribute__((ext_vector_type(4)));
    __shared__ __attribute__((aligned(32))) T img[2][2][SPW_KC * SPW_STR];      // [stage][V, S][row k'][128 (+ pad)]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave & 1, wj = wave >> 1;
    const int l15 = lane & 15, l4 = lane >> 4;
    const long t0 = (long)blockIdx.x * TB, k0 = (long)blockIdx.y * TB;
    // staging: thread -> row tid >> 5 of the stage, elements 4 (tid & 31) .. + 3 of it
    const int sr = tid >> 5, sc = (tid & 31) * 4;
    const T* vg = g.V + t0 + sc + (long)sr * g.ldv;
    const T* sg = g.S + k0 + sc + (long)sr * g.lds;
    const int so = sr * SPW_STR + sc;
    acc_t acc[FJ][FI];
#pragma unroll
    for (int x = 0; x < FJ; ++x)
#pragma unroll
        for (int y = 0; y < FI; ++y) acc[x][y] = (acc_t){0, 0, 0, 0};
    const int nk = g.mpad / SPW_KC;
    v4 rv = *reinterpret_cast<const v4*>(vg), rs = *reinterpret_cast<const v4*>(sg);
    *reinterpret_cast<v4*>(&img[0][0][so]) = rv;
    *reinterpret_cast<v4*>(&img[0][1][so]) = rs;
    __syncthreads();
    for (int kb = 0; kb < nk; ++kb) {
        const int cur = kb & 1;
        if (kb + 1 < nk) {
            rv = *reinterpret_cast<const v4*>(vg + (long)(kb + 1) * SPW_KC * g.ldv);
            rs = *reinterpret_cast<const v4*>(sg + (long)(kb + 1) * SPW_KC * g.lds);
        }
        const T* Vs = img[cur][0];
        const T* Ss = img[cur][1];
#pragma unroll
        for (int kk = 0; kk < SPW_KC / 4; ++kk) {
            T fi[FI], fj[FJ];
            const int row = (kk * 4 + l4) * SPW_STR;
#pragma unroll
            for (int f = 0; f < FI; ++f) fi[f] = Vs[row + wi * 64 + f * 16 + l15];
#pragma unroll
            for (int f = 0; f < FJ; ++f) fj[f] = Ss[row + wj * 64 + f * 16 + l15];
#pragma unroll
            for (int x = 0; x < FJ; ++x)
#pragma unroll
                for (int y = 0; y < FI; ++y) acc[x][y] = Num<T>::mfma(fj[x], fi[y], acc[x][y]);
        }
        if (kb + 1 < nk) {
            *reinterpret_cast<v4*>(&img[cur ^ 1][0][so]) = rv;
            *reinterpret_cast<v4*>(&img[cur ^ 1][1][so]) = rs;
        }
        __syncthreads();
    }
    // lane holds t = t0 + wi*64 + y*16 + (lane & 15), k = k0 + wj*64 + x*16 + drow(lane >> 4, r)
    double wt[FI];
#pragma unroll
    for (int y = 0; y < FI; ++y) wt[y] = g.w[t0 + wi * 64 + y * 16 + l15];
#pragma unroll
    for (int x = 0; x < FJ; ++x)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long k = k0 + wj * 64 + x * 16 + Num<T>::drow(l4, r);
            const double ak = (double)g.a[k];
            T* cp = g.out + k * g.ldo + t0 + wi * 64 + l15;
#pragma unroll
            for (int y = 0; y < FI; ++y) cp[y * 16] = (T)(g.scale * ((double)acc[x][y][r] + wt[y] * ak));
        }
}

// out(j, i) = in(i, j) for a square column-major matrix of n = 32 x gridDim.x rows (in: leading dimension ldi, out: ldo).
// grid = (n / 32, n / 32), 256 threads.
template <typename T>
__global__ __launch_bounds__(256) void sparse_transpose_kernel(const T* __restrict__ in, long ldi, T* __restrict__ out, long ldo) {
    __shared__ T t[32][33];
    const int bi = blockIdx.x * 32, bj = blockIdx.y * 32, x = threadIdx.x & 31, y0 = threadIdx.x >> 5;
    for (int y = y0; y < 32; y += 8) t[y][x] = in[(long)(bj + y) * ldi + bi + x];          // t[col][row]
    __syncthreads();
    for (int y = y0; y < 32; y += 8) out[(long)(bi + y) * ldo + bj + x] = t[x][y];          // element (bj + x, bi + y) <- (bi + y, bj + x)
}

// ---------------------------------------------------------------------------------------------
// The gradient of the bound in the inducing locations (gphip_sparse_bound_grad_inducing).  The weights are
// the ones the theta reductions contract -- W = -2 G per chunk, W = -2 H once -- but the sums run per COLUMN (inducing point)
// instead of over all entries:
//     A_s(j, c) = sum_t (-W(t, j)) (dk/dk_s) sf_s^2 m2dg_s(r_s^2) u_sc,     u_sc = xs_s(t, c) - zs_s(j, c)   (scaled differences)
// for term s of the covariance form, so that dF/dz_jc = scale sum_s A_s(j, c) / l_sc (scale = 1/2 for -2 G, 1 for -2 H: the sum
// over the rows of -2 H is already the 2 sum_l H_kl term; the l = k entry contributes u = 0).  Contracting with the differences
// and not with sum f x - z sum f keeps the cancellation out.
//
// One workgroup = one tile of 128 columns x one strip of rows, walked in slabs of 32 rows.  W is contiguous in t, the index the
// threads do NOT own, so a slab of it goes through LDS: the staging reads 32 consecutive t (256 / 128 bytes) per column, lanes
// along t, and stores the slab as [column][33]; thread (column jj, half) then reads its own row of the slab (stride 33 elements:
// 32 lanes of an fp64 read, 64 lanes of an fp32 read fall on distinct banks) while the slab's points are LDS broadcasts (all lanes
// read the same t) and the column points sit in LDS as [coordinate][128].  The two halves of the 256 threads take 16 rows of a
// slab each and leave separate partials: no cross-lane reduction, no atomics, every sum in a fixed order.
// DW = coordinates held per term (the tiles are zero-filled from d to DW: u = 0 there, no bounds test in the loops).  GLB: more than
// KB_LDS_MAXD dimensions (two terms: more than 16) -- the points come from global memory as in grad_reduce_general_kernel and one launch covers the window
// [d0, d0 + DW) of coordinates.  TWO: the covariance form has a second term (its accumulators exist only then).  Partials: part[(2 strip + half) nterm + s][mpad][d], fp64 whatever T is.
// grid = (mpad / 128, strips).
// ---------------------------------------------------------------------------------------------
template <typename T>
struct SparseZGradArgs {
    const T* W; long ldw;              // W(t, j) at W[j ldw + t]
    const T* xr; const T* xr2; int ldr;        // scaled row points [d][ldr] of term 1 / term 2
    const T* zs; const T* zs2; int ldz;        // scaled column points (Z) [d][ldz]
    int nrows, ncols, d, d0;
    int strip_rows;                    // rows per strip (multiple of 32)
    const double* slotp; KSpec ks;
    double* part; int mpad;
};

constexpr int ZG_TR = 32;                      // rows per slab
constexpr int ZG_PITCH = ZG_TR + 1;

template <typename T, int DW, bool GLB> __host__ __device__ constexpr size_t sparse_zgrad_lds(int nterm) {
    return ((size_t)TB * ZG_PITCH + (GLB ? 0 : (size_t)nterm * DW * (TB + ZG_TR))) * sizeof(T);
}

template <typename T, int DW, bool GLB, bool TWO>
__global__ __launch_bounds__(256) void sparse_zgrad_kernel(SparseZGradArgs<T> a) {
    extern __shared__ double lds_raw[];
    constexpr bool two = TWO;                    // a second term (a.ks.op != 0)
    constexpr int DW2 = TWO ? DW : 1;
    const int d = a.d, d0 = GLB ? a.d0 : 0;
    T* Ws = reinterpret_cast<T*>(lds_raw);       // [128][33] weight slab
    T* zj1 = Ws + TB * ZG_PITCH;                 // [DW][128] column points, [DW][32] slab points; then the same for term 2
    T* xt1 = zj1 + DW * TB;
    T* zj2 = xt1 + DW * ZG_TR;
    T* xt2 = zj2 + DW * TB;
    const int tid = threadIdx.x, jj = tid & 127, half = tid >> 7;
    const int j0 = blockIdx.x * TB, j = j0 + jj;
    const long r0 = (long)blockIdx.y * a.strip_rows;
    const long r1 = r0 + a.strip_rows < a.nrows ? r0 + a.strip_rows : a.nrows;
    if (!GLB)
        for (int idx = tid; idx < DW * TB; idx += 256) {
            const int c = idx >> 7, q = idx & 127;
            zj1[idx] = c < d ? a.zs[(long)c * a.ldz + j0 + q] : (T)0;
            if (two) zj2[idx] = c < d ? a.zs2[(long)c * a.ldz + j0 + q] : (T)0;
        }
    const double* sp = a.slotp;
    const double sf2a = sp[0], sf2b = two ? sp[SP_SF2B] : 0.0;
    const T al1 = (T)sp[SP_ALPHA1], al2 = (T)sp[SP_ALPHA2];
    double acc1[DW], acc2[DW2];
#pragma unroll
    for (int q = 0; q < DW; ++q) acc1[q] = 0.0;
#pragma unroll
    for (int q = 0; q < DW2; ++q) acc2[q] = 0.0;
    const int st = tid & 31, sc = tid >> 5;      // staging: row st of the slab, columns sc, sc + 8, ..
    for (long t0 = r0; t0 < r1; t0 += ZG_TR) {
        __syncthreads();                         // (the previous slab has been read)
        {
            const bool in = t0 + st < a.nrows;
            T v[16];
#pragma unroll
            for (int p = 0; p < 16; ++p) v[p] = in ? a.W[(long)(j0 + p * 8 + sc) * a.ldw + t0 + st] : (T)0;
#pragma unroll
            for (int p = 0; p < 16; ++p) Ws[(p * 8 + sc) * ZG_PITCH + st] = v[p];
        }
        if (!GLB)
            for (int idx = tid; idx < DW * ZG_TR; idx += 256) {
                const int c = idx >> 5, q = idx & 31;
                const bool in = c < d && t0 + q < a.nrows;
                xt1[idx] = in ? a.xr[(long)c * a.ldr + t0 + q] : (T)0;
                if (two) xt2[idx] = in ? a.xr2[(long)c * a.ldr + t0 + q] : (T)0;
            }
        __syncthreads();
        const int tl0 = half * (ZG_TR / 2);
        const int left = (int)(r1 - t0);
        const int tl1 = tl0 + ZG_TR / 2 < left ? tl0 + ZG_TR / 2 : left;
        if (j >= a.ncols) continue;
        for (int tl = tl0; tl < tl1; ++tl) {
            T u1[DW], u2[DW2];
            T r2a = (T)0, r2b = (T)0;
            if (GLB) {
                const long t = t0 + tl;
                for (int c = 0; c < d; ++c) {
                    const T u = a.xr[(long)c * a.ldr + t] - a.zs[(long)c * a.ldz + j];
                    r2a += u * u;
                }
                if (two)
                    for (int c = 0; c < d; ++c) {
                        const T u = a.xr2[(long)c * a.ldr + t] - a.zs2[(long)c * a.ldz + j];
                        r2b += u * u;
                    }
#pragma unroll
                for (int q = 0; q < DW; ++q) {
                    const bool in = d0 + q < d;
                    u1[q] = in ? a.xr[(long)(d0 + q) * a.ldr + t] - a.zs[(long)(d0 + q) * a.ldz + j] : (T)0;
                    if (two) u2[q] = in ? a.xr2[(long)(d0 + q) * a.ldr + t] - a.zs2[(long)(d0 + q) * a.ldz + j] : (T)0;
                }
            } else {
#pragma unroll
                for (int q = 0; q < DW; ++q) {
                    u1[q] = xt1[q * ZG_TR + tl] - zj1[q * TB + jj];
                    r2a += u1[q] * u1[q];
                }
                if (two) {
#pragma unroll
                    for (int q = 0; q < DW; ++q) {
                        u2[q] = xt2[q * ZG_TR + tl] - zj2[q * TB + jj];
                        r2b += u2[q] * u2[q];
                    }
                }
            }
            T g1, m1, da1, g2 = (T)0, m2 = (T)0, da2 = (T)0;
            kfamily<T>(a.ks.fam1, r2a, al1, g1, m1, da1);
            if (two) kfamily<T>(a.ks.fam2, r2b, al2, g2, m2, da2);
            const double k1 = sf2a * (double)g1, k2 = sf2b * (double)g2;
            const double dk1 = (a.ks.op == 2) ? k2 : 1.0, dk2 = (a.ks.op == 2) ? k1 : 1.0;       // dk/dk1, dk/dk2
            const double w = -(double)Ws[jj * ZG_PITCH + tl];
            const double f1 = w * dk1 * sf2a * (double)m1, f2 = w * dk2 * sf2b * (double)m2;
#pragma unroll
            for (int q = 0; q < DW; ++q) acc1[q] = __builtin_fma(f1, (double)u1[q], acc1[q]);
            if (two) {
#pragma unroll
                for (int q = 0; q < DW; ++q) acc2[q] = __builtin_fma(f2, (double)u2[q], acc2[q]);
            }
        }
    }
    const int nterm = two ? 2 : 1;
    const long md = (long)a.mpad * d;
    double* p1 = a.part + (long)(2 * blockIdx.y + half) * nterm * md + (long)j * d + d0;
#pragma unroll
    for (int q = 0; q < DW; ++q)
        if (d0 + q < d) {
            p1[q] = acc1[q];
            if (two) p1[md + q] = acc2[q];
        }
}

// acc(j, c) += scale sum_s (sum over the nparts partials of A_s(j, c)) / l_sc, partials in order.  ie1 / ie2: 1 / l of the two terms [d].
__global__ __launch_bounds__(256) void sparse_zgrad_finish_kernel(const double* __restrict__ part, int nparts, int nterm, long md, int d,
                                                                  const double* __restrict__ ie1, const double* __restrict__ ie2, double scale,
                                                                  double* __restrict__ acc) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= md) return;
    const int c = (int)(idx % d);
    double s1 = 0.0, s2 = 0.0;
    for (int q = 0; q < nparts; ++q) {
        s1 += part[(long)q * nterm * md + idx];
        if (nterm == 2) s2 += part[((long)q * nterm + 1) * md + idx];
    }
    double v = s1 * ie1[c];
    if (nterm == 2) v += s2 * ie2[c];
    acc[idx] += scale * v;
}

}  // namespace gphip
