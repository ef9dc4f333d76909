// Leave-one-out cross-validation (Rasmussen & Williams §5.4.2) from ONE factorisation: device kernels of gphip_loo / gphip_loo_grad.
//
//   alpha = K^-1 (y - m) = U z,   k_i = [K^-1]_ii = sum_{j >= i} U_ij^2          (U = L^-T upper triangular, z = L^-1 (y - m))
//   mu_-i = y_i - alpha_i / k_i,  var_-i = 1 / k_i,  log p_i = 1/2 log k_i - 1/2 alpha_i^2 / k_i - 1/2 log 2 pi
//   gradient:  g = alpha / k,  beta = K^-1 g,  c = 1 / k + g^2,  M = K^-1 diag(c) K^-1 = B B^T with B = K^-1 diag(sqrt c)
//              dL/dtheta = 1/2 sum_ab (alpha_a beta_b + beta_a alpha_b - M_ab) dK_ab/dtheta      (GradArgs::beta, gp_kernels.h)
//
// Every sum has a fixed order (per-chunk partial sums, then the chunks in order; no atomics): two calls give the same bytes.
#pragma once

#include "gp_kernels.h"

namespace gphip {

constexpr int LOO_BLK = 64;          // block edge of loo_mirror_scale_kernel (one 64 x 64 block of K^-1 in LDS)
constexpr int LOO_RED = 1024;        // threads of loo_total_kernel: part of the documented summation order of L_LOO

// alpha = U z AND the squared row norms k of U in ONE pass over the upper triangle (both read the same elements; U column-major,
// leading dimension ld, explicit zeros below the diagonal inside the diagonal tiles, tiles below it never read).  Workgroup
// (tile row, chunk of `chunk` columns), thread = row, as utri_gemv_partial_kernel: four independent accumulator pairs keep
// eight loads in flight (that kernel's comment has the latency figures).  part_a / part_k: [chunk][npad].
template <typename T>
__global__ __launch_bounds__(128) void loo_rownorm_partial_kernel(const T* __restrict__ U, long ld, const T* __restrict__ z, int npad,
                                                                  int chunk, double* __restrict__ part_a, double* __restrict__ part_k) {
    const int r = blockIdx.x * TB + threadIdx.x;
    const int c1 = min((int)(blockIdx.y + 1) * chunk, npad);
    const int c0 = max((int)blockIdx.y * chunk, (int)(blockIdx.x * TB));
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0;
    int c = c0;
#pragma unroll 2
    for (; c + 4 <= c1; c += 4) {
        const double u0 = (double)U[(long)c * ld + r], u1 = (double)U[(long)(c + 1) * ld + r], u2 = (double)U[(long)(c + 2) * ld + r],
                     u3 = (double)U[(long)(c + 3) * ld + r];
        s0 = __builtin_fma(u0, (double)z[c], s0);
        s1 = __builtin_fma(u1, (double)z[c + 1], s1);
        s2 = __builtin_fma(u2, (double)z[c + 2], s2);
        s3 = __builtin_fma(u3, (double)z[c + 3], s3);
        q0 = __builtin_fma(u0, u0, q0);
        q1 = __builtin_fma(u1, u1, q1);
        q2 = __builtin_fma(u2, u2, q2);
        q3 = __builtin_fma(u3, u3, q3);
    }
    for (; c < c1; ++c) {
        const double u = (double)U[(long)c * ld + r];
        s0 = __builtin_fma(u, (double)z[c], s0);
        q0 = __builtin_fma(u, u, q0);
    }
    part_a[(long)blockIdx.y * npad + r] = (s0 + s1) + (s2 + s3);
    part_k[(long)blockIdx.y * npad + r] = (q0 + q1) + (q2 + q3);
}

// Per training point: the chunks in order -> alpha_i, k_i, then the leave-one-out moments.  Padding rows (i >= n) get zeros.
// out6: [6][npad] doubles = mean, var, logp, g = alpha / k, s = sqrt(1 / k + g^2), k.
template <typename T>
__global__ void loo_moments_kernel(const double* __restrict__ part_a, const double* __restrict__ part_k, int nchunks, int npad, int n,
                                   const T* __restrict__ y, T* __restrict__ alpha, double* __restrict__ out6) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npad) return;
    double a = 0.0, k = 0.0;
    // (row i has no elements in the chunks left of its diagonal tile: those partial sums are stored zeros)
    for (int c = 0; c < nchunks; ++c) {
        a += part_a[(long)c * npad + i];
        k += part_k[(long)c * npad + i];
    }
    // alpha in the handle's arithmetic, as utri_gemv_finish_kernel leaves it: the moments use what the gradient will use
    const T at = (T)a;
    alpha[i] = i < n ? at : (T)0;
    a = (double)at;
    const bool real = i < n;
    const double g = a / k, var = 1.0 / k;
    out6[i] = real ? (double)y[i] - g : 0.0;
    out6[(long)npad + i] = real ? var : 0.0;
    out6[2l * npad + i] = real ? 0.5 * log(k) - 0.5 * a * g - 0.91893853320467274178 : 0.0;
    out6[3l * npad + i] = real ? g : 0.0;
    out6[4l * npad + i] = real ? sqrt(var + g * g) : 0.0;
    out6[5l * npad + i] = real ? k : 0.0;
}

// L_LOO = sum of logp[0 .. n) in a fixed, documented order (include/gphip.h): thread t of 1024 adds the elements t, t + 1024, ..
// in that order, then a binary tree p[t] += p[t + off], off = 512, 256, .. 1.
__global__ __launch_bounds__(LOO_RED) void loo_total_kernel(const double* __restrict__ logp, int n, double* __restrict__ out) {
    __shared__ double s[LOO_RED];
    const int tid = threadIdx.x;
    double v = 0.0;
    for (int i = tid; i < n; i += LOO_RED) v += logp[i];
    s[tid] = v;
    __syncthreads();
    for (int off = LOO_RED / 2; off > 0; off >>= 1) {
        if (tid < off) s[tid] += s[tid + off];
        __syncthreads();
    }
    if (tid == 0) out[0] = s[0];
}

// K^-1 (lower 128-tiles valid, column-major, leading dimension ld) -> B = K^-1 diag(s) as a FULL matrix, in place, and the
// per-chunk partial sums of beta = K^-1 g from the same pass.  One 64 x 64 block (bi >= bj) per workgroup, held in LDS:
//   lower block (bi, bj)  <- v(r, c) s[col],      upper block (bj, bi) <- v(r, c) s[row of the lower block]   (the mirror)
//   part[bj][rows of bi]  = sum_c v(r, c) g[bj 64 + c],     part[bi][rows of bj] = sum_r v(r, c) g[bi 64 + r]   (bi > bj)
// so every (chunk, row block) pair is written exactly once and beta needs no second read of K^-1.  Diagonal blocks take their
// lower elements as the truth (v(r, c) = v(c, r) for r < c).  No workgroup reads what another writes: only lower blocks are read.
template <typename T>
__global__ __launch_bounds__(256) void loo_mirror_scale_kernel(T* __restrict__ Kv, long ld, int npad, const double* __restrict__ s,
                                                               const double* __restrict__ g, double* __restrict__ part) {
    __shared__ T t[LOO_BLK][LOO_BLK + 1];                 // t[c][r]
    __shared__ double gs[2][LOO_BLK], ss[2][LOO_BLK];     // [0]: columns (block bj), [1]: rows (block bi)
    const int bi = blockIdx.x, bj = blockIdx.y, tid = threadIdx.x;
    if (bj > bi) return;
    const int lane = tid & 63, q0 = tid >> 6;
    const long r0 = (long)bi * LOO_BLK, c0 = (long)bj * LOO_BLK;
    for (int c = q0; c < LOO_BLK; c += 4) t[c][lane] = Kv[(c0 + c) * ld + r0 + lane];
    if (tid < 64) { gs[0][tid] = g[c0 + tid]; ss[0][tid] = s[c0 + tid]; }
    else if (tid < 128) { gs[1][tid - 64] = g[r0 + tid - 64]; ss[1][tid - 64] = s[r0 + tid - 64]; }
    __syncthreads();
    const bool diag = bi == bj;
    auto v = [&](int r, int c) -> double { return (double)((diag && r < c) ? t[r][c] : t[c][r]); };
    // lower block, scaled by its columns' s (lane = row: coalesced along the column)
    for (int c = q0; c < LOO_BLK; c += 4) Kv[(c0 + c) * ld + r0 + lane] = (T)(v(lane, c) * ss[0][c]);
    // its mirror: element (row c0 + c, column r0 + r) = v(r, c) s[r0 + r]  (lane = c: coalesced along the column r0 + r)
    if (!diag)
        for (int r = q0; r < LOO_BLK; r += 4) Kv[(r0 + r) * ld + c0 + lane] = (T)(v(r, lane) * ss[1][r]);
    if (tid < 64) {
        double acc = 0.0;
        for (int c = 0; c < LOO_BLK; ++c) acc = __builtin_fma(v(lane, c), gs[0][c], acc);
        part[(long)bj * npad + r0 + lane] = acc;
    } else if (tid < 128 && !diag) {
        double acc = 0.0;
        for (int r = 0; r < LOO_BLK; ++r) acc = __builtin_fma(v(r, lane), gs[1][r], acc);
        part[(long)bi * npad + c0 + lane] = acc;
    }
}

}  // namespace gphip
