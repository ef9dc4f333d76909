// gp_joint.h -- device kernels of the joint predictive path (gphip_predict_cov / _draws / _logpdf, gphip_joint.inc).
//
//   downdate_kernel         C -= [V; z^T] V^T on the lower tiles of a tile-major M x M workspace (the hot path; gp_contract.h)
//                           (SEG: the two-segment form of the sparse object, C -= V1 V1^T - sn^2 V2 V2^T over a stacked index)
//   joint_unpack_kernel     lower tiles -> dense row-major M x M, both triangles (exactly symmetric)
//   joint_rhs_kernel        the workspace's rhs row -> a vector
//   joint_cblock_kernel     the sparse object's rhs-row operand: -c / sn^2 gathered from a factor's rhs tile row
//   joint_normal_kernel     counter-based standard normals (Philox4x32-10, Box-Muller in fp64), keyed by (seed, s, j)
//   joint_trmm_kernel       out = mean + Z L^T with L lower triangular in the tile-major factor
#pragma once
#include "gp_contract.h"

#include <stdint.h>

namespace gphip {

// ---------------------------------------------------------------------------------------------
// Downdate: strip_contract (gp_contract.h) with the strided-k operands.  V = L^-1 K(X, X*) is the column-major mpad x Npad block
// the forward substitution leaves (row t = test point t, ld = mpad); Z is a 128 x Npad column-major block (ld = 128) whose row 0
// is z = L^-1 r and whose other rows are zero: it is the I operand of the workspace's right-hand-side tile row, so that row
// turns from y* - m(X*) into y* - mu in the same launch.  One slot: the slot strides are zero.
//
// SEG (the sparse object's joint prediction, gphip_sparse.inc): the same over a STACKED contraction index of length
// K = 2 kseg.  V is [V1 | V2], V1 = L_u^-1 k(Z, X*) in columns [0, kseg) and V2 = L_B^-1 V1 in columns [kseg, 2 kseg), and
//     C -= V1 V1^T - sn^2 V2 V2^T,      rhs row -= c^T V2^T
// The J fragments take s1 in the first segment and s2 in the second -- one VALU multiply per J fragment where the plain form
// has its negation.  The host sets (s1, s2) = (-1, +sn^2) when the accumulators start at C and (+1, -sn^2) when the strip's
// product goes to a partial tile that strip_reduce_kernel subtracts.  Z then is 128 x 2 kseg with row 0 = 0 in the first
// segment and -c / sn^2 in the second, which serves both signs.  A strip may span the boundary.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct DowndateArgs : ContractArgs<T> {
    int kseg;                    // SEG: columns of the first segment
    T s1, s2;                    // SEG: factor of the J fragments in the first / second segment
};

template <typename T, bool SEG = false>
__global__ __launch_bounds__(256, 2) void downdate_kernel(DowndateArgs<T> g) {
    if constexpr (SEG) strip_contract<T>(g, StridedK<T>{}, JSegment<T>(g.kseg, g.s1, g.s2));
    else strip_contract<T>(g, StridedK<T>{}, JNegate<T>{});
}

// dense row-major out[i * M + j] = C(max(i, j), min(i, j)): both triangles read the same element
template <typename T>
__global__ __launch_bounds__(256) void joint_unpack_kernel(const T* __restrict__ C, int R, int M, double* __restrict__ out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)M * M) return;
    const int i = (int)(e / M), j = (int)(e % M);
    const int a = i >= j ? i : j, b = i >= j ? j : i;
    out[e] = (double)C[tile_index(a >> 7, b >> 7, R) * TS + (long)(b & 127) * TB + (a & 127)];
}

// out[j] = (ystar ? ystar[j] : 0) - rhs(j), j < M: with the rhs row at y* - mu this is mu (ystar null, y* = 0)
template <typename T>
__global__ void joint_rhs_kernel(const T* __restrict__ C, int R, int M, const double* __restrict__ ystar, double* __restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    const double r = (double)C[tile_index(R - 1, j >> 7, R) * TS + (long)(j & 127) * TB];
    out[j] = (ystar ? ystar[j] : 0.0) - r;
}

// The sparse object's rhs-row operand: out[(k0 + j) * 128] = -c_j / sn2, j < npad, with c in row 0 of the rhs tile row of the
// tile-major factor A (R tile rows).  out is a zeroed 128 x (k0 + npad) column-major block (ld 128).
template <typename T>
__global__ void joint_cblock_kernel(const T* __restrict__ A, int R, int npad, double sn2, T* __restrict__ out, long k0) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < npad) out[(k0 + j) * TB] = (T)(-(double)A[tile_index(R - 1, j >> 7, R) * TS + (long)(j & 127) * TB] / sn2);
}

// ---------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11), counter (j, s, 0x4A4F494E, 0), key = the 64-bit seed: one standard normal per
// (seed, s, j) by Box-Muller from two 53-bit uniforms.  Nothing depends on how a call is chunked or tiled.
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline void philox_words(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t* out) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__host__ __device__ inline double philox_normal(uint64_t seed, uint32_t s, uint32_t j) {
    uint32_t c[4];
    philox_words(seed, j, s, 0x4A4F494Eu, 0u, c);
    const uint64_t a = (((uint64_t)c[0] << 32) | c[1]) >> 11, b = (((uint64_t)c[2] << 32) | c[3]) >> 11;
    const double u1 = ((double)a + 0.5) * 0x1.0p-53;                 // (0, 1)
    const double u2 = (double)b * 0x1.0p-53;                         // [0, 1)
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
}
// a uniform on [0, 1) with 32 bits from the same counter space, third counter word 0x554E4946 ("UNIF"): never a normal's counter
__host__ __device__ inline double philox_uniform(uint64_t seed, uint32_t s, uint32_t j) {
    uint32_t c[4];
    philox_words(seed, j, s, 0x554E4946u, 0u, c);
    return (double)c[0] * 0x1.0p-32;
}

// Z[s][j] (ld ldz) for the draws s0 .. s0 + S - 1 of the call, j < M; zero for M <= j < ldz
__global__ __launch_bounds__(256) void joint_normal_kernel(double* __restrict__ Z, long ldz, int S, int M, int s0, uint64_t seed) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)S * ldz) return;
    const int s = (int)(e / ldz), j = (int)(e % ldz);
    Z[e] = j < M ? philox_normal(seed, (uint32_t)(s0 + s), (uint32_t)j) : 0.0;
}

// out[s][i] = mean[i] + sum_{j <= i} L(i, j) Z[s][j], i < M.  L: lower triangle of the tile-major factor (upper parts of the
// diagonal tiles ignored).  One workgroup = 64 draws x 64 points, j in blocks of 32 ascending (a fixed order: fp64 sums).
constexpr int JT_B = 64, JT_K = 32;
template <typename T>
__global__ __launch_bounds__(256) void joint_trmm_kernel(const T* __restrict__ L, int R, int M, const double* __restrict__ Z, long ldz,
                                                         int S, const double* __restrict__ mean, double* __restrict__ out, long ldo) {
    __shared__ double Ls[JT_K][JT_B + 1];      // [j][i]
    __shared__ double Zs[JT_K][JT_B + 1];      // [j][s]
    const int tid = threadIdx.x;
    const int i0 = blockIdx.x * JT_B, s0 = blockIdx.y * JT_B;
    const int tx = tid & 15, ty = tid >> 4;    // points i0 + tx + 16 a, draws s0 + ty + 16 b
    double acc[4][4] = {};
    const int jend = (i0 + JT_B < M) ? i0 + JT_B : M;
    for (int j0 = 0; j0 < jend; j0 += JT_K) {
        for (int e = tid; e < JT_K * JT_B; e += 256) {
            const int ii = e & (JT_B - 1), jj = e >> 6;            // i fastest: contiguous inside a tile column
            const int i = i0 + ii, j = j0 + jj;
            double v = 0.0;
            if (i < M && j < M && j <= i) v = (double)L[tile_index(i >> 7, j >> 7, R) * TS + (long)(j & 127) * TB + (i & 127)];
            Ls[jj][ii] = v;
            const int ss = e / JT_K, jz = e % JT_K;                 // j fastest: contiguous in a row of Z
            const int s = s0 + ss, j2 = j0 + jz;
            Zs[jz][ss] = (s < S && j2 < M) ? Z[(long)s * ldz + j2] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < JT_K; ++k) {
            double lv[4], zv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) lv[a] = Ls[k][tx + 16 * a];
#pragma unroll
            for (int b = 0; b < 4; ++b) zv[b] = Zs[k][ty + 16 * b];
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int a = 0; a < 4; ++a) acc[b][a] = __builtin_fma(lv[a], zv[b], acc[b][a]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int i = i0 + tx + 16 * a, s = s0 + ty + 16 * b;
            if (i < M && s < S) out[(long)s * ldo + i] = mean[i] + acc[b][a];
        }
}

}  // namespace gphip
