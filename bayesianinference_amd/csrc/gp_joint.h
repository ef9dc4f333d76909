// gp_joint.h -- device kernels of the joint predictive path (gphip_predict_cov / _draws / _logpdf, gphip_joint.inc).
//
//   downdate_kernel         C -= [V; z^T] V^T on the lower tiles of a tile-major M x M workspace (the hot path)
//                           (SEG: the two-segment form of the sparse object, C -= V1 V1^T - sn^2 V2 V2^T over a stacked index)
//   downdate_reduce_kernel  C -= sum of the K-strip partials, strips added in a fixed order
//   joint_unpack_kernel     lower tiles -> dense row-major M x M, both triangles (exactly symmetric)
//   joint_rhs_kernel        the workspace's rhs row -> a vector
//   joint_cblock_kernel     the sparse object's rhs-row operand: -c / sn^2 gathered from a factor's rhs tile row
//   joint_normal_kernel     counter-based standard normals (Philox4x32-10, Box-Muller in fp64), keyed by (seed, s, j)
//   joint_trmm_kernel       out = mean + Z L^T with L lower triangular in the tile-major factor
#pragma once
#include "gp_kernels.h"

#include <stdint.h>

namespace gphip {

// ---------------------------------------------------------------------------------------------
// Downdate.  V = L^-1 K(X, X*) is the column-major mpad x Npad block the forward substitution leaves (row t = test point t,
// ld = mpad); Z is a 128 x Npad column-major block (ld = 128) whose row 0 is z = L^-1 r and whose other rows are zero: it is
// the I operand of the workspace's right-hand-side tile row, so that row turns from y* - m(X*) into y* - mu in the same launch.
// One workgroup = one 128 x 128 output tile x one strip of the contraction.  The few output tiles of a typical call (M = 1000:
// 44) cannot fill 256 CUs, so K is split into nsplit strips (grid.y); each strip's product goes to its own partial tile and
// downdate_reduce_kernel adds the strips in order -- no atomics, bit-repeatable.  nsplit = 1 (P null): the accumulators start
// at C and take the negated J fragment, the epilogue is stores only (the trailing-SYRK form of gemm_nt_kernel).
// Staging, MFMA shape and the software pipeline are gemm_nt_kernel's 2 x 2-wave, two-stage form.
//
// SEG (the sparse object's joint prediction, gphip_sparse.inc): the same pipeline over a STACKED contraction index of length
// K = 2 kseg.  V is [V1 | V2], V1 = L_u^-1 k(Z, X*) in columns [0, kseg) and V2 = L_B^-1 V1 in columns [kseg, 2 kseg), and
//     C -= V1 V1^T - sn^2 V2 V2^T,      rhs row -= c^T V2^T
// A stage of GK columns lies in one segment (GK divides 128, kseg is a multiple of 128), so the segment's factor is a
// wave-uniform scalar per stage: the J fragments take s1 in the first segment and s2 in the second -- one VALU multiply per J
// fragment where the plain form has its negation.  The host sets (s1, s2) = (-1, +sn^2) when the accumulators start at C and
// (+1, -sn^2) when the strip's product goes to a partial tile that downdate_reduce_kernel subtracts.  Z then is 128 x 2 kseg
// with row 0 = 0 in the first segment and -c / sn^2 in the second, which serves both signs.  A strip may span the boundary.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct DowndateArgs {
    T* C; int R;                 // workspace (slot 0 base) of R = Mt + 1 tile rows
    const T* V; long ldv;        // V(t, k) at V[t + k ldv]
    const T* Z;                  // 128 x K, ld 128: row 0 = z
    int Mt;                      // tile rows of V
    int ntri;                    // Mt (Mt + 1) / 2: tiles 0 .. ntri-1 = the lower triangle (column-major), then the rhs row's Mt tiles
    int ntiles;                  // ntri + Mt
    int kstrip;                  // contraction columns per strip (multiple of 128)
    int K;                       // contraction length (Npad of the training points)
    T* P;                        // [strip][tile][128 x 128] partial tiles; null: C -= directly
    int kseg;                    // SEG: columns of the first segment
    T s1, s2;                    // SEG: factor of the J fragments in the first / second segment
};

template <typename T>
__device__ __forceinline__ void downdate_tile(int t, int ntri, int Mt, int& ti, int& tj) {
    if (t < ntri) tri_decode(t, Mt, ti, tj);
    else { ti = Mt; tj = t - ntri; }
}

template <typename T, bool SEG = false>
__global__ __launch_bounds__(256, 2) void downdate_kernel(DowndateArgs<T> g) {
    constexpr int FI = 4, FJ = 4;
    extern __shared__ double smem_raw[];
    T* smem = reinterpret_cast<T*>(smem_raw);
    typedef typename Num<T>::acc_t acc_t;
    constexpr int GK = Num<T>::GK;
    constexpr int STAGE = STAGE_BYTES / (int)sizeof(T);
    constexpr int JOFF = STAGE / 2;
    constexpr bool F64 = sizeof(T) == 8;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int uw = __builtin_amdgcn_readfirstlane(wave);
    const int wi = uw & 1, wj = uw >> 1;
    const int t = blockIdx.x, split = blockIdx.y;
    int ti, tj;
    downdate_tile<T>(t, g.ntri, g.Mt, ti, tj);
    ti = __builtin_amdgcn_readfirstlane(ti);
    tj = __builtin_amdgcn_readfirstlane(tj);
    const long k0 = (long)split * g.kstrip;
    const long klen = (g.K - k0 < g.kstrip) ? g.K - k0 : g.kstrip;
    const bool rhs = ti == g.Mt;
    const long lda = rhs ? (long)TB : g.ldv, ldb = g.ldv;
    const T* a_run = rhs ? g.Z + k0 * TB : g.V + (long)ti * TB + k0 * g.ldv;
    const T* b_run = g.V + (long)tj * TB + k0 * g.ldv;
    auto stage = [&](int st) {
        T* Is = smem + st * STAGE;
        T* Js = Is + JOFF;
        const T* Ag = a_run;
        const T* Bg = b_run;
        a_run += (long)GK * lda;
        b_run += (long)GK * ldb;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int q = uw + 4 * s;             // instruction index 0..15 within the stage
            if (F64) {
                __builtin_amdgcn_global_load_lds((glb_void*)(Ag + (long)q * lda + 2 * lane), (lds_void*)(Is + q * LDT), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((glb_void*)(Bg + (long)q * ldb + 2 * lane), (lds_void*)(Js + q * LDT), 16, 0, 0);
            } else {
                const long kcol = 4 * (q >> 1) + (q & 1) + 2 * (lane >> 5);
                const int row = 4 * (lane & 31);
                __builtin_amdgcn_global_load_lds((glb_void*)(Ag + kcol * lda + row), (lds_void*)(Is + q * LDP), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((glb_void*)(Bg + kcol * ldb + row), (lds_void*)(Js + q * LDP), 16, 0, 0);
            }
        }
    };
    const bool direct = g.P == nullptr;
    // lane holds i = wi*64 + y*16 + (lane&15), j = wj*64 + x*16 + drow(lane>>4, r) of the tile (column-major, ld 128)
    const long toff = (long)(wj * 16 * FJ) * TB + wi * (16 * FI) + (lane & 15);
    T* Cg = g.C + tile_index(ti, tj, g.R) * TS + toff;
    T* Pg = direct ? nullptr : g.P + ((long)split * g.ntiles + t) * TS + toff;
    const int l4 = lane >> 4;
    const int nk = (int)(klen / GK);
    // rows this wave computes (wave-uniform): the rhs tile row has ONE real row (the first 16-row group of wave column 0), and
    // nothing reads the strictly-upper 64 x 64 quadrant of a diagonal tile
    int ny = FI;
    if (rhs) ny = wi == 0 ? 1 : 0;
    else if (ti == tj && wi == 0 && wj == 1) ny = 0;
    acc_t acc[FJ][FI];
    auto load_frags = [&](int buf, int kk, T* fi, T* fj) {
        const T* Is = smem + buf * STAGE + wi * (16 * FI) + (lane & 15);
        const T* Js = smem + buf * STAGE + JOFF;
        const int k = 4 * kk + l4;
#pragma unroll
        for (int f = 0; f < FI; ++f) fi[f] = Is[lds_off<T>(k, f * 16)];
#pragma unroll
        for (int f = 0; f < FJ; ++f) fj[f] = Js[lds_off<T>(k, wj * (16 * FJ) + f * 16 + (lane & 15))];
    };
    auto pin_frags = [&](T* fi, T* fj) {
#pragma unroll
        for (int f = 0; f < FI; ++f) asm volatile("" : "+v"(fi[f]));
#pragma unroll
        for (int f = 0; f < FJ; ++f) asm volatile("" : "+v"(fj[f]));
    };
    auto pipeline = [&](auto nyc) {
        constexpr int NY = decltype(nyc)::value;
        constexpr int NKK = GK / 4;
        T sc = g.s1;                      // SEG: the factor of the stage the MFMAs are reading
        auto mfma_block = [&](const T* fi, const T* fj) {
            T nj[FJ];
#pragma unroll
            for (int f = 0; f < FJ; ++f) nj[f] = SEG ? sc * fj[f] : (direct ? -fj[f] : fj[f]);
#pragma unroll
            for (int x = 0; x < FJ; ++x)
#pragma unroll
                for (int y = 0; y < NY; ++y) acc[x][y] = Num<T>::mfma(nj[x], fi[y], acc[x][y]);
        };
        T fa[2][FI], fb[2][FJ];
        stage(0);
#pragma unroll
        for (int x = 0; x < FJ; ++x)
#pragma unroll
            for (int y = 0; y < FI; ++y) {
                if (!direct || y >= NY) {
                    acc[x][y] = (acc_t){0, 0, 0, 0};
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[x][y][r] = Cg[(long)(x * 16 + Num<T>::drow(l4, r)) * TB + y * 16];
                }
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (NY > 0) load_frags(0, 0, fa[0], fb[0]);
        for (int kb = 0; kb < nk; ++kb) {
            const int cur = kb & 1;
            if (kb + 1 < nk) stage(cur ^ 1);
            if (SEG) sc = k0 + (long)kb * GK < g.kseg ? g.s1 : g.s2;
            if (NY > 0) {
#pragma unroll
                for (int kk = 0; kk + 1 < NKK; ++kk) {
                    pin_frags(fa[kk & 1], fb[kk & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                    load_frags(cur, kk + 1, fa[(kk + 1) & 1], fb[(kk + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_block(fa[kk & 1], fb[kk & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                }
                pin_frags(fa[(NKK - 1) & 1], fb[(NKK - 1) & 1]);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (NY > 0) {
                if (kb + 1 < nk) load_frags(cur ^ 1, 0, fa[0], fb[0]);
                __builtin_amdgcn_sched_barrier(0);
                mfma_block(fa[(NKK - 1) & 1], fb[(NKK - 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        T* out = direct ? Cg : Pg;
#pragma unroll
        for (int x = 0; x < FJ; ++x)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                T* cp = out + (long)(x * 16 + Num<T>::drow(l4, r)) * TB;
#pragma unroll
                for (int y = 0; y < NY; ++y) cp[y * 16] = acc[x][y][r];
            }
    };
    if (ny == FI) pipeline(std::integral_constant<int, FI>{});
    else if (ny == 1) pipeline(std::integral_constant<int, 1>{});
    else pipeline(std::integral_constant<int, 0>{});
}

// C -= P[0] + P[1] + .. + P[nsplit-1], elementwise, strips in order (fp64 sums).  grid = (ntiles, 16), 256 threads x 4 elements.
// Only what downdate_kernel wrote: the first 16 rows of an rhs tile, a diagonal tile without its strictly-upper quadrant.
template <typename T>
__global__ __launch_bounds__(256) void downdate_reduce_kernel(T* __restrict__ C, int R, int ntri, int Mt, int ntiles,
                                                              const T* __restrict__ P, int nsplit) {
    const int t = blockIdx.x;
    int ti, tj;
    downdate_tile<T>(t, ntri, Mt, ti, tj);
    T* Ct = C + tile_index(ti, tj, R) * TS;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = (blockIdx.y * 4 + u) * 256 + threadIdx.x;          // element of the tile: row e % 128, column e / 128
        const int i = e & 127, j = e >> 7;
        if (ti == Mt && i >= 16) continue;
        if (ti == tj && i < 64 && j >= 64) continue;
        double s = 0.0;
        for (int q = 0; q < nsplit; ++q) s += (double)P[((long)q * ntiles + t) * TS + e];
        Ct[e] = (T)((double)Ct[e] - s);
    }
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
__host__ __device__ inline double philox_normal(uint64_t seed, uint32_t s, uint32_t j) {
    uint32_t c0 = j, c1 = s, c2 = 0x4A4F494Eu, c3 = 0u;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const uint64_t a = (((uint64_t)c0 << 32) | c1) >> 11, b = (((uint64_t)c2 << 32) | c3) >> 11;
    const double u1 = ((double)a + 0.5) * 0x1.0p-53;                 // (0, 1)
    const double u2 = (double)b * 0x1.0p-53;                         // [0, 1)
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
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
