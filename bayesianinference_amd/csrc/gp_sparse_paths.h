// gp_sparse_paths.h -- device side of gphip_sparse_paths_create (include/gphip.h): the three kernels that
// stand between the feature pass at the inducing points and the substitutions with L_u and L_B.  Included by
// gphip_sparse_paths.inc.  The evaluation kernels are those of the exact object (gp_paths.h, gp_paths_own.h), unchanged.
//
//   sparse_paths_prior_kernel   -(f~_s(z_i) + sqrt(j) zeta_si) into the vector block of the K_uu context; zeta and sqrt(j) zeta kept
//   sparse_paths_rhs_kernel     c_i + sn xi_si into the vector block of B's context, c from B's rhs row; xi kept
//   sparse_paths_join_kernel    the K_uu block += B's block
// All three are one thread per element of a vector block V(s, i) at V[i ld + s] (draw index contiguous, the layout of the
// substitutions), zero for s >= S and i >= m; the random numbers are Philox counters (s, i) under the caller's key.
#pragma once
#include "gp_paths.h"

namespace gphip {

// f~ = the feature pass's strips added in order (part[(q S + s) mpad + i], paths_contract_kernel's layout with one component)
template <typename T>
__global__ __launch_bounds__(256) void sparse_paths_prior_kernel(const double* __restrict__ part, int nstrips, int S, long m, long mpad,
                                                                 double sqrt_j, uint64_t key, double* __restrict__ zeta,
                                                                 double* __restrict__ eps, T* __restrict__ V, long ld) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= mpad * ld) return;
    const long i = e / ld;
    const int s = (int)(e % ld);
    if (i >= m || s >= S) { V[e] = (T)0; return; }
    double f = 0.0;
    for (int q = 0; q < nstrips; ++q) f += part[((long)q * S + s) * mpad + i];
    const double z = philox_normal(key, (uint32_t)s, (uint32_t)i), ep = sqrt_j * z;
    zeta[(long)s * m + i] = z;
    eps[(long)s * m + i] = ep;
    V[e] = (T)(-(f + ep));
}

// A: B's packed workspace after its factorisation, R its tile rows: c = L_B^-1 V r is row 0 of the bordering tile row
// (gather_rhs_row_kernel's address)
template <typename T>
__global__ __launch_bounds__(256) void sparse_paths_rhs_kernel(const T* __restrict__ A, int R, int S, long m, long mpad, double sn,
                                                               uint64_t key, double* __restrict__ xi, T* __restrict__ V, long ld) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= mpad * ld) return;
    const long i = e / ld;
    const int s = (int)(e % ld);
    if (i >= m || s >= S) { V[e] = (T)0; return; }
    const double c = (double)A[tile_index(R - 1, (int)(i >> 7), R) * TS + (long)(i & 127) * TB];
    const double z = philox_normal(key, (uint32_t)s, (uint32_t)i);
    xi[(long)s * m + i] = z;
    V[e] = (T)(c + sn * z);
}

template <typename T>
__global__ __launch_bounds__(256) void sparse_paths_join_kernel(T* __restrict__ Vu, const T* __restrict__ Vb, long n) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long)gridDim.x * 256) Vu[e] += Vb[e];
}

}  // namespace gphip
