// gp_extend.h -- the device kernel of gphip_extend (gphip_extend.inc): the factor of the N + M points assembled from parts.
//
//   L' = [ L    0   ]      L, z    the parent's factor and rhs row (tile-major, Rp tile rows)
//        [ V^T  L_S ]      V       = L^-1 k(X, X_new), column-major mpad x Npad as the forward substitution leaves it
//   z' = [ z ; z_new ]     L_S, z_new   the child's factor of Sigma and its rhs row (tile-major, Rc tile rows)
//
// A streaming copy: every element of the new workspace is written exactly once, nothing is computed.
#pragma once
#include "gp_kernels.h"

namespace gphip {

template <typename T>
struct ExtendArgs {
    T* out; int Rn;                 // the new workspace (slot 0): Rn = Nt' + 1 tile rows
    const T* A; int Rp;             // the parent's workspace
    const T* V; long mpad;          // V(t, j) at j * mpad + t
    const T* C; int Rc;             // the child's workspace
    int N, M;                       // old points, new points
};

// 16 bytes of T: what one lane moves per access (a native vector: it lives in four registers, one dwordx4 load / store)
template <typename T> struct ExtPack;
template <> struct ExtPack<double> { typedef double type __attribute__((ext_vector_type(2))); };
template <> struct ExtPack<float> { typedef float type __attribute__((ext_vector_type(4))); };

// element (gi, gj) of a matrix tile row of the new factor
template <typename T>
__device__ __forceinline__ T extend_elem(const ExtendArgs<T>& a, int gi, int gj) {
    const int NM = a.N + a.M;
    if (gi >= NM || gj >= NM) return gi == gj ? (T)1 : (T)0;           // the identity padding of a fresh factorisation
    if (gj > gi && gj >= a.N) return (T)0;                             // strictly upper part of a new diagonal tile: never read
    if (gi < a.N)                                                      // (both below N: the parent's element, either triangle of its tile)
        return a.A[tile_index(gi >> 7, gj >> 7, a.Rp) * TS + (long)(gj & 127) * TB + (gi & 127)];
    if (gj < a.N) return a.V[(long)gj * a.mpad + (gi - a.N)];
    const int ci = gi - a.N, cj = gj - a.N;
    return a.C[tile_index(ci >> 7, cj >> 7, a.Rc) * TS + (long)(cj & 127) * TB + (ci & 127)];
}

// row 0 of the right-hand-side tile row: z, z_new, and in the corner -(z^T z + z_new^T z_new)
template <typename T>
__device__ __forceinline__ T extend_rhs(const ExtendArgs<T>& a, int gj) {
    const int NM = a.N + a.M, np = (a.Rn - 1) * TB;
    if (gj == np)
        return a.A[tile_index(a.Rp - 1, a.Rp - 1, a.Rp) * TS] + a.C[tile_index(a.Rc - 1, a.Rc - 1, a.Rc) * TS];
    if (gj < a.N) return a.A[tile_index(a.Rp - 1, gj >> 7, a.Rp) * TS + (long)(gj & 127) * TB];
    if (gj < NM) return a.C[tile_index(a.Rc - 1, (gj - a.N) >> 7, a.Rc) * TS + (long)((gj - a.N) & 127) * TB];
    return (T)0;
}

// One workgroup per destination tile (grid = Rn (Rn + 1) / 2, column-major packed order).  A lane owns 16 bytes of a tile
// column, a wave 1 KiB of it (fp64: one whole column): every store is a 16-byte store to a 16-byte aligned address.  The loads are
// 16 bytes wherever the source has the destination's alignment: always in the old part (same position of the same tile), in the
// V and L_Sigma parts when N is a multiple of 16 / sizeof(T) (their row offset is N mod 128); element by element otherwise,
// still coalesced (the source's contiguous index is the destination's).
template <typename T>
__global__ __launch_bounds__(256) void extend_assemble_kernel(ExtendArgs<T> a) {
    constexpr int VEC = 16 / (int)sizeof(T), CPC = TB / VEC;           // elements per access, accesses per tile column
    constexpr int NQ = (int)(TS / VEC) / 256;                          // accesses per lane and tile
    typedef typename ExtPack<T>::type pack_t;
    int ti, tj;
    tri_decode((int)blockIdx.x, a.Rn, ti, tj);
    T* dst = a.out + tile_index(ti, tj, a.Rn) * TS;
    const int tid = threadIdx.x;
    if (ti < a.Rn - 1 && (ti + 1) * TB <= a.N) {                       // a tile of old points only: the parent's tile as it is
        const pack_t* src = reinterpret_cast<const pack_t*>(a.A + tile_index(ti, tj, a.Rp) * TS);
        pack_t* d = reinterpret_cast<pack_t*>(dst);
        static_assert(NQ % 8 == 0, "eight accesses in flight per lane");
#pragma unroll 1
        for (int q0 = 0; q0 < NQ; q0 += 8) {
            const pack_t v0 = src[(q0 + 0) * 256 + tid], v1 = src[(q0 + 1) * 256 + tid], v2 = src[(q0 + 2) * 256 + tid],
                         v3 = src[(q0 + 3) * 256 + tid], v4 = src[(q0 + 4) * 256 + tid], v5 = src[(q0 + 5) * 256 + tid],
                         v6 = src[(q0 + 6) * 256 + tid], v7 = src[(q0 + 7) * 256 + tid];
            d[(q0 + 0) * 256 + tid] = v0; d[(q0 + 1) * 256 + tid] = v1; d[(q0 + 2) * 256 + tid] = v2; d[(q0 + 3) * 256 + tid] = v3;
            d[(q0 + 4) * 256 + tid] = v4; d[(q0 + 5) * 256 + tid] = v5; d[(q0 + 6) * 256 + tid] = v6; d[(q0 + 7) * 256 + tid] = v7;
        }
        return;
    }
    const bool rhs = ti == a.Rn - 1;
    const bool al = (a.N % VEC) == 0;
    const int NM = a.N + a.M;
    for (int q = tid; q < (int)(TS / VEC); q += 256) {
        const int c = q / CPC, r0 = (q % CPC) * VEC;
        const int gj = tj * TB + c, gi0 = ti * TB + r0;
        pack_t v;
        const T* src = nullptr;                                       // a 16-byte aligned run of VEC source elements, where there is one
        if (!rhs) {
            if (gi0 + VEC <= a.N && gj < a.N)
                src = a.A + tile_index(ti, tj, a.Rp) * TS + (long)c * TB + r0;
            else if (al && gi0 >= a.N && gi0 + VEC <= NM && gj < a.N)
                src = a.V + (long)gj * a.mpad + (gi0 - a.N);
            else if (al && gi0 >= a.N && gi0 + VEC <= NM && gj >= a.N && gj <= gi0) {
                const int ci = gi0 - a.N, cj = gj - a.N;
                src = a.C + tile_index(ci >> 7, cj >> 7, a.Rc) * TS + (long)(cj & 127) * TB + (ci & 127);
            }
        }
        if (src) {
            v = *reinterpret_cast<const pack_t*>(src);
        } else if (rhs) {
            v = (pack_t)(T)0;
            if (r0 == 0) v[0] = extend_rhs<T>(a, gj);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = extend_elem<T>(a, gi0 + e, gj);
        }
        *reinterpret_cast<pack_t*>(dst + (long)c * TB + r0) = v;
    }
}

}  // namespace gphip
