// gp_contract.h -- the strip-split tile contraction that the joint downdate (gp_joint.h) and the sparse accumulation
// (gp_sparse.h) share.  Not part of gp_kernels.h: that file's text is embedded into every run-time compiled kernel.
//
//   strip_contract       device skeleton: one 128 x 128 output tile x one strip of the contraction index per workgroup
//   StridedK / SwizzledK operand policies: the contraction index is the strided / the contiguous one of the operands
//   JNegate / JSegment / JIdentity / JWeight    what a J fragment takes before the MFMA
//   strip_reduce_kernel  C -/+= the strip partials, strips added in a fixed order
//   strip_split          host: how many strips a launch is cut into
#pragma once
#include "gp_kernels.h"

#include <algorithm>
#include <type_traits>

namespace gphip {

// ---------------------------------------------------------------------------------------------
// The output is the lower tiles plus an rhs tile row of a tile-major workspace of R = Mt + 1 tile rows: tile t of the list is
// lower-triangle tile t (column-major) for t < ntri, then the rhs row's Mt tiles.  Tile (ti, tj) takes the product of the I
// operand's tile row ti with the J operand's tile row tj over the contraction index k; both are tile rows of V, except that
// the rhs row's I operand is the thin block Z whose row 0 is the only one that is not zero.
// One workgroup = one tile x one strip of k (grid = (ntiles, nsplit, slots)).  The few tiles of a typical call cannot fill
// 256 CUs, so k is cut into nsplit strips of kstrip; each strip's product goes to its own partial tile of P and
// strip_reduce_kernel adds the strips in order -- no atomics, bit-repeatable.  nsplit = 1 (P null): the accumulators start at C
// and the epilogue is stores only.  2 x 2 waves of 64 x 64, 4 x 4 accumulators of 16 x 16 x 4 MFMA per wave, two LDS stages
// filled by LDS-DMA: gemm_nt_kernel's two-stage software pipeline.
// Thin tiles: an rhs tile has ONE real row, so only its first 16-row group is computed, and nothing reads the strictly-upper
// 64 x 64 quadrant of a diagonal tile.  What is not computed is not stored either: thin_skip() is the one statement of the rule.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct ContractArgs {
    T* C; int R;                 // workspace (slot 0 base) of R = Mt + 1 tile rows
    const T* V; long ldv;        // the operand block (slot 0 base), column-major with leading dimension ldv
    const T* Z;                  // I operand of the rhs tile row (slot 0 base); its layout is the operand policy's
    int Mt;                      // tile rows of the output
    int ntri;                    // Mt (Mt + 1) / 2
    int ntiles;                  // ntri + Mt
    int kstrip;                  // contraction indices per strip (multiple of 128)
    int K;                       // contraction length (multiple of 128)
    T* P;                        // [strip][tile][128 x 128] partial tiles; null: straight into C
    long c_bstride, v_bstride, z_bstride, p_bstride;      // elements between the slots (blockIdx.z) of C, V, Z and P
};

__device__ __forceinline__ void contract_tile(int t, int ntri, int Mt, int& ti, int& tj) {
    if (t < ntri) tri_decode(t, Mt, ti, tj);
    else { ti = Mt; tj = t - ntri; }
}

// element (i, j) of tile (ti, tj) is neither computed nor stored
__device__ __forceinline__ bool thin_skip(int ti, int tj, int Mt, int i, int j) {
    return (ti == Mt && i >= 16) || (ti == tj && i < 64 && j >= 64);
}

// a lane's place: lane of the wave, wave of the workgroup (uniform) and the wave's 64 x 64 quarter (rows wi, columns wj) of the tile
struct WavePos { int lane, uw, wi, wj, l4, l15; };

// ---------------------------------------------------------------------------------------------
// Operand policy, strided k: V(t, k) at V[t + k ldv] with t the OUTPUT index, Z a 128 x K column-major block (ld 128).  For one
// k both operands are contiguous in their output index: staging, stage image (LDT / LDP) and fragment offsets are
// gemm_nt_kernel's.  A stacked contraction index ([V1 | V2], gp_joint.h) is this form with a longer K.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct StridedK {
    static constexpr int GK = Num<T>::GK;                  // contraction indices per stage
    static constexpr size_t LDS = 2 * STAGE_BYTES;         // two stages
    static constexpr int STAGE = STAGE_BYTES / (int)sizeof(T), JOFF = STAGE / 2;
    const T *a_run, *b_run;
    long lda, ldb;
    // V, Z: this slot's; (ti, tj), rhs: the workgroup's tile; k0: where its strip starts
    __device__ __forceinline__ void start(const ContractArgs<T>& g, const T* V, const T* Z, int ti, int tj, bool rhs, long k0) {
        lda = rhs ? (long)TB : g.ldv;
        ldb = g.ldv;
        a_run = rhs ? Z + k0 * TB : V + (long)ti * TB + k0 * g.ldv;
        b_run = V + (long)tj * TB + k0 * g.ldv;
    }
    __device__ __forceinline__ void stage(double* lds, int st, const WavePos& w) {
        T* Is = reinterpret_cast<T*>(lds) + st * STAGE;
        T* Js = Is + JOFF;
        const T* Ag = a_run;
        const T* Bg = b_run;
        a_run += (long)GK * lda;
        b_run += (long)GK * ldb;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int q = w.uw + 4 * s;           // instruction index 0..15 within the stage
            if (sizeof(T) == 8) {
                __builtin_amdgcn_global_load_lds((glb_void*)(Ag + (long)q * lda + 2 * w.lane), (lds_void*)(Is + q * LDT), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((glb_void*)(Bg + (long)q * ldb + 2 * w.lane), (lds_void*)(Js + q * LDT), 16, 0, 0);
            } else {
                const long kcol = 4 * (q >> 1) + (q & 1) + 2 * (w.lane >> 5);
                const int row = 4 * (w.lane & 31);
                __builtin_amdgcn_global_load_lds((glb_void*)(Ag + kcol * lda + row), (lds_void*)(Is + q * LDP), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((glb_void*)(Bg + kcol * ldb + row), (lds_void*)(Js + q * LDP), 16, 0, 0);
            }
        }
    }
    __device__ __forceinline__ void load_frags(const double* lds, int buf, int kk, T* fi, T* fj, const WavePos& w) const {
        const T* Is = reinterpret_cast<const T*>(lds) + buf * STAGE + w.wi * 64 + w.l15;
        const T* Js = reinterpret_cast<const T*>(lds) + buf * STAGE + JOFF;
        const int k = 4 * kk + w.l4;
#pragma unroll
        for (int f = 0; f < 4; ++f) fi[f] = Is[lds_off<T>(k, f * 16)];
#pragma unroll
        for (int f = 0; f < 4; ++f) fj[f] = Js[lds_off<T>(k, w.wj * 64 + f * 16 + w.l15)];
    }
};

// ---------------------------------------------------------------------------------------------
// Operand policy, contiguous k: V(k, t) at V[k + t ldv] with t the OUTPUT index, so the contraction index is the CONTIGUOUS one
// of both operands and the output indices are the strided ones: an operand tile of one stage is 128 output rows x 128 bytes of
// consecutive k (16 doubles / 32 floats).  Z is 16 rows x ldz, row-contiguous in k (row 0 the real one, rows 1 .. 15 zero): an rhs
// tile reads the first 16 rows of its I image only, so only the first two DMA instructions of the I operand are issued for it.
// Staging: LDS-DMA, 16 bytes per lane.  A DMA writes LDS lane-linearly, so the stage image is [row][8 chunks of 16 bytes] with
// no room for padding; read as it lies, the 16 rows of an MFMA operand (one element per lane, row = lane & 15, k = lane >> 4)
// would sit 128 bytes apart -- two banks' worth for sixteen lanes.  The image is therefore swizzled: chunk c of row i lies in
// slot c ^ ((i >> 1) & 7) of its row.  The permutation is applied on the SOURCE address of the DMA (lane l of an instruction
// fills slot l & 7 of row l >> 3, so it fetches chunk (l & 7) ^ swz(row); the eight lanes of a row still cover one whole
// 128-byte line) and again on the fragment read.  16 rows x one chunk then cover sixteen different 16-byte groups of the 256
// bytes the banks serve per cycle: the reads are conflict-free in both types (fp64: half a wave reads the two halves of one
// chunk; fp32: the four k of a wave are the four floats of one chunk).
// Which k an MFMA step contracts is the same for both operands, so their order inside a stage is free: step kk takes chunk
// 2 kk + (l4 >> 1), element l4 & 1 (fp64) or chunk kk, element l4 (fp32).
// ---------------------------------------------------------------------------------------------
template <typename T>
struct SwizzledK {
    static constexpr int GK = 128 / (int)sizeof(T);        // contraction indices per stage
    static constexpr int OPND = TB * 128;                  // bytes of one operand image of a stage: 128 rows x 128 bytes
    static constexpr int STAGE = 2 * OPND;
    static constexpr size_t LDS = 2 * STAGE;               // two stages, 64 KiB: two workgroups per CU
    static constexpr int CE = 16 / (int)sizeof(T);         // elements per 16-byte chunk
    long ldz;                                              // leading dimension of Z (the caller's; the rest is set by start())
    const T *a_run, *b_run;
    long lda, ldb;
    bool rhs;
    __device__ __forceinline__ void start(const ContractArgs<T>& g, const T* V, const T* Z, int ti, int tj, bool rhs_, long k0) {
        rhs = rhs_;
        lda = rhs ? ldz : g.ldv;
        ldb = g.ldv;
        a_run = (rhs ? Z : V + (long)ti * TB * g.ldv) + k0;
        b_run = V + (long)tj * TB * g.ldv + k0;
    }
    __device__ __forceinline__ void stage(double* lds, int st, const WavePos& w) {
        char* Is = reinterpret_cast<char*>(lds) + st * STAGE;
        char* Js = Is + OPND;
        const T* Ag = a_run;
        const T* Bg = b_run;
        a_run += GK;
        b_run += GK;
        // this lane's share of a DMA instruction: slot lane & 7 of row lane >> 3 of the instruction's eight rows
        const int lr = w.lane >> 3, lp = w.lane & 7;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int q = w.uw + 4 * s;           // instruction index 0..15 within the stage: rows 8 q .. 8 q + 7
            const int row = 8 * q + lr;
            const int c = lp ^ ((row >> 1) & 7);
            if (!rhs || q < 2)
                __builtin_amdgcn_global_load_lds((glb_void*)(Ag + (long)row * lda + c * CE), (lds_void*)(Is + q * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((glb_void*)(Bg + (long)row * ldb + c * CE), (lds_void*)(Js + q * 1024), 16, 0, 0);
        }
    }
    // byte offset of this lane's element of row (16 f + l15) of a 64-row half, MFMA step kk: the rows' swizzle term is l15 >> 1
    __device__ __forceinline__ static int frag_off(int row, int kk, const WavePos& w) {
        const int c = sizeof(T) == 8 ? 2 * kk + (w.l4 >> 1) : kk, e = sizeof(T) == 8 ? (w.l4 & 1) : w.l4;
        return (row * 8 + (c ^ (w.l15 >> 1))) * 16 + e * (int)sizeof(T);
    }
    __device__ __forceinline__ void load_frags(const double* lds, int buf, int kk, T* fi, T* fj, const WavePos& w) const {
        const char* Is = reinterpret_cast<const char*>(lds) + buf * STAGE;
        const char* Js = Is + OPND;
#pragma unroll
        for (int f = 0; f < 4; ++f) fi[f] = *reinterpret_cast<const T*>(Is + frag_off(w.wi * 64 + f * 16 + w.l15, kk, w));
#pragma unroll
        for (int f = 0; f < 4; ++f) fj[f] = *reinterpret_cast<const T*>(Js + frag_off(w.wj * 64 + f * 16 + w.l15, kk, w));
    }
};

// ---------------------------------------------------------------------------------------------
// J-scale policy: at(k) is called once per stage with the stage's first contraction index, then (*this)(fj, direct, kk) on every J
// fragment of MFMA step kk of the stage (a lane's fragment of step kk is contraction index k + 4 kk + (lane >> 4) in both operand
// policies).  direct: the accumulators started at C (no partial tiles).
// ---------------------------------------------------------------------------------------------
template <typename T>
struct JIdentity {               // C += I J^T
    __device__ __forceinline__ void at(long) {}
    __device__ __forceinline__ T operator()(T fj, bool, int) const { return fj; }
};
template <typename T>
struct JNegate {                 // C -= I J^T: accumulators that start at C take the negated fragment, a partial tile the product itself
    __device__ __forceinline__ void at(long) {}
    __device__ __forceinline__ T operator()(T fj, bool direct, int) const { return direct ? -fj : fj; }
};
template <typename T>
struct JSegment {                // factor s1 for k < kseg, s2 from there on; a stage lies in one segment (GK divides 128 divides kseg)
    int kseg;
    T s1, s2, sc;
    __device__ __forceinline__ JSegment(int kseg_, T s1_, T s2_) : kseg(kseg_), s1(s1_), s2(s2_), sc(s1_) {}
    __device__ __forceinline__ void at(long k) { sc = k < kseg ? s1 : s2; }
    __device__ __forceinline__ T operator()(T fj, bool, int) const { return sc * fj; }
};
// C += I diag(w) J^T: a weight per contraction index, w [kend] in the operands' type (zero where an operand is padding).  A lane
// needs one weight per MFMA step: NKK values per stage, held in registers.  Those of the NEXT stage are requested in at(), next to
// the staging loads of that stage, and the pipeline's wait before its barrier covers them, so no MFMA waits for a weight.
template <typename T, int GK>
struct JWeight {
    static constexpr int NKK = GK / 4;
    const T* w;                  // + (lane >> 4): this lane's weight of step kk of the stage at k is w[k + 4 kk]
    long kend;
    T cur[NKK], nxt[NKK];
    __device__ __forceinline__ void fetch(long k) {
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) nxt[kk] = k < kend ? w[k + 4 * kk] : (T)0;
    }
    // w_: the weights of the workgroup's slot; k0: where its strip starts; kend_: the contraction length (a multiple of GK)
    __device__ __forceinline__ JWeight(const T* w_, long k0, long kend_) : w(w_ + (threadIdx.x >> 4 & 3)), kend(kend_) { fetch(k0); }
    __device__ __forceinline__ void at(long k) {
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) cur[kk] = nxt[kk];
        fetch(k + GK);
    }
    __device__ __forceinline__ T operator()(T fj, bool, int kk) const { return cur[kk] * fj; }
};

template <typename T, class Opnd, class JScale>
__device__ __forceinline__ void strip_contract(const ContractArgs<T>& g, Opnd op, JScale js) {
    constexpr int FI = 4, FJ = 4;
    extern __shared__ double smem_raw[];
    typedef typename Num<T>::acc_t acc_t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int uw = __builtin_amdgcn_readfirstlane(wave);
    const WavePos w{lane, uw, uw & 1, uw >> 1, lane >> 4, lane & 15};
    const int wi = w.wi, wj = w.wj, l4 = w.l4;
    const int t = blockIdx.x, split = blockIdx.y;
    const long slot = blockIdx.z;
    int ti, tj;
    contract_tile(t, g.ntri, g.Mt, ti, tj);
    ti = __builtin_amdgcn_readfirstlane(ti);
    tj = __builtin_amdgcn_readfirstlane(tj);
    const long k0 = (long)split * g.kstrip;
    const long klen = (g.K - k0 < g.kstrip) ? g.K - k0 : g.kstrip;
    op.start(g, g.V + slot * g.v_bstride, g.Z + slot * g.z_bstride, ti, tj, ti == g.Mt, k0);
    constexpr int GK = Opnd::GK;
    const bool direct = g.P == nullptr;
    // lane holds i = wi*64 + y*16 + (lane&15), j = wj*64 + x*16 + drow(lane>>4, r) of the tile (column-major, ld 128)
    const long toff = (long)(wj * 16 * FJ) * TB + wi * (16 * FI) + (lane & 15);
    T* Cg = g.C + slot * g.c_bstride + tile_index(ti, tj, g.R) * TS + toff;
    T* Pg = direct ? nullptr : g.P + slot * g.p_bstride + ((long)split * g.ntiles + t) * TS + toff;
    const int nk = (int)(klen / GK);
    // 16-row groups this wave computes (wave-uniform): thin_skip() holds for a whole group, and the groups kept come first
    int ny = 0;
#pragma unroll
    for (int y = 0; y < FI; ++y) ny += thin_skip(ti, tj, g.Mt, wi * (16 * FI) + y * 16, wj * (16 * FJ)) ? 0 : 1;
    acc_t acc[FJ][FI];
    auto pin_frags = [&](T* fi, T* fj) {
#pragma unroll
        for (int f = 0; f < FI; ++f) asm volatile("" : "+v"(fi[f]));
#pragma unroll
        for (int f = 0; f < FJ; ++f) asm volatile("" : "+v"(fj[f]));
    };
    auto pipeline = [&](auto nyc) {
        constexpr int NY = decltype(nyc)::value;
        constexpr int NKK = GK / 4;
        auto mfma_block = [&](const T* fi, const T* fj, int kk) {
            T nj[FJ];
#pragma unroll
            for (int f = 0; f < FJ; ++f) nj[f] = js(fj[f], direct, kk);
#pragma unroll
            for (int x = 0; x < FJ; ++x)
#pragma unroll
                for (int y = 0; y < NY; ++y) acc[x][y] = Num<T>::mfma(nj[x], fi[y], acc[x][y]);
        };
        T fa[2][FI], fb[2][FJ];
        op.stage(smem_raw, 0, w);
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
        if (NY > 0) op.load_frags(smem_raw, 0, 0, fa[0], fb[0], w);
        for (int kb = 0; kb < nk; ++kb) {
            const int cur = kb & 1;
            if (kb + 1 < nk) op.stage(smem_raw, cur ^ 1, w);
            js.at(k0 + (long)kb * GK);
            if (NY > 0) {
#pragma unroll
                for (int kk = 0; kk + 1 < NKK; ++kk) {
                    pin_frags(fa[kk & 1], fb[kk & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                    op.load_frags(smem_raw, cur, kk + 1, fa[(kk + 1) & 1], fb[(kk + 1) & 1], w);
                    __builtin_amdgcn_sched_barrier(0);
                    mfma_block(fa[kk & 1], fb[kk & 1], kk);
                    __builtin_amdgcn_sched_barrier(0);
                }
                pin_frags(fa[(NKK - 1) & 1], fb[(NKK - 1) & 1]);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (NY > 0) {
                if (kb + 1 < nk) op.load_frags(smem_raw, cur ^ 1, 0, fa[0], fb[0], w);
                __builtin_amdgcn_sched_barrier(0);
                mfma_block(fa[(NKK - 1) & 1], fb[(NKK - 1) & 1], NKK - 1);
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

// C += sign x (P[0] + P[1] + .. + P[nsplit-1]), elementwise, strips in order (fp64 sums), of what strip_contract wrote.
// grid = (ntiles, 16, slots), 256 threads x 4 elements.
template <typename T>
__global__ __launch_bounds__(256) void strip_reduce_kernel(T* __restrict__ C, int R, int ntri, int Mt, int ntiles, const T* __restrict__ P,
                                                           int nsplit, double sign, long c_bstride, long p_bstride) {
    const int t = blockIdx.x;
    C += (long)blockIdx.z * c_bstride;
    P += (long)blockIdx.z * p_bstride;
    int ti, tj;
    contract_tile(t, ntri, Mt, ti, tj);
    T* Ct = C + tile_index(ti, tj, R) * TS;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int e = (blockIdx.y * 4 + u) * 256 + threadIdx.x;          // element of the tile: row e % 128, column e / 128
        if (thin_skip(ti, tj, Mt, e & 127, e >> 7)) continue;
        double s = 0.0;
        for (int q = 0; q < nsplit; ++q) s += (double)P[((long)q * ntiles + t) * TS + e];
        Ct[e] = (T)((double)Ct[e] + sign * s);
    }
}

// Split rule.  wgs: workgroups of the launch without strips (output tiles x slots); kt: 128-tiles of the contraction index.
// While wgs is below two per CU, the contraction is cut into strips of whole tiles so that wgs x strips >= 2 per CU; strips are
// equal but the last.  forced > 0: that many strips, at most kt.  Returns the strips used, *strip_tiles: tiles per strip.
inline int strip_split(long wgs, int kt, int forced, int ncu, int* strip_tiles) {
    const long target = 2l * std::max(ncu, 1);
    int nsplit = wgs >= target ? 1 : (int)std::min<long>(kt, (target + wgs - 1) / wgs);
    if (forced > 0) nsplit = std::min(forced, kt);
    *strip_tiles = (kt + nsplit - 1) / nsplit;
    return (kt + *strip_tiles - 1) / *strip_tiles;
}

}  // namespace gphip
