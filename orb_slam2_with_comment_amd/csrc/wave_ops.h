// Wave-level cross-lane primitives for gfx950 (wave64), the one home of the reductions and scans
// of every kernel: DPP moves inside a row of 16 lanes (quad perms, half-row mirror, row rotate by
// 8), v_permlane16/32_swap across rows and readlane for row totals.  Every step is a VALU move with
// no LDS round trip (a __shfl_xor butterfly is one ds_bpermute per step and dword) and every lane
// ends with the result.  The integer / min / max reductions have no order; every floating-point
// sum has a fixed one.
#pragma once
#include <hip/hip_runtime.h>

namespace orbmi {

constexpr int kDppXor1 = 0xB1;         // quad_perm [1,0,3,2]
constexpr int kDppXor2 = 0x4E;         // quad_perm [2,3,0,1]
constexpr int kDppHalfMirror = 0x141;  // lane i <-> 7-i within 8 (pairs lane bit 2 clear/set)
constexpr int kDppRor8 = 0x128;        // row_ror:8 = lane i <-> i^8 within 16

// the row moves: the value of the lane that CTRL names inside the own row of 16 lanes
template <int CTRL>
__device__ inline unsigned dpp_mov_u32(unsigned v) {
    return __builtin_amdgcn_update_dpp(0u, v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ inline unsigned long long dpp_mov_u64(unsigned long long u) {
    const unsigned lo = dpp_mov_u32<CTRL>((unsigned)u), hi = dpp_mov_u32<CTRL>((unsigned)(u >> 32));
    return (unsigned long long)hi << 32 | lo;
}
template <int CTRL>
__device__ inline double dpp_mov(double v) {
    return __longlong_as_double((long long)dpp_mov_u64<CTRL>((unsigned long long)__double_as_longlong(v)));
}

// v_permlane{16,32}_swap on the dword pair (x, y): across rows, partner = lane ^ W (W = 16 or 32)
template <int W>
__device__ inline void permlane_swap(unsigned& x, unsigned& y) {
    static_assert(W == 16 || W == 32, "lane ^ 16 or lane ^ 32");
    if constexpr (W == 32) {
        auto r = __builtin_amdgcn_permlane32_swap(x, y, false, false);
        x = r[0]; y = r[1];
    } else {
        auto r = __builtin_amdgcn_permlane16_swap(x, y, false, false);
        x = r[0]; y = r[1];
    }
}

// the cross-row partners: the value of lane ^ W.  The swap of (v, v) leaves the own value and the
// partner's, in an order that depends on the lane; the one that differs from the own is the
// partner's (equal values: either), which is all that a sum, a minimum or a maximum needs
template <int W>
__device__ inline unsigned swap_partner_u32(unsigned v) {
    unsigned x = v, y = v;
    permlane_swap<W>(x, y);
    return x == v ? y : x;
}
template <int W>
__device__ inline unsigned long long swap_partner_u64(unsigned long long u) {
    unsigned xl = (unsigned)u, xh = (unsigned)(u >> 32), yl = xl, yh = xh;
    permlane_swap<W>(xl, yl);
    permlane_swap<W>(xh, yh);
    const unsigned long long a = (unsigned long long)xh << 32 | xl, b = (unsigned long long)yh << 32 | yl;
    return a == u ? b : a;
}

// the swap on (a, b): lanes with the bit clear end with a_own + a_partner, lanes with it set with
// b_partner + b_own
template <int W>
__device__ inline double swap_combine(double a, double b) {
    const unsigned long long ua = (unsigned long long)__double_as_longlong(a);
    const unsigned long long ub = (unsigned long long)__double_as_longlong(b);
    unsigned xl = (unsigned)ua, xh = (unsigned)(ua >> 32), yl = (unsigned)ub, yh = (unsigned)(ub >> 32);
    permlane_swap<W>(xl, yl);
    permlane_swap<W>(xh, yh);
    const double nx = __longlong_as_double((long long)(((unsigned long long)xh << 32) | xl));
    const double ny = __longlong_as_double((long long)(((unsigned long long)yh << 32) | yl));
    return nx + ny;
}

// one reduce-scatter step inside a row: lanes with `upper` keep b, the others a, each adding
// the partner's copy of what it keeps
template <int CTRL>
__device__ inline double dpp_combine(double a, double b, bool upper) {
    const double recv = dpp_mov<CTRL>(upper ? a : b);
    return (upper ? b : a) + recv;
}

// Reduce-scatter of 32 per-lane values over the wave: afterwards lane l holds the wave sum of
// value l >> 1 (32 exchanges instead of 6 per value)
__device__ inline double wave_reduce_scatter32(double (&v)[32]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < 16; j++) v[j] = swap_combine<32>(v[j], v[16 + j]);
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = swap_combine<16>(v[j], v[8 + j]);
#pragma unroll
    for (int j = 0; j < 4; j++) v[j] = dpp_combine<kDppRor8>(v[j], v[4 + j], lane & 8);
#pragma unroll
    for (int j = 0; j < 2; j++) v[j] = dpp_combine<kDppHalfMirror>(v[j], v[2 + j], lane & 4);
    v[0] = dpp_combine<kDppXor2>(v[0], v[1], lane & 2);
    return v[0] + dpp_mov<kDppXor1>(v[0]);
}

// minimum of a u64 key over the G lanes of a group (G a power of two, groups aligned to G lanes;
// every lane ends with it): G = 8 and 16 stay inside a DPP row, G = 64 (the wave) goes on across
// the rows, G = 1 is the value itself, the other sizes shuffle
template <int G>
__device__ inline unsigned long long group_min_u64(unsigned long long v) {
    static_assert(G >= 1 && G <= 64 && (G & (G - 1)) == 0, "a power of two up to the wave");
    unsigned long long w;
    if constexpr (G == 8 || G == 16 || G == 64) {
        w = dpp_mov_u64<kDppXor1>(v); v = w < v ? w : v;
        w = dpp_mov_u64<kDppXor2>(v); v = w < v ? w : v;
        w = dpp_mov_u64<kDppHalfMirror>(v); v = w < v ? w : v;
        if constexpr (G >= 16) { w = dpp_mov_u64<kDppRor8>(v); v = w < v ? w : v; }
        if constexpr (G == 64) {
            w = swap_partner_u64<16>(v); v = w < v ? w : v;
            w = swap_partner_u64<32>(v); v = w < v ? w : v;
        }
    } else {
#pragma unroll
        for (int o = G / 2; o > 0; o >>= 1) {
            w = __shfl_xor(v, o, G);
            v = w < v ? w : v;
        }
    }
    return v;
}

// wave minimum of a u64 key
__device__ inline unsigned long long wave_min_u64(unsigned long long v) { return group_min_u64<64>(v); }

// wave maximum of a u32 key
__device__ inline unsigned wave_max_u32(unsigned v) {
    unsigned w;
    w = dpp_mov_u32<kDppXor1>(v); v = w > v ? w : v;
    w = dpp_mov_u32<kDppXor2>(v); v = w > v ? w : v;
    w = dpp_mov_u32<kDppHalfMirror>(v); v = w > v ? w : v;
    w = dpp_mov_u32<kDppRor8>(v); v = w > v ? w : v;
    w = swap_partner_u32<16>(v); v = w > v ? w : v;
    w = swap_partner_u32<32>(v); v = w > v ? w : v;
    return v;
}

// wave sum of an int
__device__ inline int wave_sum_i32(int v) {
    v += (int)dpp_mov_u32<kDppXor1>((unsigned)v);
    v += (int)dpp_mov_u32<kDppXor2>((unsigned)v);
    v += (int)dpp_mov_u32<kDppHalfMirror>((unsigned)v);
    v += (int)dpp_mov_u32<kDppRor8>((unsigned)v);
    v += (int)swap_partner_u32<16>((unsigned)v);
    return v + (int)swap_partner_u32<32>((unsigned)v);
}

// Inclusive prefix sum across the 64 lanes: inside each row of 16 lanes by DPP row shifts (a lane
// without a source adds 0), then the totals of the rows before by readlane
__device__ inline int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);  // row_shr:8
    const int t0 = __builtin_amdgcn_readlane(v, 15), t1 = __builtin_amdgcn_readlane(v, 31);
    const int t2 = __builtin_amdgcn_readlane(v, 47);
    const int row = lane >> 4;
    return v + (row > 0 ? t0 : 0) + (row > 1 ? t1 : 0) + (row > 2 ? t2 : 0);
}

// Block-wide exclusive scan of one int per thread; `scratch` holds >= blockDim/64 + 1 ints.
// Returns the exclusive prefix; *total receives the block sum.  Contains __syncthreads().
__device__ inline int block_excl_scan(int v, int* scratch, int* total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    const int incl = wave_incl_scan(v);
    if (lane == 63) scratch[wid] = incl;
    __syncthreads();
    // every thread adds up the wave totals itself (broadcast LDS reads, no serial pass)
    int before = 0, all = 0;
    for (int w = 0; w < nw; w++) {
        const int t = scratch[w];
        before += w < wid ? t : 0;
        all += t;
    }
    *total = all;
    __syncthreads();  // scratch may be rewritten by the next scan
    return before + incl - v;
}

// *counter += the number of active lanes with flag set, as one atomic per wave (a counter shared
// by the whole grid serialises per-thread atomics; an integer sum has no order).  A null counter
// counts nothing.
__device__ inline void wave_count_add(int* counter, bool flag) {
    const unsigned long long m = __ballot(flag);
    if (counter && flag && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(counter, (int)__popcll(m));
}

// all-reduce of one value over the wave (every lane ends with the same sum: each step adds the
// partner's value, and a + b == b + a)
__device__ inline double wave_sum(double v) {
    v += dpp_mov<kDppXor1>(v);
    v += dpp_mov<kDppXor2>(v);
    v += dpp_mov<kDppHalfMirror>(v);
    v += dpp_mov<kDppRor8>(v);
    v = swap_combine<16>(v, v);
    return swap_combine<32>(v, v);
}

__device__ inline double readlane_d(double v, int l) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, l);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), l);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// One value per thread over a workgroup of NT, for the kernels whose sums must not depend on the
// launch: thread t's partial goes into LDS (red: NT doubles), then a halving tree in a fixed order.
// Every thread of the workgroup calls it and ends with the result.  (The headline kernels' block
// sums -- lba.hip's block_sum, pose.hip's pose_reduce -- are other algorithms.)
template <int NT, class Op>
__device__ __forceinline__ double block_reduce_fixed(double part, double* red, Op op) {
    red[threadIdx.x] = part;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = op(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    return red[0];
}
template <int NT>
__device__ __forceinline__ double block_sum_fixed(double part, double* red) {
    return block_reduce_fixed<NT>(part, red, [](double a, double b) { return a + b; });
}
// The sum of n values `stride` apart: thread t adds t, t + NT, ... in that order, then the tree
template <int NT, class Index>
__device__ __forceinline__ double strided_sum_fixed(const double* src, Index n, int stride, double* red) {
    double part = 0;
    for (Index i = threadIdx.x; i < n; i += NT) part = part + src[(size_t)i * stride];
    return block_sum_fixed<NT>(part, red);
}

}  // namespace orbmi
