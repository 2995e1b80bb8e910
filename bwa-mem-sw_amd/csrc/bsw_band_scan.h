/*
 * bsw_band_scan.h — the parts every wave-per-alignment kernel of the int32 family is built from (bsw_wave_kernel.hip,
 * bsw_long_kernel.hip, bsw_global_kernel.hip, bsw_global_long_kernel.hip, bsw_align_kernel.hip, bsw_align_long_kernel.hip), each
 * stated once: the DPP move and the inclusive 64-lane max-scan behind the F recurrence, the maximum over a 16- or 8-lane group,
 * the packed-base decode, the target stream, the 5x5 matrix as packed columns, and the launchers' per-device dynamic-LDS limit.
 * State is passed by reference and everything is inlined: a kernel compiles to what it did with its own copy.
 * (The four-seeds-per-wavefront and the lane kernels keep their own DPP code: bsw_quad_kernel.hip has its wait-state reasoning.)
 */
#pragma once

#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <atomic>

#include "bsw_device.h"

namespace bsw {
namespace {

template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf>
__device__ __forceinline__ int dpp_mov(int old, int src)
{
    return __builtin_amdgcn_update_dpp(old, src, CTRL, ROW_MASK, BANK_MASK, false);
}

/* inclusive max-scan over the 64 lanes (row_shr 1,2,4,8 + row_bcast 15/31); IDENT: at or below every input */
template <int IDENT = INT_MIN>
__device__ __forceinline__ int wave_scan_max(int x)
{
    x = max(x, dpp_mov<0x111>(IDENT, x));
    x = max(x, dpp_mov<0x112>(IDENT, x));
    x = max(x, dpp_mov<0x114>(IDENT, x));
    x = max(x, dpp_mov<0x118>(IDENT, x));
    x = max(x, dpp_mov<0x142, 0xa>(IDENT, x));
    x = max(x, dpp_mov<0x143, 0xc>(IDENT, x));
    return x;
}

/* max over the GW (16 or 8) lanes of a group, in every lane: (mirror,) half mirror, two quad permutes */
template <int GW>
__device__ __forceinline__ int group_max(int v)
{
    if (GW == 16) v = max(v, dpp_mov<0x140>(INT_MIN, v));   /* row_mirror      */
    v = max(v, dpp_mov<0x141>(INT_MIN, v));                 /* row_half_mirror */
    v = max(v, dpp_mov<0x4e>(INT_MIN, v));                  /* quad_perm [2,3,0,1] */
    v = max(v, dpp_mov<0xb1>(INT_MIN, v));                  /* quad_perm [1,0,3,2] */
    return v;
}
template <int GW>
__device__ __forceinline__ unsigned long long group_max_u64(unsigned long long v)
{
    /* two 32-bit butterflies would not keep (hi, lo) together: compare as 64 bits after moving both halves */
    for (int s = GW == 16 ? 0 : 1; s < 4; ++s) {
        int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32), lo2, hi2;
        switch (s) {
        case 0: lo2 = dpp_mov<0x140>(0, lo); hi2 = dpp_mov<0x140>(0, hi); break;
        case 1: lo2 = dpp_mov<0x141>(0, lo); hi2 = dpp_mov<0x141>(0, hi); break;
        case 2: lo2 = dpp_mov<0x4e>(0, lo); hi2 = dpp_mov<0x4e>(0, hi); break;
        default: lo2 = dpp_mov<0xb1>(0, lo); hi2 = dpp_mov<0xb1>(0, hi); break;
        }
        const unsigned long long o = ((unsigned long long)(uint32_t)hi2 << 32) | (uint32_t)lo2;
        v = o > v ? o : v;
    }
    return v;
}

/* does pred hold in any lane of this lane's group of GW (thread tid of the workgroup)?  Every lane of the wavefront calls it. */
template <int GW>
__device__ __forceinline__ bool group_any(const bool pred, const int tid)
{
    const unsigned long long m = __builtin_amdgcn_ballot_w64(pred);
    return ((m >> (tid & (64 - GW))) & (GW == 16 ? 0xffffull : 0xffull)) != 0;
}

/* base idx of a packed sequence (16 bases of 4 bits per word), codes above 4 read as N; w = the word that holds it */
__device__ __forceinline__ int base_code(uint64_t w, int idx)
{
    const int c = (int)((w >> ((idx & 15) * 4)) & 7ull);
    return c > 4 ? 4 : c;
}
__device__ __forceinline__ int base_at(const uint64_t *__restrict__ seq, uint32_t off, int idx)
{
    return base_code(seq[off + (uint32_t)(idx >> 4)], idx);
}

/* The target stream of a row loop: base i of the ntw-word target at seq + t_off, for i = 0, 1, 2, ... in turn.  Lane l holds
 * packed word l of a 1024-base chunk (twl / twh, one coalesced load per 1024 rows), every 16 rows one word is broadcast with a
 * readlane pair (cur_lo / cur_hi); the four are the caller's, zero before row 0. */
__device__ __forceinline__ int target_base(const uint64_t *__restrict__ seq, const uint32_t t_off, const int ntw, const int i,
                                           const int lane, uint32_t &twl, uint32_t &twh, uint32_t &cur_lo, uint32_t &cur_hi)
{
    if ((i & 1023) == 0) {                                  /* coalesced refill: 64 words = 1024 target bases */
        const int wi = (i >> 4) + lane;
        const uint64_t tv = wi < ntw ? seq[t_off + wi] : 0ull;
        twl = (uint32_t)tv;
        twh = (uint32_t)(tv >> 32);
    }
    if ((i & 15) == 0) {
        const int src = (i >> 4) & 63;
        cur_lo = __builtin_amdgcn_readlane(twl, src);
        cur_hi = __builtin_amdgcn_readlane(twh, src);
    }
    const int ti = (int)((((i & 8) ? cur_hi : cur_lo) >> ((i & 7) * 4)) & 7);
    return ti < 4 ? ti : 4;
}

/* The 5x5 matrix by query base q (0 .. 4): the scores of target bases ACGT packed 4 x int8 (lo) and of a target N (hi) */
__device__ __forceinline__ void matrix_column(const bsw_dparams &P, const int q, uint32_t &lo, int &hi)
{
    lo = (uint32_t)(uint8_t)P.mat[q] | ((uint32_t)(uint8_t)P.mat[5 + q] << 8) |
         ((uint32_t)(uint8_t)P.mat[10 + q] << 16) | ((uint32_t)(uint8_t)P.mat[15 + q] << 24);
    hi = P.mat[20 + q];
}
/* the column of query base qb (0 .. 4) among the five */
__device__ __forceinline__ void matrix_column_of(const int qb, const uint32_t (&cp_lo)[5], const int (&cp_hi)[5], uint32_t &lo, int &hi)
{
    lo = cp_lo[4];
    hi = cp_hi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        lo = qb == q ? cp_lo[q] : lo;
        hi = qb == q ? cp_hi[q] : hi;
    }
}

/* The dynamic-LDS limit is a property of the kernel ON A DEVICE: it is set on every device the kernel is launched on (the
 * current one), remembered per device only once it has succeeded, and a failure is returned, never cached.  set_on: the
 * caller's own static word per kernel instantiation, bit d = set on device d. */
inline hipError_t set_lds_ceiling(const void *kernel, int bytes, std::atomic<uint64_t> &set_on)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = dev >= 0 && dev < 64 ? 1ull << dev : 0ull;
    if (bit && (set_on.load(std::memory_order_acquire) & bit)) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) set_on.fetch_or(bit, std::memory_order_release);
    return e;
}

}  // namespace
}  // namespace bsw
