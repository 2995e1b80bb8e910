/*
 * bsw_band_scan.h — wave helpers shared by the kernels whose lanes follow the band (bsw_long_kernel.hip,
 * bsw_global_long_kernel.hip): a DPP move and the inclusive 64-lane max-scan behind the F recurrence.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <limits.h>

namespace bsw {
namespace {

template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf>
__device__ __forceinline__ int bdpp(int old, int src)
{
    return __builtin_amdgcn_update_dpp(old, src, CTRL, ROW_MASK, BANK_MASK, false);
}

/* inclusive max-scan over the 64 lanes (row_shr 1,2,4,8 + row_bcast 15/31) */
__device__ __forceinline__ int band_scan_max(int x)
{
    x = max(x, bdpp<0x111>(INT_MIN, x));
    x = max(x, bdpp<0x112>(INT_MIN, x));
    x = max(x, bdpp<0x114>(INT_MIN, x));
    x = max(x, bdpp<0x118>(INT_MIN, x));
    x = max(x, bdpp<0x142, 0xa>(INT_MIN, x));
    x = max(x, bdpp<0x143, 0xc>(INT_MIN, x));
    return x;
}

}  // namespace
}  // namespace bsw
