/*
 * bsw_reads_pack_kernel.hip — the device side of bsw_reads_upload_start: a piece of a read block, one byte per base as it crossed
 * PCIe, becomes its part of the resident read store (4 bits per base, every read on a word boundary).
 *
 * Bound by memory: 1 byte per base in, half a byte out.  A group of BSW_RDPACK_GROUP lanes takes a read and lane l produces its
 * words l, l + 16, ...: the lanes of a group load neighbouring 16-byte lines of the read and store neighbouring 8-byte words.
 * A word is bsw_rdpack_word_enc (bsw_reads_pack.h): two aligned 16-byte loads, a funnel shift, two squeezes — no byte loads, no
 * LDS, nothing in scratch.  A read of length 0 writes nothing.  The record says how a read's bases are encoded — codes, FASTQ
 * letters (translated eight bytes at a time in front of the squeeze), or 4-bit words (one load, half a byte per base in) — the
 * same for the 16 lanes of a read, so the branch on it never splits a group.
 */
#include <hip/hip_runtime.h>
#include <algorithm>
#include "bsw_reads_pack.h"

namespace bsw {

#define RDPACK_THREADS 256
#define RDPACK_MAX_BLOCKS 16384u

__global__ __launch_bounds__(RDPACK_THREADS) void bsw_reads_pack_kernel(const uint8_t *__restrict__ raw, const bsw_rdpack_rec *__restrict__ rec,
                                                                         uint32_t n, uint64_t *__restrict__ store)
{
    const int lane = (int)(threadIdx.x & (BSW_RDPACK_GROUP - 1));
    const uint32_t per_block = RDPACK_THREADS / BSW_RDPACK_GROUP;
    const uint32_t stride = gridDim.x * per_block;
    for (uint32_t r = blockIdx.x * per_block + threadIdx.x / BSW_RDPACK_GROUP; r < n; r += stride) {
        const bsw_rdpack_rec rc = rec[r];
        const int nw = (rc.len + 15) >> 4;
        uint64_t *dst = store + rc.woff;
        for (int k = lane; k < nw; k += BSW_RDPACK_GROUP) dst[k] = bsw_rdpack_word_enc(raw, rc.raw_off, rc.len, k, rc.enc);
    }
}

hipError_t launch_reads_pack(const uint8_t *raw, const bsw_rdpack_rec *rec, uint32_t n, uint64_t *store, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (((uintptr_t)raw & 15) != 0) return hipErrorInvalidValue;
    const uint32_t per_block = RDPACK_THREADS / BSW_RDPACK_GROUP;
    const uint32_t blocks = std::min<uint32_t>((n + per_block - 1) / per_block, RDPACK_MAX_BLOCKS);
    hipLaunchKernelGGL(bsw_reads_pack_kernel, dim3(blocks), dim3(RDPACK_THREADS), 0, s, raw, rec, n, store);
    return hipGetLastError();
}

}  // namespace bsw
