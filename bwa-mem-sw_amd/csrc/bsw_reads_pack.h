/*
 * bsw_reads_pack.h — one word of the resident read store out of the reads' RAW BYTES (bsw_reads_upload_start): what
 * bsw_reads_pack_kernel computes per lane, stated once (internal; the public C ABI is include/bwa_sw_mi355.h).
 *
 * A piece of a read block lies in a raw buffer, one byte per base, a read anywhere in it (the caller's memory as it lies, or a
 * gather).  The store wants the device sequence format: 4 bits per base, base k of a word in bits [4k, 4k+3], every byte value
 * above 4 stored as 4, every read on a word boundary, the nibbles behind a read's last base zero.  Output word k of a read takes
 * the 16 bytes from raw_off + 16 k: two aligned 16-byte loads around that address, funnel-shifted by its low four bits, then
 * eight bytes squeezed into 32 bits twice.  The upper load is made only when the word needs a byte of it, and then it runs up
 * to 15 bytes past the read: the raw buffer is 16-byte aligned and carries BSW_RDPACK_RAW_SLACK allocated bytes behind its last
 * byte, whose content is masked away.
 *
 * BSW_HD: the kernel inlines it, g++ compiles it for tests/test_reads_pack_model.py, and the host double's stand-in launcher
 * is checked against it.
 */
#ifndef BSW_READS_PACK_H
#define BSW_READS_PACK_H

#include <stdint.h>
#include "bsw_device.h"

#define BSW_RDPACK_RAW_SLACK 16     /* allocated bytes behind the last raw byte of a piece */
#define BSW_RDPACK_GROUP     16     /* lanes per read: lane l produces words l, l + 16, ... */

/* one read of a piece: where its bytes start in the piece's raw buffer, where its words go in the store, its length */
typedef struct bsw_rdpack_rec {
    uint32_t raw_off, woff;
    int32_t  len;
    uint32_t pad;
} bsw_rdpack_rec;

typedef uint64_t bsw_rdpack_v2 __attribute__((vector_size(16), aligned(16)));

/* eight bytes with a code each -> eight nibbles in the low 32 bits */
BSW_HD uint64_t bsw_rdpack_squeeze8(uint64_t x)
{
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return x;
}

/* every byte above 4 becomes 4 (5..7 by bit arithmetic; a byte with a bit above those, which bwa never produces, bytewise) */
BSW_HD uint64_t bsw_rdpack_clamp(uint64_t x)
{
    if (x & 0xF8F8F8F8F8F8F8F8ull) {
        uint64_t v = 0;
        for (int k = 0; k < 8; ++k) {
            const uint64_t b = (x >> (8 * k)) & 0xff;
            v |= (b > 4 ? 4ull : b) << (8 * k);
        }
        return v;
    }
    const uint64_t n = x & 0x0404040404040404ull;
    return x & ~((n >> 1) | (n >> 2));
}

/* word k (16 k < len) of the read whose first byte is raw[raw_off]; raw is 16-byte aligned */
BSW_HD uint64_t bsw_rdpack_word(const uint8_t *raw, uint32_t raw_off, int len, int k)
{
    int valid = len - 16 * k;
    if (valid <= 0) return 0;
    if (valid > 16) valid = 16;
    const uint64_t p = (uint64_t)raw_off + 16ull * (uint64_t)k;
    const uint32_t ph = (uint32_t)(p & 15);
    const bsw_rdpack_v2 *q = (const bsw_rdpack_v2 *)(raw + (p & ~15ull));
    const bsw_rdpack_v2 a = q[0];
    bsw_rdpack_v2 b = {0, 0};
    if (ph + (uint32_t)valid > 16) b = q[1];
    /* bytes ph .. ph + 15 of the 32 */
    const uint64_t x0 = ph & 8 ? a[1] : a[0], x1 = ph & 8 ? b[0] : a[1], x2 = ph & 8 ? b[1] : b[0];
    const uint32_t sh = 8u * (ph & 7);
    const uint64_t lo = sh ? (x0 >> sh) | (x1 << (64u - sh)) : x0;
    const uint64_t hi = sh ? (x1 >> sh) | (x2 << (64u - sh)) : x1;
    uint64_t v = bsw_rdpack_squeeze8(bsw_rdpack_clamp(lo)) | (bsw_rdpack_squeeze8(bsw_rdpack_clamp(hi)) << 32);
    if (valid < 16) v &= (1ull << (4 * valid)) - 1ull;
    return v;
}

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
namespace bsw {
/* store[rec[i].woff + k] = word k of read i, for the n reads of a piece; raw: 16-byte aligned, BSW_RDPACK_RAW_SLACK behind it.
 * (bsw_reads_pack_kernel.hip) */
hipError_t launch_reads_pack(const uint8_t *raw, const bsw_rdpack_rec *rec, uint32_t n, uint64_t *store, hipStream_t s);
}  // namespace bsw
#endif

#endif
