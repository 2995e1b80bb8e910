/*
 * bsw_reads_pack.h — one word of the resident read store out of the reads' RAW BYTES (bsw_reads_upload_start[_enc]): what
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
 * The bytes are codes (BSW_READS_CODES), or FASTQ letters (BSW_READS_ASCII: the same loads and shift, the eight bytes of a
 * 64-bit register translated at once in front of the squeeze), or the read already lies 4-bit packed on an 8-byte boundary
 * (BSW_READS_PACKED: output word k is the lower or upper half of ONE aligned 16-byte load, its nibbles clamped and its tail
 * masked).  The encoding travels per read in the record; bsw_rdpack_word_enc takes it, bsw_rdpack_word is its encoding 0.
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

/* how a read lies in the raw buffer (the values of BSW_READS_CODES / _ASCII / _PACKED, include/bwa_sw_mi355.h) */
#define BSW_RDPACK_CODES  0u
#define BSW_RDPACK_ASCII  1u
#define BSW_RDPACK_PACKED 2u

/* one read of a piece: where its bytes start in the piece's raw buffer, where its words go in the store, its length in bases,
 * its encoding (uniform over the lanes of a read; the reads of one launch may differ) */
typedef struct bsw_rdpack_rec {
    uint32_t raw_off, woff;
    int32_t  len;
    uint32_t enc;
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

/* eight FASTQ letters -> eight codes: A a 0, C c 1, G g 2, T t 3, every other byte 4.  The case bit folded away, the code of a
 * letter is ((b >> 1) ^ (b >> 2)) & 3; a byte equals one of the four patterns iff the XOR with it is a zero byte, found bytewise
 * without a carry between bytes ((y & 0x7f) + 0x7f sets bit 7 of a byte iff its low seven bits are not all zero). */
BSW_HD uint64_t bsw_rdpack_letters8(uint64_t x)
{
    const uint64_t L7 = 0x7F7F7F7F7F7F7F7Full, H = 0x8080808080808080ull;
    const uint64_t u = x & 0xDFDFDFDFDFDFDFDFull;
    const uint64_t ya = u ^ 0x4141414141414141ull, yc = u ^ 0x4343434343434343ull, yg = u ^ 0x4747474747474747ull, yt = u ^ 0x5454545454545454ull;
    const uint64_t na = ((ya & L7) + L7) | ya, nc = ((yc & L7) + L7) | yc, ng = ((yg & L7) + L7) | yg, nt = ((yt & L7) + L7) | yt;
    const uint64_t other = (na & nc & ng & nt & H) >> 7;                 /* 0x01 in every byte that is none of the four */
    const uint64_t code = ((u >> 1) ^ (u >> 2)) & 0x0303030303030303ull;
    return (code & ~(other * 3ull)) | (other << 2);
}

/* sixteen nibbles, every one above 4 becomes 4: n + 3 carries into bit 3 for 5..7, bit 3 itself says 8..15, and a nibble that
 * has bit 3 either way keeps bit 2 alone (4 + 3 = 7 carries nowhere) */
BSW_HD uint64_t bsw_rdpack_clamp_nibbles(uint64_t x)
{
    const uint64_t lo3 = x & 0x7777777777777777ull;
    const uint64_t big = (((lo3 + 0x3333333333333333ull) | x) & 0x8888888888888888ull) >> 3;      /* 0x1 in every nibble above 4 */
    return (x & ~(big * 15ull)) | (big << 2);
}

/* word k (16 k < len) of the read whose first byte is raw[raw_off], its bases encoded as enc says; raw is 16-byte aligned, and
 * raw_off of a BSW_RDPACK_PACKED read a multiple of 8 */
BSW_HD uint64_t bsw_rdpack_word_enc(const uint8_t *raw, uint32_t raw_off, int len, int k, uint32_t enc)
{
    int valid = len - 16 * k;
    if (valid <= 0) return 0;
    if (valid > 16) valid = 16;
    if (enc == BSW_RDPACK_PACKED) {                  /* the word lies there: one half of one aligned load */
        const uint64_t p = (uint64_t)raw_off + 8ull * (uint64_t)k;
        const bsw_rdpack_v2 a = *(const bsw_rdpack_v2 *)(raw + (p & ~15ull));
        uint64_t v = bsw_rdpack_clamp_nibbles(p & 8 ? a[1] : a[0]);
        if (valid < 16) v &= (1ull << (4 * valid)) - 1ull;
        return v;
    }
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
    const uint64_t c0 = enc == BSW_RDPACK_ASCII ? bsw_rdpack_letters8(lo) : bsw_rdpack_clamp(lo);
    const uint64_t c1 = enc == BSW_RDPACK_ASCII ? bsw_rdpack_letters8(hi) : bsw_rdpack_clamp(hi);
    uint64_t v = bsw_rdpack_squeeze8(c0) | (bsw_rdpack_squeeze8(c1) << 32);
    if (valid < 16) v &= (1ull << (4 * valid)) - 1ull;
    return v;
}

/* encoding 0: one byte per base, codes */
BSW_HD uint64_t bsw_rdpack_word(const uint8_t *raw, uint32_t raw_off, int len, int k)
{
    return bsw_rdpack_word_enc(raw, raw_off, len, k, BSW_RDPACK_CODES);
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
