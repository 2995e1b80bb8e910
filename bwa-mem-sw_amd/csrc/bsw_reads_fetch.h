/*
 * bsw_reads_fetch.h — one output word of a query sequence out of the RESIDENT READ STORE (bsw_reads_upload): the third source
 * of bsw_pack_kernel beside raw bytes and the pac (internal; the public C ABI is include/bwa_sw_mi355.h).
 *
 * The store is the device sequence format itself — 4 bits per base, 16 bases per uint64, base k of a word in bits [4k, 4k+3],
 * codes 0..4 — with every read on a word boundary, so a base has a POSITION: 16 * (word offset of its read) + index in the read.
 * A sequence the kernels want is a run of L bases that starts at position s and runs forwards (right flank, forward-strand CIGAR
 * slice, mate) or backwards (left flank, reverse-strand CIGAR read); it starts anywhere inside a word, so output word k is a
 * 64-bit funnel shift over two store words.  BSW_READS_SLACK zeroed words sit in front of the first read and behind the last
 * one: the two-word read of a window that hangs over either end of the store stays inside the allocation.
 *
 * BSW_HD: the kernel inlines it, and g++ compiles it for tests/test_reads_fetch_model.py as it does bsw_lane2_core.h.
 */
#ifndef BSW_READS_FETCH_H
#define BSW_READS_FETCH_H

#include <stdint.h>
#include "bsw_device.h"

/* flag bits of launch_pack's `rev_left` argument */
#define BSW_PACK_REV_LEFT 1     /* the left query is read backwards from its offset */
#define BSW_PACK_STORE    4     /* the queries come from the resident read store: raw = the store's word 0, rawoff = base positions */

#define BSW_READS_SLACK   2     /* zeroed words in front of and behind the reads of a device copy */

/* the 16 nibbles of a word in reverse order */
BSW_HD uint64_t bsw_rev_nibbles64(uint64_t v)
{
    v = __builtin_bswap64(v);
    return ((v >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((v & 0x0F0F0F0F0F0F0F0Full) << 4);
}

/* word k (16 k < L) of the sequence of L bases whose base i sits at position s + i (forwards) or s - i (backwards).  `store`
 * addresses word 0 of the reads; words -1 and (last + 1) are slack.  Nibbles past L are cleared. */
BSW_HD uint64_t bsw_reads_word(const uint64_t *store, uint32_t s, int backwards, int L, int k)
{
    const int valid = L - 16 * k;
    if (valid <= 0) return 0;
    /* the window's lowest position: s + 16 k forwards, (s - 16 k) - 15 backwards (>= -15: the sequence lies inside the store) */
    const int64_t p = backwards ? (int64_t)s - 16 * (int64_t)k - 15 : (int64_t)s + 16 * (int64_t)k;
    const int64_t w = ((p + 16) >> 4) - 1;
    const uint32_t sh = 4u * (uint32_t)((p + 16) & 15);
    const uint64_t lo = store[w], hi = store[w + 1];
    uint64_t v = sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
    if (backwards) v = bsw_rev_nibbles64(v);
    if (valid < 16) v &= (1ull << (4 * valid)) - 1ull;
    return v;
}

#endif
