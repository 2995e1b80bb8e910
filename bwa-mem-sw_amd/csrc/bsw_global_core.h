/*
 * bsw_global_core.h — what bsw_global_kernel.hip and bsw_global_long_kernel.hip compute alike, stated once: the cell of bwa's
 * ksw_global2 with its direction byte, and the CIGAR writer of the traceback.  Where the row lives (registers against an LDS
 * ring) and how the backtrack matrix is walked (lane 0 reading HBM against a wave-uniform walk over LDS tiles) is each kernel's.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bsw {
namespace {

/* One cell: m = H(i-1,j-1) + s, e = E(i,j), f = F(i,j) -> h = H(i,j), en = E(i+1,j) and the direction byte h | e<<2 | f<<4
 * (bwa's encoding: h 0 = diagonal, 1 = from E, 2 = from F; the e and f fields say whether the gap is extended).  The order of
 * the >= / > tests is bwa's: the direction of a tie depends on it. */
__device__ __forceinline__ void global_cell(const int m, const int e, const int f, const int oe_del, const int e_del,
                                            const int oe_ins, const int e_ins, int &h, int &en, uint32_t &d)
{
    d = m >= e ? 0u : 1u;
    h = m >= e ? m : e;
    d = h >= f ? d : 2u;
    h = h >= f ? h : f;
    int t = m - oe_del;
    const int e2 = e - e_del;
    d |= e2 > t ? 1u << 2 : 0u;
    en = e2 > t ? e2 : t;
    t = m - oe_ins;
    d |= (f - e_ins) > t ? 2u << 4 : 0u;
}

/* The CIGAR of a traceback, which meets its operations last to first: runs of one operation are merged in `last` and a
 * finished run goes to cg[] while it fits max_cigar.  Every lane that walks makes the same calls; `writer` says whether this
 * lane is the one that stores. */
struct cigar_writer {
    uint32_t *cg;
    int max_cigar;
    bool writer;
    int n_cigar = 0;
    uint32_t last = 0xffffffffu;

    __device__ __forceinline__ void push(const uint32_t op, const int len)
    {
        if (n_cigar == 0 || op != (last & 0xf)) {
            if (writer && n_cigar > 0 && n_cigar <= max_cigar) cg[n_cigar - 1] = last;
            last = ((uint32_t)len << 4) | op;
            ++n_cigar;
        } else last += (uint32_t)len << 4;
    }
    /* After the walk stopped at (i, k): the rest of the target is a deletion, the rest of the query an insertion; then the runs
     * are put in order.  Returns n_cigar, negated when the runs did not fit (the caller retries with more room). */
    __device__ __forceinline__ int finish(const int i, const int k)
    {
        if (i >= 0) push(2u, i + 1);
        if (k >= 0) push(1u, k + 1);
        if (writer) {
            if (n_cigar > 0 && n_cigar <= max_cigar) cg[n_cigar - 1] = last;
            if (n_cigar <= max_cigar)
                for (int a = 0; a < n_cigar >> 1; ++a) { const uint32_t t = cg[a]; cg[a] = cg[n_cigar - 1 - a]; cg[n_cigar - 1 - a] = t; }
        }
        return n_cigar > max_cigar ? -n_cigar : n_cigar;
    }
};

}  // namespace
}  // namespace bsw
