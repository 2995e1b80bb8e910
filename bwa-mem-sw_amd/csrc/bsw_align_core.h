/*
 * bsw_align_core.h — bwa's ksw_align2 around the striped pass, what bsw_align_kernel.hip and bsw_align_long_kernel.hip compute
 * alike, stated once: the xtra flags, the result of a pass, the constants of a launch and of a pass, the b[] list of sub-optimal
 * ends, the new-maximum / stop rule, the qe key, the second-best scan, the start-point pass's predicate and result, the store.
 * The DP loops (H, E and Hmax in registers against LDS) are each kernel's.  One alignment per group of NP = 16 (8-bit mode) or
 * 8 (16-bit mode) lanes, l = the lane within its group.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsw_band_scan.h"
#include "bsw_device.h"

namespace bsw {
namespace {

/* ksw.h's xtra: the low 16 bits are a score, then */
constexpr int XBYTE = 0x10000, XSTOP = 0x20000, XSUBO = 0x40000, XSTART = 0x80000;

struct align_res { int score, te, qe, score2, te2, tb, qb; };

/* per launch: ksw_qinit's shift (8-bit mode stores score + shift) and the matrix maximum */
__device__ __forceinline__ void matrix_shift_max(const bsw_dparams &P, int &shift, int &mx)
{
    int smin = 127, smax = 0;
#pragma unroll
    for (int a = 0; a < 25; ++a) { smin = min(smin, (int)P.mat[a]); smax = max(smax, (int)P.mat[a]); }
    shift = (256 - (smin & 0xff)) & 0xff;
    mx = smax;
}

/* per pass: the largest H the mode can hold, the score a row needs to enter b[] (XSUBO), the score that ends the pass (XSTOP) */
template <bool BYTE>
__device__ __forceinline__ int align_hcap(const int shift) { return BYTE ? 255 - shift : 32767; }
__device__ __forceinline__ int align_minsc(const int xtra) { return (xtra & XSUBO) ? (xtra & 0xffff) : 0x10000; }
__device__ __forceinline__ int align_endsc(const int xtra) { return (xtra & XSTOP) ? (xtra & 0xffff) : 0x10000; }

/* b[]: row i, whose maximum imax reached minsc, is appended, or replaces the last entry when it is the row right after it and
 * scores higher; an entry is (score << 32 | row), stored by the group's lane 0.  The list's state goes in and comes back by
 * value (start it at {0, -2, 0}): through references both kernels need two more VGPRs. */
struct blist_at { int n_b, last_i, last_s; };
__device__ __forceinline__ blist_at blist_note(unsigned long long *__restrict__ bl, const int l, const int i, const int imax, blist_at b)
{
    if (b.n_b == 0 || b.last_i + 1 != i) {
        if (l == 0) bl[b.n_b] = ((unsigned long long)(uint32_t)imax << 32) | (uint32_t)i;
        ++b.n_b; b.last_i = i; b.last_s = imax;
    } else if (b.last_s < imax) {
        if (l == 0) bl[b.n_b - 1] = ((unsigned long long)(uint32_t)imax << 32) | (uint32_t)i;
        b.last_i = i; b.last_s = imax;
    }
    return b;
}

/* a new maximum gmax ends the pass when it saturates the 8-bit mode or reaches XSTOP's score */
template <bool BYTE>
__device__ __forceinline__ bool align_stops(const int gmax, const int shift, const int endsc)
{
    return BYTE ? (gmax + shift >= 255 || gmax >= endsc) : (gmax >= endsc);
}
/* the result as the row loop leaves it: 255 = the 8-bit mode overflowed (the host repeats the alignment in 16-bit mode) */
template <bool BYTE>
__device__ __forceinline__ align_res align_res_of(const int gmax, const int shift, const int te)
{
    align_res r;
    r.score = BYTE ? (gmax + shift < 255 ? gmax : 255) : gmax;
    r.te = te; r.qe = -1; r.score2 = -1; r.te2 = -1; r.tb = -1; r.qb = -1;
    return r;
}

/* qe: the first maximum of the kept column Hmax in memory order at = j * NP + l; the group's largest key names it */
__device__ __forceinline__ int qe_key(const int hmax, const int at) { return (hmax << 16) | (0xffff - at); }
template <int NP>
__device__ __forceinline__ int qe_of_key(const int key, const int slen)
{
    const int mi = 0xffff - (key & 0xffff);
    return mi / NP + (mi % NP) * slen;                       /* memory order -> query position j + l * slen */
}

/* second best: of b[]'s n_b entries outside [te - d, te + d], d = ceil(score / mx), the first of the highest score.  scan: this
 * group has a list to scan (group-uniform); every lane of the wavefront that reaches the pass's end makes the call. */
template <int NP>
__device__ __forceinline__ void second_best(const bool scan, const unsigned long long *__restrict__ bl, const int n_b, const int l,
                                            const int mx, align_res &r)
{
    if (__builtin_amdgcn_ballot_w64(scan) == 0) return;
    __threadfence_block();
    const int d = (r.score + mx - 1) / mx, low = r.te - d, high = r.te + d;
    unsigned long long best = 0;                             /* (score + 1) << 32 | ~index : 0 = none */
    if (scan)
        for (int x = l; x < n_b; x += NP) {
            const unsigned long long ent = bl[x];
            const int e = (int)(uint32_t)ent, sc = (int)(ent >> 32);
            if (e < low || e > high) {
                const unsigned long long kk = ((unsigned long long)(uint32_t)(sc + 1) << 32) | (uint32_t)(0x7fffffff - x);
                best = kk > best ? kk : best;
            }
        }
    best = group_max_u64<NP>(best);
    if (scan && best != 0) {
        const int x = 0x7fffffff - (int)(uint32_t)best;
        const int sc = (int)(best >> 32) - 1;
        if (sc > r.score2) { r.score2 = sc; r.te2 = (int)(uint32_t)bl[x]; }
    }
}

/* the start-point pass (XSTART) runs unless XSUBO's score was not reached; it ran on the mirrored prefixes, so its ends are
 * distances back from (te, qe), and they count only if it found the same score */
__device__ __forceinline__ bool wants_start_pass(const int xtra, const int score)
{
    return !((xtra & XSTART) == 0 || ((xtra & XSUBO) && score < (xtra & 0xffff)));
}
__device__ __forceinline__ void take_start(const bool second, const align_res &rr, align_res &r)
{
    if (second && r.score == rr.score) { r.tb = r.te - rr.te; r.qb = r.qe - rr.qe; }
}

__device__ __forceinline__ void store_kswr(bsw_kswr *__restrict__ out, const align_res r)
{
    bsw_kswr o;
    o.score = r.score; o.te = r.te; o.qe = r.qe; o.score2 = r.score2; o.te2 = r.te2; o.tb = r.tb; o.qb = r.qb;
    *out = o;
}

}  // namespace
}  // namespace bsw
