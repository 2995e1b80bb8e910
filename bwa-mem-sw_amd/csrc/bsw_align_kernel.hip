/*
 * bsw_align_kernel.hip — bwa's striped local alignment ksw_align2 (ksw_u8 / ksw_i16; SURVEY.md §8f row F4, second
 * half: the Smith-Waterman of mate rescue, mem_matesw) on gfx950.
 *
 * The outputs of the SSE2 code depend on its striping (which query position shares a vector with which, where the
 * lazy-F loop stops, that E is taken from H before the lazy-F correction, the memory order of the qe search — see
 * oracle/ksw_align_ref.c), so the kernel keeps the striping: ONE 16-LANE DPP ROW PLAYS ONE __m128i.  Lane l of the
 * row is byte lane l (8-bit mode: one alignment per row), or the row holds two alignments of 8 word lanes each
 * (16-bit mode); the slen vectors of H, E and Hmax are slen registers per lane, statically addressed (H is updated in
 * place: the old value is the next column's diagonal); _mm_slli_si128 is one `row_shr:1` with the group's lane 0
 * forced to zero; the horizontal max and the "all lanes done" test of the lazy-F loop are DPP butterflies / a ballot.
 * Four (eight) alignments per wavefront; the per-lane score profile lives in LDS, one column per thread.  The sub-optimal list b[] goes to HBM (8 bytes per
 * qualifying row) and is scanned by the row's 16 lanes afterwards.  The start-point pass (KSW_XSTART) runs in the same
 * kernel on the mirrored prefixes by index arithmetic, no sequence is reversed in memory.
 * Integer max/add work, ~14 VALU + 1 LDS read per cell and lane: VALU-issue-bound like the extension kernels, but at
 * one cell per lane-op (no two-per-register packing: the striping decides what shares a register).
 */
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "bsw_align_core.h"
#include "bsw_device.h"
#include "bsw_stage.h"

namespace bsw {

namespace {

/* One run of ksw_u8 (BYTE) / ksw_i16 for the alignment of this 16-lane row.  `on`: the row takes part (row-uniform).
 * Query position k is q[qrev ? qlast - k : k]; target row i is t[i <= trev ? trev - i : i] (trev = -1: forwards).
 * qrc: q is the reverse complement of the stored sequence s of qn + 1 bases, q[idx] = comp(s[qn - idx]) (mem_matesw's is_rev). */
template <int SLEN, bool BYTE>
__device__ __forceinline__ align_res align_pass(const bool on, const int qlen, const int tlen, const uint64_t *__restrict__ seq,
                                            const uint32_t q_off, const int qlast, const bool qrev, const bool qrc, const int qn,
                                            const uint32_t t_off, const int trev,
                                            const int xtra, const bsw_dparams &P, const int shift, const int mx,
                                            int8_t (*prof)[SLEN][256], unsigned long long *__restrict__ bl)
{
    constexpr int NP = BYTE ? 16 : 8;                /* lanes of the SSE vector = lanes of the group: a 16-lane DPP row holds one
                                                         8-bit alignment or two 16-bit ones */
    const int tid = threadIdx.x, l = tid & (NP - 1);
    constexpr bool lane_on = true;
    const int slen = (qlen + NP - 1) / NP;
    const int oe_del = P.o_del + P.e_del, oe_ins = P.o_ins + P.e_ins, e_del = P.e_del, e_ins = P.e_ins;
    const int hcap = align_hcap<BYTE>(shift), minsc = align_minsc(xtra), endsc = align_endsc(xtra);
    /* ksw_qinit: the score of (target base a, query position j + l * slen), 0 past the end of the query */
#pragma unroll
    for (int j = 0; j < SLEN; ++j) {
        const int k = j + l * slen;
        const bool real = on && lane_on && j < slen && k < qlen;
        const int idx = qrev ? qlast - k : k;
        int qc = real ? base_at(seq, q_off, qrc ? qn - idx : idx) : 0;
        if (qrc) qc = qc < 4 ? 3 - qc : 4;                           /* (a non-real lane's 0 becomes 3: its profile is 0 anyway) */
#pragma unroll
        for (int a = 0; a < 5; ++a) prof[a][j][tid] = real ? P.mat[a * 5 + qc] : (int8_t)0;
    }
    int H[SLEN], E[SLEN], Hmax[SLEN];
#pragma unroll
    for (int j = 0; j < SLEN; ++j) H[j] = E[j] = Hmax[j] = 0;
    int gmax = 0, te = -1, hl = 0;       /* hl = H[slen - 1] of the previous row */
    blist_at b{0, -2, 0};
    bool live = on && slen > 0;
    for (int i = 0;; ++i) {
        const bool ra = live && i < tlen;
        if (__builtin_amdgcn_ballot_w64(ra) == 0) break;
        const int ti = ra ? (i <= trev ? trev - i : i) : 0;
        const int tb = ra ? base_at(seq, t_off, ti) : 0;
        int f = 0, mxv = 0;
        int h = dpp_mov<0x111>(0, hl);                                     /* H(i-1,-1): the last vector, one lane up */
        h = l == 0 ? 0 : h;
#pragma unroll
        for (int j = 0; j < SLEN; ++j) {
            if (ra && j < slen) {
                const int s = prof[tb][j][tid];
                int hh = min(h + s, hcap);
                if (BYTE) hh = max(hh, 0);
                const int e = E[j];
                hh = max(max(hh, e), f);
                mxv = max(mxv, hh);
                h = H[j];
                H[j] = hh;
                E[j] = max(max(e - e_del, hh - oe_del), 0);
                f = max(max(f - e_ins, hh - oe_ins), 0);
            }
        }
        /* lazy F: at most 16 rounds, out as soon as no lane's F exceeds H - oe_ins */
        bool lz = ra;
        for (int k = 0; k < 16; ++k) {
            if (__builtin_amdgcn_ballot_w64(lz) == 0) break;
            const int fs = dpp_mov<0x111>(0, f);
            f = lz ? (l == 0 ? 0 : fs) : f;
#pragma unroll
            for (int j = 0; j < SLEN; ++j) {
                if (__builtin_amdgcn_ballot_w64(lz) == 0) break;           /* usually after the first vector or two */
                const bool go = lz && j < slen;
                int hh = max(H[j], f);
                H[j] = go ? hh : H[j];
                hh = max(hh - oe_ins, 0);
                const int fn = max(f - e_ins, 0);
                f = go ? fn : f;
                const bool any = group_any<NP>(go && lane_on && fn > hh, tid);
                lz = go ? any : lz;                                        /* (rows past their slen keep lz and skip on their own) */
            }
        }
#pragma unroll
        for (int j = 0; j < SLEN; ++j) hl = (ra && j == slen - 1) ? H[j] : hl;
        const int imax = group_max<NP>(mxv);
        if (ra && imax >= minsc) b = blist_note(bl, l, i, imax, b);        /* the b array of sub-optimal ends */
        if (ra && imax > gmax) {
            gmax = imax; te = i;
#pragma unroll
            for (int j = 0; j < SLEN; ++j) Hmax[j] = H[j];
            if (align_stops<BYTE>(gmax, shift, endsc)) live = false;
        }
    }
    align_res r = align_res_of<BYTE>(gmax, shift, te);
    if (!BYTE || r.score != 255) {
        /* qe: the first maximum of the kept column in memory order i = j * NP + lane -> position j + lane * slen */
        int key = -1;
#pragma unroll
        for (int j = 0; j < SLEN; ++j)
            if (lane_on && j < slen) key = max(key, qe_key(Hmax[j], j * NP + l));
        key = group_max<NP>(key);
        if (slen > 0) r.qe = qe_of_key<NP>(key, slen);
        second_best<NP>(b.n_b > 0, bl, b.n_b, l, mx, r);
    }
    return r;
}

}  // namespace

/* one local alignment per 16-lane row; tasks[] says where its sequences sit in seq, its flags, its slice of the b[] scratch */
template <int SLEN, bool BYTE>
__global__ __launch_bounds__(256) void bsw_align_kernel(const bsw_dparams P, const uint64_t *__restrict__ seq,
                                                        const bsw_adtask *__restrict__ tasks, const uint32_t *__restrict__ order,
                                                        const uint32_t n, unsigned long long *__restrict__ blist, bsw_kswr *__restrict__ out)
{
    __shared__ int8_t prof[5][SLEN][256];
    constexpr int GW = BYTE ? 16 : 8, APB = 256 / GW;               /* lanes per alignment, alignments per workgroup */
    const int tid = threadIdx.x, l = tid & (GW - 1);
    const uint32_t slot = blockIdx.x * (uint32_t)APB + (uint32_t)(tid / GW);
    const bool valid = slot < n;
    const uint32_t ai = order[valid ? slot : 0];
    const bsw_adtask T = tasks[ai];
    int smin = 127, smax = 0;                                        /* (matrix_shift_max of bsw_align_core.h, stated here: through */
#pragma unroll                                                       /* the shared function the 20-word kernel spills to scratch) */
    for (int a = 0; a < 25; ++a) { smin = min(smin, (int)P.mat[a]); smax = max(smax, (int)P.mat[a]); }
    const int shift = (256 - (smin & 0xff)) & 0xff, mx = smax;
    unsigned long long *bl = blist + T.b_off;
    const bool qrc = (T.pad & BSW_AD_QRC) != 0;
    align_res r = align_pass<SLEN, BYTE>(valid, T.qlen, T.tlen, seq, T.q_off, 0, false, qrc, T.qlen - 1, T.t_off, -1, T.xtra, P, shift, mx,
                                     prof, bl);
    const bool second = valid && wants_start_pass(T.xtra, r.score);
    if (__builtin_amdgcn_ballot_w64(second) != 0) {
        /* (the profile is rebuilt for the mirrored prefix; every thread owns its column of it: no barrier) */
        const align_res rr = align_pass<SLEN, BYTE>(second, r.qe + 1, T.tlen, seq, T.q_off, r.qe, true, qrc, T.qlen - 1, T.t_off, r.te,
                                                XSTOP | r.score, P, shift, mx, prof, bl);
        take_start(second, rr, r);
    }
    if (valid && l == 0) store_kswr(&out[ai], r);
}

/* classes: (mode, vectors per lane) -> query length up to lanes * vectors */
/* (10 / 20 vectors: 150 bp reads, the common case, without the predicated tail of the 16 / 32 vector kernels) */
/* (32 / 64 byte vectors and 64 / 128 word vectors: queries up to 1024 bases — bwa's ksw_align2 has no length limit and
 * mate rescue of 2x300 reads must not lose its alignment; the long classes run at one wave per SIMD, rare by design) */
static const struct { int byte, slen; } kAlignClasses[] = {{1, 8}, {1, 10}, {1, 16}, {1, 32}, {1, 64}, {0, 16}, {0, 20}, {0, 32}, {0, 64}, {0, 128}};
int align_class_count() { return (int)(sizeof(kAlignClasses) / sizeof(kAlignClasses[0])); }
int align_class_of(int qlen, int byte_mode)
{
    for (int c = 0; c < align_class_count(); ++c)
        if (kAlignClasses[c].byte == (byte_mode ? 1 : 0) && qlen <= kAlignClasses[c].slen * (byte_mode ? 16 : 8)) return c;
    return -1;
}

hipError_t launch_align(int cls, const bsw_dparams &P, const uint64_t *seq, const bsw_adtask *tasks, const uint32_t *order, uint32_t n,
                        unsigned long long *blist, bsw_kswr *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const bool byte = kAlignClasses[cls].byte != 0;
    const uint32_t apb = byte ? 16u : 32u;
    const dim3 grid((n + apb - 1u) / apb), block(256);
    switch (cls) {
    case 0: hipLaunchKernelGGL((bsw_align_kernel<8, true>), grid, block, 0, s, P, seq, tasks, order, n, blist, out); break;
    case 1: hipLaunchKernelGGL((bsw_align_kernel<10, true>), grid, block, 0, s, P, seq, tasks, order, n, blist, out); break;
    case 2: hipLaunchKernelGGL((bsw_align_kernel<16, true>), grid, block, 0, s, P, seq, tasks, order, n, blist, out); break;
    case 3: hipLaunchKernelGGL((bsw_align_kernel<32, true>), grid, block, 0, s, P, seq, tasks, order, n, blist, out); break;
    case 4: hipLaunchKernelGGL((bsw_align_kernel<64, true>), grid, block, 0, s, P, seq, tasks, order, n, blist, out); break;
    case 5: hipLaunchKernelGGL((bsw_align_kernel<16, false>), grid, block, 0, s, P, seq, tasks, order, n, blist, out); break;
    case 6: hipLaunchKernelGGL((bsw_align_kernel<20, false>), grid, block, 0, s, P, seq, tasks, order, n, blist, out); break;
    case 7: hipLaunchKernelGGL((bsw_align_kernel<32, false>), grid, block, 0, s, P, seq, tasks, order, n, blist, out); break;
    case 8: hipLaunchKernelGGL((bsw_align_kernel<64, false>), grid, block, 0, s, P, seq, tasks, order, n, blist, out); break;
    case 9: hipLaunchKernelGGL((bsw_align_kernel<128, false>), grid, block, 0, s, P, seq, tasks, order, n, blist, out); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace bsw
