/*
 * bsw_align_long_kernel.hip — bwa's striped local alignment ksw_align2 (ksw_u8 / ksw_i16) for queries the register kernel
 * (bsw_align_kernel.hip) cannot hold: up to BSW_ALIGN_LONG_MAX_QLEN = 8 191 bases.  The opt-in of bsw_set_align_long.
 *
 * Everything the results depend on is bsw_align_kernel's: ONE 16-LANE DPP ROW PLAYS ONE __m128i (16 byte lanes, or two
 * alignments of 8 word lanes), query position k sits in vector k % slen, lane k / slen, E is taken from H before the lazy-F
 * correction, the row maximum and b[] come from the uncorrected pass, qe is the first maximum of the kept column in memory
 * order, the start-point pass runs on the mirrored prefixes by index arithmetic.  What differs is where the slen vectors live:
 * in LDS, addressed by a run-time vector index, so slen is a loop bound and not a template parameter.
 *
 * LDS per alignment, P = positions of the launch's class (lanes x slen bound); lane l owns entry [j][l] of every array, in both
 * passes, so no lane ever reads what another lane wrote and the kernel needs no barrier:
 *   HE   [P] uint32   H (low half, updated in place: the old value is the next column's diagonal) and E (high half) of one
 *                     position in one dword: a cell is ONE ds_read_b32 and ONE ds_write_b32 for both; byte values fit in 255,
 *                     word values saturate at 32 767, neither is negative
 *   Hmax [P] uint16   the H column of the best row so far (copied on a new maximum only)
 *   QC   [P] uint8    8 x the query code of the position in striped order, 40 for a position past the query's end: the score is a
 *                     byte of the 64-bit word that holds the five matrix entries of the row's target base (and a zero sixth),
 *                     shifted down by QC — no striped profile (5 bytes a position) is kept
 * = 7 bytes a position, 56 KiB for the largest class.  The stride from one alignment to the next is padded to 16 (8) dwords
 * modulo 32 banks, so the two byte rows (four word groups) of a 32-lane half, which ds_read_b32 / ds_write_b32 serve in one
 * cycle, fall on different banks.
 * Cost per vector of the main pass, from the gfx950 code (8-bit mode; 16-bit mode has no clamp at zero): 15 VALU in the cell (64-bit
 * shift, add with sign extension, min, max, max with E's half, max, sub, and, two subs, max3, sub, max, max3, shift-or), 5 VALU
 * and 9 SALU of loop control (the vector index is compared per lane and balloted, two address adds), one ds_read_b32 + one
 * ds_read_u8 + one ds_write_b32.  A lazy-F vector: one read, one write, 5 VALU + a compare and ballot.  A new maximum: one
 * ds_read_b32 + one ds_write_b16 per position.  The loop is a dependent chain through LDS, so a lone wave is bound by latency,
 * not by issue.  The DPP shifts read registers written several instructions earlier by VALU; the compiler inserts the wait
 * states where they do not.
 */
#include <hip/hip_runtime.h>
#include <atomic>
#include <limits.h>
#include <stdint.h>

#include "bsw_align_core.h"
#include "bsw_device.h"
#include "bsw_stage.h"

namespace bsw {

namespace {

/* One run of ksw_u8 (BYTE) / ksw_i16 for the alignment of this lane group; the arguments are align_pass's of
 * bsw_align_kernel.hip.  he / hm / qc: the group's three LDS arrays at this lane's column, entry j at [j * NP]. */
template <bool BYTE>
__device__ __forceinline__ align_res align_long_pass(const bool on, const int qlen, const int tlen, const uint64_t *__restrict__ seq,
                                                 const uint32_t q_off, const int qlast, const bool qrev, const bool qrc, const int qn,
                                                 const uint32_t t_off, const int trev, const int xtra, const bsw_dparams &P,
                                                 const int shift, const int mx, const uint64_t (&rows)[5],
                                                 uint32_t *he, uint16_t *hm, uint8_t *qc, unsigned long long *__restrict__ bl)
{
    constexpr int NP = BYTE ? 16 : 8;
    const int tid = threadIdx.x, l = tid & (NP - 1);
    const int slen = (qlen + NP - 1) / NP;
    const int oe_del = P.o_del + P.e_del, oe_ins = P.o_ins + P.e_ins, e_del = P.e_del, e_ins = P.e_ins;
    const int hcap = align_hcap<BYTE>(shift), minsc = align_minsc(xtra), endsc = align_endsc(xtra);
    /* ksw_qinit: the code of query position j + l * slen, 5 past the end of the query (a zero score); H = E = Hmax = 0 */
    for (int j = 0;; ++j) {
        const bool act = on && j < slen;
        if (__builtin_amdgcn_ballot_w64(act) == 0) break;
        if (act) {
            const int k = j + l * slen;
            int code = 5;
            if (k < qlen) {
                const int idx = qrev ? qlast - k : k, si = qrc ? qn - idx : idx;
                code = base_code(seq[q_off + (uint32_t)(si >> 4)], si);
                if (qrc) code = code < 4 ? 3 - code : 4;
            }
            he[j * NP] = 0u;
            hm[j * NP] = (uint16_t)0;
            qc[j * NP] = (uint8_t)(code * 8);
        }
    }
    int gmax = 0, te = -1;
    blist_at b{0, -2, 0};
    bool live = on && slen > 0;
    int tw_at = -1;
    uint64_t tw = 0;                                                      /* the target's word of 16 bases in use */
    for (int i = 0;; ++i) {
        const bool ra = live && i < tlen;
        if (__builtin_amdgcn_ballot_w64(ra) == 0) break;
        const int ti = ra ? (i <= trev ? trev - i : i) : 0;
        if (ra && (ti >> 4) != tw_at) { tw_at = ti >> 4; tw = seq[t_off + (uint32_t)tw_at]; }
        const int tb = ra ? base_code(tw, ti) : 0;
        const uint64_t sp = tb == 0 ? rows[0] : tb == 1 ? rows[1] : tb == 2 ? rows[2] : tb == 3 ? rows[3] : rows[4];
        int f = 0, mxv = 0;
        const int hl = ra ? (int)(he[(slen - 1) * NP] & 0xffffu) : 0;    /* H(i-1,-1): the last vector, one lane up */
        int h = dpp_mov<0x111>(0, hl);
        h = l == 0 ? 0 : h;
        for (int j = 0;; ++j) {
            const bool act = ra && j < slen;
            if (__builtin_amdgcn_ballot_w64(act) == 0) break;
            if (act) {
                const uint32_t v = he[j * NP];
                const int s = (int)(int8_t)(uint8_t)(sp >> qc[j * NP]);
                const int e = (int)(v >> 16);
                int hh = min(h + s, hcap);
                if (BYTE) hh = max(hh, 0);
                hh = max(max(hh, e), f);
                mxv = max(mxv, hh);
                h = (int)(v & 0xffffu);
                const int en = max(max(e - e_del, hh - oe_del), 0);
                f = max(max(f - e_ins, hh - oe_ins), 0);
                he[j * NP] = (uint32_t)hh | ((uint32_t)en << 16);
            }
        }
        /* lazy F: at most 16 rounds, out as soon as no lane's F exceeds H - oe_ins */
        bool lz = ra;
        for (int k = 0; k < 16; ++k) {
            if (__builtin_amdgcn_ballot_w64(lz) == 0) break;
            const int fs = dpp_mov<0x111>(0, f);
            f = lz ? (l == 0 ? 0 : fs) : f;
            for (int j = 0;; ++j) {
                const bool go = lz && j < slen;
                if (__builtin_amdgcn_ballot_w64(go) == 0) break;           /* (a group past its slen keeps lz for the next round) */
                int fn = f, hh = 0;
                if (go) {
                    const uint32_t v = he[j * NP];
                    hh = max((int)(v & 0xffffu), f);
                    he[j * NP] = (v & 0xffff0000u) | (uint32_t)hh;
                    hh = max(hh - oe_ins, 0);
                    fn = max(f - e_ins, 0);
                    f = fn;
                }
                const bool any = group_any<NP>(go && fn > hh, tid);
                lz = go ? any : lz;
            }
        }
        const int imax = group_max<NP>(mxv);
        if (ra && imax >= minsc) b = blist_note(bl, l, i, imax, b);        /* the b array of sub-optimal ends */
        const bool better = ra && imax > gmax;
        if (__builtin_amdgcn_ballot_w64(better) != 0) {
            for (int j = 0;; ++j) {
                const bool act = better && j < slen;
                if (__builtin_amdgcn_ballot_w64(act) == 0) break;
                if (act) hm[j * NP] = (uint16_t)(he[j * NP] & 0xffffu);
            }
            if (better) {
                gmax = imax; te = i;
                if (align_stops<BYTE>(gmax, shift, endsc)) live = false;
            }
        }
    }
    align_res r = align_res_of<BYTE>(gmax, shift, te);
    const bool fin = on && (!BYTE || r.score != 255);
    /* qe: the first maximum of the kept column in memory order i = j * NP + lane -> position j + lane * slen */
    int key = -1;
    for (int j = 0;; ++j) {
        const bool act = fin && j < slen;
        if (__builtin_amdgcn_ballot_w64(act) == 0) break;
        if (act) key = max(key, qe_key((int)hm[j * NP], j * NP + l));
    }
    key = group_max<NP>(key);
    if (fin && slen > 0) r.qe = qe_of_key<NP>(key, slen);
    /* second best: second_best of bsw_align_core.h, stated here (through the shared function this kernel is allotted one SGPR
     * less, and the build pin is exact) */
    const bool scan = fin && b.n_b > 0;
    if (__builtin_amdgcn_ballot_w64(scan) != 0) {
        __threadfence_block();
        const int d = (r.score + mx - 1) / mx, low = te - d, high = te + d;
        unsigned long long best = 0;                                       /* (score + 1) << 32 | ~index : 0 = none */
        if (scan)
            for (int x = l; x < b.n_b; x += NP) {
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
    return r;
}

}  // namespace

/* one local alignment per group of 16 (BYTE) / 8 lanes; pmax: the positions the launch's class gives every alignment in LDS,
 * stride: dwords from one alignment's arrays to the next one's.  A task whose query does not fit pmax (the launcher never lists
 * one) gets ksw_align2's empty result and touches no LDS. */
template <bool BYTE>
__global__ __launch_bounds__(256) void bsw_align_long_kernel(const bsw_dparams P, const uint64_t *__restrict__ seq,
                                                             const bsw_adtask *__restrict__ tasks, const uint32_t *__restrict__ order,
                                                             const uint32_t n, unsigned long long *__restrict__ blist, bsw_kswr *__restrict__ out,
                                                             const uint32_t pmax, const uint32_t stride)
{
    extern __shared__ uint32_t al_lds[];
    constexpr int GW = BYTE ? 16 : 8;
    const int tid = threadIdx.x, l = tid & (GW - 1), g = tid / GW;
    const uint32_t apb = blockDim.x / GW;
    const uint32_t slot = blockIdx.x * apb + (uint32_t)g;
    const bool listed = slot < n;
    const uint32_t ai = order[listed ? slot : 0];
    const bsw_adtask T = tasks[ai];
    const bool valid = listed && T.qlen >= 0 && (uint32_t)((T.qlen + GW - 1) / GW) * (uint32_t)GW <= pmax;
    int shift, mx;
    matrix_shift_max(P, shift, mx);
    uint64_t rows[5];                                                      /* the five scores of a target base, a byte each; byte 5 = 0 */
#pragma unroll
    for (int a = 0; a < 5; ++a) {
        uint64_t w = 0;
#pragma unroll
        for (int b = 0; b < 5; ++b) w |= (uint64_t)(uint8_t)P.mat[a * 5 + b] << (8 * b);
        rows[a] = w;
    }
    uint32_t *he = al_lds + (size_t)g * stride + l;
    uint16_t *hm = (uint16_t *)(al_lds + (size_t)g * stride + pmax) + l;
    uint8_t *qc = (uint8_t *)(al_lds + (size_t)g * stride + pmax + pmax / 2) + l;
    unsigned long long *bl = blist + T.b_off;
    const bool qrc = (T.pad & BSW_AD_QRC) != 0;
    align_res r = align_long_pass<BYTE>(valid, T.qlen, T.tlen, seq, T.q_off, 0, false, qrc, T.qlen - 1, T.t_off, -1, T.xtra, P, shift, mx,
                                    rows, he, hm, qc, bl);
    const bool second = valid && wants_start_pass(T.xtra, r.score);
    if (__builtin_amdgcn_ballot_w64(second) != 0) {
        const align_res rr = align_long_pass<BYTE>(second, r.qe + 1, T.tlen, seq, T.q_off, r.qe, true, qrc, T.qlen - 1, T.t_off, r.te,
                                               XSTOP | r.score, P, shift, mx, rows, he, hm, qc, bl);
        take_start(second, rr, r);
    }
    if (listed && l == 0) store_kswr(&out[ai], valid ? r : align_res_of<BYTE>(0, 0, -1));   /* (not valid: the empty result) */
}

/* classes: (mode, slen bound), powers of two; the bound decides the LDS an alignment gets and with it the alignments a workgroup holds */
static const struct { int byte, slen; } kAlignLongClasses[] = {
    {1, 16}, {1, 32}, {1, 64}, {1, 128}, {1, 256}, {1, 512},
    {0, 32}, {0, 64}, {0, 128}, {0, 256}, {0, 512}, {0, 1024}};
int align_long_class_count() { return (int)(sizeof(kAlignLongClasses) / sizeof(kAlignLongClasses[0])); }
int align_long_class_of(int qlen, int byte_mode)
{
    for (int c = 0; c < align_long_class_count(); ++c)
        if (kAlignLongClasses[c].byte == (byte_mode ? 1 : 0) && qlen <= kAlignLongClasses[c].slen * (byte_mode ? 16 : 8) &&
            qlen <= 8191) return c;
    return -1;
}

/* the launch geometry of a class: positions and dword stride per alignment, alignments per workgroup, LDS bytes */
static void align_long_class_geometry(int cls, uint32_t *pmax, uint32_t *stride, uint32_t *apb, size_t *lds)
{
    const bool byte = kAlignLongClasses[cls].byte != 0;
    const uint32_t gw = byte ? 16u : 8u, pos = (uint32_t)kAlignLongClasses[cls].slen * gw;
    const uint32_t bytes = ((7u * pos + 127u) & ~127u) + 4u * gw;          /* +16 (8) dwords modulo 32 banks from one alignment to the next */
    /* as many alignments as 64 KiB hold, up to 256 lanes; where that is less than a wavefront, up to a wavefront within the
     * 160 KiB of a CU (the largest class of each mode: two alignments in 112 KiB; the second largest: four in 112 KiB) */
    uint32_t a = 256u / gw;
    while (a > 1u && (size_t)a * bytes > (64u << 10)) a >>= 1;
    while (a * gw < 64u && (size_t)(2u * a) * bytes <= (160u << 10)) a <<= 1;
    *pmax = pos; *stride = bytes / 4u; *apb = a; *lds = (size_t)a * bytes;
}

/* what a class's launch looks like, for the build audit (tests/test_align_long_build_cpu.py): 0, or -1 for no such class */
extern "C" int bsw_alnl_class_geometry(int cls, int *byte_mode, int *slen_bound, uint32_t *alignments_per_workgroup, uint32_t *lds_per_alignment,
                                       uint64_t *lds_per_workgroup)
{
    if (cls < 0 || cls >= align_long_class_count()) return -1;
    uint32_t pmax, stride, apb;
    size_t lds;
    align_long_class_geometry(cls, &pmax, &stride, &apb, &lds);
    *byte_mode = kAlignLongClasses[cls].byte; *slen_bound = kAlignLongClasses[cls].slen;
    *alignments_per_workgroup = apb; *lds_per_alignment = stride * 4u; *lds_per_workgroup = (uint64_t)lds;
    return 0;
}

/* The dynamic-LDS limit is a property of the kernel ON A DEVICE.  It is ONE constant for every class, the 160 KiB of a CU, so
 * that threads launching different classes at once (the slot threads of a pipeline, the scalar queue's leader, a second context)
 * can never lower it below a launch on its way; set per device by set_lds_ceiling (bsw_band_scan.h), as bsw_long_kernel.hip
 * and bsw_global_long_kernel.hip do. */
#define ALNL_LDS_CEILING (160 * 1024)
template <bool BYTE>
static hipError_t align_long_lds_attr()
{
    static std::atomic<uint64_t> set_on{0};                            /* per instantiation */
    return set_lds_ceiling(reinterpret_cast<const void *>(&bsw_align_long_kernel<BYTE>), ALNL_LDS_CEILING, set_on);
}

hipError_t launch_align_long(int cls, const bsw_dparams &P, const uint64_t *seq, const bsw_adtask *tasks, const uint32_t *order, uint32_t n,
                             unsigned long long *blist, bsw_kswr *out, hipStream_t s)
{
    if (cls < 0 || cls >= align_long_class_count()) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const bool byte = kAlignLongClasses[cls].byte != 0;
    uint32_t pmax, stride, apb;
    size_t lds;
    align_long_class_geometry(cls, &pmax, &stride, &apb, &lds);
    const dim3 grid((n + apb - 1u) / apb), block(apb * (byte ? 16u : 8u));
    if (lds > (size_t)ALNL_LDS_CEILING) return hipErrorInvalidValue;
    if (lds > (64u << 10)) {                          /* (8-bit mode beyond 2 048 bases, 16-bit mode beyond 1 024) */
        const hipError_t he = byte ? align_long_lds_attr<true>() : align_long_lds_attr<false>();
        if (he != hipSuccess) return he;
    }
    if (byte) hipLaunchKernelGGL((bsw_align_long_kernel<true>), grid, block, lds, s, P, seq, tasks, order, n, blist, out, pmax, stride);
    else hipLaunchKernelGGL((bsw_align_long_kernel<false>), grid, block, lds, s, P, seq, tasks, order, n, blist, out, pmax, stride);
    return hipGetLastError();
}

}  // namespace bsw
