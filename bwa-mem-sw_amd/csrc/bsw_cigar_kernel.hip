/*
 * bsw_cigar_kernel.hip — gfx950 kernel of bwa_gen_cigar2's last step (bwa.c): NM and the MD string from the CIGAR that
 * bsw_global_kernel / bsw_global_long_kernel left on the device, the packed read and the target fetched from the resident
 * reference (bsw_cigar.hip is the host side).  It also settles bwa's no-gap shortcut (l_query == re - rb and w_ == 0):
 * CIGAR l_query M and the score sum(mat[rseq[i] * 5 + query[i]]), no DP.
 *
 * One wavefront per alignment (a workgroup of 64 lanes).  The CIGAR ops are walked in order, the same op by every lane:
 *   M  in steps of 1 024 bases, 16 per lane: the lane's 16 read and 16 target nibbles come out of two words each by a
 *      funnel shift, their XOR marks the mismatches (one bit per nibble), a ballot skips the step when nothing
 *      mismatches — the common case — and otherwise every mismatch becomes an MD token digits(u) + letter.  u (the match
 *      run before it) is the distance to the previous mismatch: inside a lane by a bit scan, across lanes through the
 *      ballot (the closest lower lane with a mismatch hands over the end of its last one), across steps in a uniform
 *      register.  An exclusive prefix sum of the lanes' token bytes places every token;
 *   D  not first and not last: the token digits(u) '^' + the deleted target bases, 64 lanes writing 64 letters at a time;
 *      a leading or trailing D only moves along the target (bwa counts it in neither NM nor MD);
 *   I  moves along the read and counts in NM.
 * The tokens of a step are assembled in 4 KiB of LDS and then copied into the task's MD slot with lane-consecutive byte
 * stores (a wavefront's store covers 64 consecutive bytes).  Bytes past max_md - 1 are never written; an MD that did not
 * fit leaves "" in the slot and md_len = -(bytes needed, NUL included).
 * A CIGAR that overflowed max_cigar (n_cigar < 0) has no NM / MD: nm = -1, md_len = 0, "".
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bsw_device.h"
#include "bsw_stage.h"

namespace bsw {

namespace {

constexpr int MD_BUF = 4096;       /* LDS bytes per wavefront: the tokens of one step (an M step produces at most ~2 060) */
constexpr int MD_STEP = 1024;      /* M bases per step: 16 per lane */
constexpr int DEL_STEP = 2048;     /* deleted bases per step */

__device__ __forceinline__ int ndigits(int u)
{
    int d = 1;
    for (uint64_t t = 10; d < 10 && (uint64_t)u >= t; t *= 10) ++d;
    return d;
}

__device__ __forceinline__ void put_dec(char *b, int u, int nd)
{
    for (int d = nd - 1; d >= 0; --d) {
        b[d] = (char)('0' + u % 10);
        u /= 10;
    }
}

/* the 16 nibbles of a packed sequence (nw words at seq + off) starting at base pos; words past the sequence read as 0 */
__device__ __forceinline__ uint64_t nib16(const uint64_t *__restrict__ seq, const uint32_t off, const int nw, const int pos)
{
    const int wi = pos >> 4, sh = (pos & 15) * 4;
    const uint64_t lo = wi < nw ? seq[off + (uint32_t)wi] : 0ull;
    const uint64_t hi = (sh && wi + 1 < nw) ? seq[off + (uint32_t)wi + 1u] : 0ull;
    return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

__device__ __forceinline__ int wave_incl_sum(int v, const int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ char base_letter(const uint64_t tab, int code)
{
    code = code < 4 ? code : 4;
    return (char)((tab >> (8 * code)) & 0xff);
}

}  // namespace

__global__ __launch_bounds__(64) void bsw_cigar_md_kernel(const bsw_dparams P, const uint64_t *__restrict__ seq,
                                                          const bsw_cdtask *__restrict__ tasks, const uint32_t n,
                                                          uint32_t *__restrict__ cigars, const int max_cigar,
                                                          const bsw_gresult *__restrict__ gres, char *__restrict__ md,
                                                          const int max_md, bsw_cresult *__restrict__ res)
{
    __shared__ char buf[MD_BUF];
    __shared__ int8_t smat[25];
    const int lane = threadIdx.x;
    const uint32_t ti = blockIdx.x;
    if (ti >= n) return;                                     /* (whole workgroup) */
#pragma unroll
    for (int k = 0; k < 25; ++k)
        if (lane == k) smat[k] = P.mat[k];
    const bsw_cdtask T = tasks[ti];
    char *slot = md ? md + (size_t)ti * (size_t)max_md : nullptr;
    uint32_t *cg = cigars + (size_t)ti * (size_t)max_cigar;
    const bool nogap = (T.flags & BSW_CD_NOGAP) != 0;
    int score = 0, n_cigar = 0;
    if (T.flags & BSW_CD_STATUS) n_cigar = -1;               /* (no alignment: the empty record below) */
    else if (nogap) {
        n_cigar = 1;
        if (lane == 0) cg[0] = (uint32_t)T.qlen << 4;
    } else {
        const bsw_gresult g = gres[ti];
        score = g.score;
        n_cigar = g.n_cigar;
    }
    if (n_cigar < 0) {
        if (lane == 0) {
            bsw_cresult r;
            r.score = (T.flags & BSW_CD_STATUS) ? 0 : score;
            r.n_cigar = (T.flags & BSW_CD_STATUS) ? 0 : n_cigar;
            r.nm = -1; r.md_len = 0; r.w = 0; r.tries = 0; r.status = 0; r._pad = 0;
            res[ti] = r;
            if (slot) slot[0] = 0;
        }
        return;
    }
    __syncthreads();                                         /* smat */
    const uint64_t tab = (T.flags & BSW_CD_REV) ? 0x4e41434754ull /* "TGCAN" */ : 0x4e54474341ull /* "ACGTN" */;
    const int nwq = (T.qlen + 15) >> 4, nwt = (T.tlen + 15) >> 4;
    const int lim = max_md - 1;                              /* bytes of the slot that may hold letters */
    int x = 0, y = 0, mbase = 0, last_end = 0, nm = 0, out = 0;   /* wave-uniform; mbase: M bases so far, last_end: where u starts */
    int sc = 0;                                              /* no-gap shortcut: this lane's part of the score */

    auto flush = [&](int total) {                            /* buf[0, total) -> slot[out, out + total) */
        __syncthreads();
        if (slot)
            for (int i = lane; i < total; i += 64)
                if (out + i < lim) slot[out + i] = buf[i];
        out += total;
        __syncthreads();
    };

    for (int k = 0; k < n_cigar; ++k) {
        const uint32_t word = nogap ? ((uint32_t)T.qlen << 4) : cg[k];
        const int op = (int)(word & 0xf), len = (int)(word >> 4);
        if (op == 0) {
            for (int c0 = 0; c0 < len; c0 += MD_STEP) {
                const int b = c0 + 16 * lane;
                const int nb = min(max(len - b, 0), 16);
                uint64_t mm = 0, tv = 0;
                if (nb > 0) {
                    const uint64_t qv = nib16(seq, T.q_off, nwq, x + b);
                    tv = nib16(seq, T.t_off, nwt, y + b);
                    uint64_t d = qv ^ tv;                    /* codes are 0..4: three bits per nibble */
                    d = (d | (d >> 1) | (d >> 2)) & 0x1111111111111111ull;
                    if (nb < 16) d &= (1ull << (4 * nb)) - 1ull;
                    mm = d;
                    if (nogap)
                        for (int i = 0; i < nb; ++i) {
                            const int tb = min((int)((tv >> (4 * i)) & 7), 4), qb = min((int)((qv >> (4 * i)) & 7), 4);
                            sc += smat[tb * 5 + qb];
                        }
                }
                const uint64_t any = __ballot(mm != 0);
                if (any) {
                    const int p0 = mbase + b;                /* M index of this lane's first base */
                    const int my_end = mm ? p0 + (63 - __clzll((long long)mm)) / 4 + 1 : 0;
                    const uint64_t below = any & ((1ull << lane) - 1ull);
                    const int from = below ? 63 - __clzll((long long)below) : lane;
                    const int pe = __shfl(my_end, from, 64);
                    const int prev = below ? pe : last_end;
                    int nbytes = 0;
                    {
                        int pv = prev;
                        for (uint64_t m = mm; m; m &= m - 1ull) {
                            const int p = p0 + (__ffsll((long long)m) - 1) / 4;
                            nbytes += ndigits(p - pv) + 1;
                            pv = p + 1;
                        }
                    }
                    const int incl = wave_incl_sum(nbytes, lane);
                    const int total = __shfl(incl, 63, 64);
                    {
                        int pos = incl - nbytes, pv = prev;
                        for (uint64_t m = mm; m; m &= m - 1ull) {
                            const int kk = (__ffsll((long long)m) - 1) / 4;
                            const int p = p0 + kk, u = p - pv, nd = ndigits(u);
                            if (pos + nd < MD_BUF) {
                                put_dec(buf + pos, u, nd);
                                buf[pos + nd] = base_letter(tab, (int)((tv >> (4 * kk)) & 7));
                            }
                            pos += nd + 1;
                            pv = p + 1;
                        }
                    }
                    last_end = __shfl(my_end, 63 - __clzll((long long)any), 64);
                    const int cnt = __popcll(mm);
                    nm += __shfl(wave_incl_sum(cnt, lane), 63, 64);
                    flush(min(total, MD_BUF));
                }
            }
            x += len; y += len; mbase += len;
        } else if (op == 2) {
            if (k > 0 && k < n_cigar - 1) {                  /* a leading or trailing D is in neither MD nor NM */
                const int u = mbase - last_end, nd = ndigits(u);
                for (int c0 = 0; c0 < len; c0 += DEL_STEP) {
                    const int h = c0 == 0 ? nd + 1 : 0;
                    if (c0 == 0 && lane == 0) {
                        put_dec(buf, u, nd);
                        buf[nd] = '^';
                    }
                    const int cnt = min(len - c0, DEL_STEP);
                    for (int i = lane; i < cnt; i += 64) {
                        const int pos = y + c0 + i, wi = pos >> 4;
                        const uint64_t v = wi < nwt ? seq[T.t_off + (uint32_t)wi] : 0ull;
                        buf[h + i] = base_letter(tab, (int)((v >> (4 * (pos & 15))) & 7));
                    }
                    flush(h + cnt);
                }
                last_end = mbase;
                nm += len;
            }
            y += len;
        } else if (op == 1) {
            x += len;
            nm += len;
        }
    }
    {
        const int u = mbase - last_end, nd = ndigits(u);
        if (lane == 0) put_dec(buf, u, nd);
        flush(nd);
    }
    if (nogap) score = __shfl(wave_incl_sum(sc, lane), 63, 64);
    if (lane == 0) {
        bsw_cresult r;
        r.score = score;
        r.n_cigar = n_cigar;
        r.nm = nm;
        r.md_len = out;
        if (slot) {
            if (out < max_md) slot[out] = 0;
            else { slot[0] = 0; r.md_len = -(out + 1); }
        }
        r.w = 0;
        r.tries = nogap ? ((T.more && score < T.min_score) ? 2 : 1) : 0;
        r.status = 0;
        r._pad = 0;
        res[ti] = r;
    }
}

hipError_t launch_cigar_md(const bsw_dparams &P, const uint64_t *seq, const bsw_cdtask *tasks, uint32_t n, uint32_t *cigars, int max_cigar,
                           const bsw_gresult *gres, char *md, int max_md, bsw_cresult *res, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bsw_cigar_md_kernel, dim3(n), dim3(64), 0, s, P, seq, tasks, n, cigars, max_cigar, gres, md, max_md, res);
    return hipGetLastError();
}

}  // namespace bsw
