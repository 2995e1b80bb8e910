/*
 * bsw_global_long_kernel.hip — gfx950 kernel for SURVEY.md §8f row F4 beyond the register kernel: bwa's banded GLOBAL
 * alignment with CIGAR (ksw_global2) for queries of 1 024 to 8 191 bases, and for every length under BSW_GLOBAL_LONG=1.
 * Parity anchor as for bsw_global_kernel.hip: oracle/ksw_global_ref.c, score and CIGAR operation by operation.
 *
 * bsw_global_kernel.hip keeps the eh[] row in registers, lane l on the FIXED columns l*C .. l*C + C - 1; at 1 024 columns
 * the registers end (the wall bsw_wave_kernel.hip met, which bsw_long_kernel.hip got past).  Here, as in bsw_long_kernel.hip,
 * ONE WAVEFRONT PER ALIGNMENT and lane l of chunk c works on column  beg + 64 c + l  of the current row: the lanes follow
 * [beg, end] along the diagonal, a row runs (end - beg) / 64 + 1 chunks (the entry eh[end] included), and the row lives in LDS.
 *   - eh[] is a RING of R records {h, e} (R a power of two >= n_col + 1, n_col = min(qlen, 2w+1)), column j at slot j & (R-1).
 *     A row reads eh[beg .. end-1] and writes eh[beg .. end]; every column it reads was written by the row before (or is a
 *     first-row entry, j <= min(w, qlen) < R), and the end - beg + 1 <= n_col + 1 columns of a row never share a slot.  So
 *     the LDS a wave needs follows the band, not the query: bwa_gen_cigar2's narrow bands run several waves per CU.  Lanes
 *     past eh[end] read a slot (always inside the ring) and never write it.
 *   - the query stays packed (16 bases per 64-bit word) in LDS after the ring; a row's score of column j is one byte of a
 *     per-row 4 x int8 word for query bases ACGT (or the row's score against a query N).
 *   - F(i,j) is an exclusive prefix max of G_j = M_j - oe_ins + (j - beg) e_ins (the column offset from beg, not j: keeps the
 *     scan input away from INT_MIN): one 6-step DPP scan per chunk, the carry between chunks a scalar;
 *     F(i,j) = max(G_pex, MINUS_INF - e_ins) - (j - beg - 1) e_ins, i.e. f enters column beg as MINUS_INF.
 *   - H(i,j-1) for eh[j].h is one wave_shr:1 (lane 0: the previous chunk's last column, or h1_init at beg).
 *   - the direction byte h | e<<2 | f<<4 goes to z row i at column j - beg: 64 consecutive bytes per chunk.
 * int32 bounds (qlen <= 8191, tlen <= 65535, w <= 65535, o+e <= 4096 as check_params enforces, |mat| <= 128): E(i,j) >=
 * MINUS_INF - tlen e_del >= -2^30 - 2^28; H >= E; h1_init and the first row >= -(4096 + 4096 * 65536) > -2^29; so every M,
 * E, H >= -1.35e9, G >= M - 4096 and F >= G_min - 8191 * 4096 = -1.39e9 > INT_MIN; from above G <= 127 * 8191 + 8191 * 4096.
 * The scan's identity INT_MIN is below all of them.
 *
 * Traceback: the walk is wave-uniform (SALU plus one LDS byte per step).  z is staged through LDS in tiles of 32 rows x 64
 * columns around the current cell (32 coalesced byte loads per lane, all in flight at once), reusing the ring's bytes; a
 * path near the diagonal crosses a tile in about 32 steps, so a long walk pays one HBM latency per ~32 steps instead of
 * one per step.  Tile positions outside the matrix (column < 0 or >= n_col, row < 0) hold 0: a step whose column lies outside
 * the band matrix reads as "diagonal", the register kernel's convention.
 */
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include <atomic>

#include "bsw_band_scan.h"
#include "bsw_device.h"
#include "bsw_global_core.h"
#include "bsw_stage.h"

namespace bsw {

namespace {

constexpr int LMINF = -0x40000000;                     /* bwa's MINUS_INF */
constexpr int TILE_R = 32, TILE_C = 64;                /* traceback tile: rows x z columns */
constexpr int QWORDS = (BSW_MAX_QLEN + 15) / 16;       /* packed query words per wave */
constexpr int MIN_RING = TILE_R * TILE_C / 8;          /* ring records that hold one tile */

}  // namespace

/* ring = eh[] records per wave (a power of two >= n_col + 1 of every task of the launch, >= MIN_RING) */
template <int WPB>
__global__ __launch_bounds__(64 * WPB) void bsw_global_long_kernel(const bsw_dparams P, const uint64_t *__restrict__ seq,
                                                                const bsw_gdtask *__restrict__ tasks,
                                                                const uint32_t *__restrict__ order, const uint32_t n,
                                                                const int ring, uint8_t *__restrict__ z,
                                                                uint32_t *__restrict__ cigars, const int max_cigar,
                                                                bsw_gresult *__restrict__ out)
{
    extern __shared__ uint2 glong_lds[];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t slot = blockIdx.x * (uint32_t)WPB + (uint32_t)wv;
    if (slot >= n) return;
    uint2 *eh = glong_lds + (size_t)wv * (size_t)(ring + QWORDS);
    uint2 *qry = eh + ring;
    const int rmask = ring - 1;
    const uint32_t ti = order[slot];
    const bsw_gdtask T = tasks[ti];
    const int qlen = T.qlen, tlen = T.tlen, w = T.w;
    const int o_del = P.o_del, e_del = P.e_del, o_ins = P.o_ins, e_ins = P.e_ins;
    const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
    const int n_col = qlen < 2 * w + 1 ? qlen : 2 * w + 1;
    uint8_t *zt = z ? z + T.z_off : nullptr;

    /* per target base: the scores against query bases ACGT packed 4 x int8, and against a query N */
    uint32_t rp[5];
    int rn[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        rp[t] = (uint32_t)(uint8_t)P.mat[t * 5] | ((uint32_t)(uint8_t)P.mat[t * 5 + 1] << 8) |
                ((uint32_t)(uint8_t)P.mat[t * 5 + 2] << 16) | ((uint32_t)(uint8_t)P.mat[t * 5 + 3] << 24);
        rn[t] = P.mat[t * 5 + 4];
    }

    const int nqw = (qlen + 15) >> 4;
    for (int k = lane; k < nqw; k += 64) {
        const uint64_t v = seq[T.q_off + (uint32_t)k];
        qry[k] = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
    }
    /* first row: eh[0] = {0,-inf}; eh[j].h = -(o_ins + e_ins*j) inside the band, -inf outside (only j <= min(w, qlen) is read) */
    for (int j = lane; j < ring; j += 64) {
        const int x = j == 0 ? 0 : (j <= w && j <= qlen ? -(o_ins + e_ins * j) : LMINF);
        eh[j] = make_uint2((uint32_t)x, (uint32_t)LMINF);
    }
    int score = qlen == 0 ? 0 : (qlen <= w ? -(o_ins + e_ins * qlen) : LMINF);      /* eh[qlen].h */

    const int ntw = (tlen + 15) >> 4;
    uint32_t twl = 0, twh = 0, cur_lo = 0, cur_hi = 0;
    for (int i = 0; i < tlen; ++i) {
        const int tb = target_base(seq, T.t_off, ntw, i, lane, twl, twh, cur_lo, cur_hi);
        uint32_t rowp = rp[4];
        int rowq = rn[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            rowp = tb == t ? rp[t] : rowp;
            rowq = tb == t ? rn[t] : rowq;
        }
        const int beg = i > w ? i - w : 0;
        const int end = i + w + 1 < qlen ? i + w + 1 : qlen;
        const int h1_init = beg == 0 ? -(o_del + e_del * (i + 1)) : LMINF;
        if (end < beg) {                                     /* the band has left the query: only eh[end] = eh[qlen] is written */
            if (lane == 0) eh[end & rmask] = make_uint2((uint32_t)h1_init, (uint32_t)LMINF);
            score = h1_init;
            continue;
        }
        uint8_t *zi = zt ? zt + (size_t)i * (size_t)n_col : nullptr;
        int carry = INT_MIN;                                 /* max G of every column left of the chunk */
        int hprev = 0;                                       /* H(i, j-1) entering the chunk */
        int hlast = h1_init;                                 /* eh[end].h */
        const int nchunk = ((end - beg) >> 6) + 1;
        for (int c = 0; c < nchunk; ++c) {
            const int r = 64 * c + lane, j = beg + r;
            const uint2 rec = eh[j & rmask];
            int X = (int)rec.x, E = (int)rec.y;
            const bool inr = j < end, wr = j <= end;
            const int jq = inr ? j : 0;
            const uint2 qw = qry[jq >> 4];
            const int qb = (int)((((jq & 8) ? qw.y : qw.x) >> ((jq & 7) * 4)) & 7);
            const int s = qb < 4 ? (int)(int8_t)(rowp >> (qb * 8)) : rowq;
            const int m = X + s;
            const int g = inr ? m - oe_ins + r * e_ins : INT_MIN;
            const int incl = wave_scan_max(g);
            const int pex = max(max(dpp_mov<0x138>(INT_MIN, incl), carry), LMINF - e_ins);  /* wave_shr:1 -> exclusive */
            const int f = pex - (r - 1) * e_ins;
            int h, en;
            uint32_t d;
            global_cell(m, E, f, oe_del, e_del, oe_ins, e_ins, h, en, d);
            if (zi && inr) zi[r] = (uint8_t)d;
            E = inr ? en : E;
            /* eh[j].h <- H(i,j-1) for j in [beg,end]; eh[end].e <- -inf */
            const int hp = dpp_mov<0x138>(hprev, h);
            X = j == beg ? h1_init : hp;
            E = j == end ? LMINF : E;
            if (wr) eh[j & rmask] = make_uint2((uint32_t)X, (uint32_t)E);
            carry = max(carry, __builtin_amdgcn_readlane(incl, 63));
            hprev = __builtin_amdgcn_readlane(h, 63);
            if ((unsigned)(end - beg - 64 * c) < 64u) hlast = __builtin_amdgcn_readlane(X, end - beg - 64 * c);
        }
        if (end == qlen) score = hlast;
    }

    int n_cigar = 0;
    if (zt) {                                                /* backtrack from the last cell, ops pushed in reverse */
        __threadfence();                                     /* the wave's z stores are visible to its loads */
        uint8_t *tile = (uint8_t *)eh;                       /* the ring is dead: TILE_R x TILE_C bytes */
        cigar_writer cw{cigars + (size_t)ti * (size_t)max_cigar, max_cigar, lane == 0};
        int which = 0, i = tlen - 1, k = (i + w + 1 < qlen ? i + w + 1 : qlen) - 1;
        int tr0 = i + 1, tc0 = 0;                            /* tile origin (row, z column); none loaded yet */
        while (i >= 0 && k >= 0) {
            const int col = k - (i > w ? i - w : 0);
            if ((unsigned)(i - tr0) >= (unsigned)TILE_R || (unsigned)(col - tc0) >= (unsigned)TILE_C) {
                tr0 = i - (TILE_R - 1);
                tc0 = col - TILE_C / 2;
                const int cc = tc0 + lane;
                uint8_t v[TILE_R];
#pragma unroll
                for (int rr = 0; rr < TILE_R; ++rr) {
                    const int row = tr0 + rr;
                    v[rr] = (row >= 0 && cc >= 0 && cc < n_col) ? zt[(size_t)row * (size_t)n_col + (size_t)cc] : (uint8_t)0;
                }
#pragma unroll
                for (int rr = 0; rr < TILE_R; ++rr) tile[rr * TILE_C + lane] = v[rr];
            }
            const int d = __builtin_amdgcn_readfirstlane((int)tile[(i - tr0) * TILE_C + (col - tc0)]);
            which = (d >> (which << 1)) & 3;
            if (which == 0) { cw.push(0u, 1); --i; --k; }
            else if (which == 1) { cw.push(2u, 1); --i; }
            else { cw.push(1u, 1); --k; }
        }
        n_cigar = cw.finish(i, k);
    }
    if (lane == 0) {
        bsw_gresult res;
        res.score = score;
        res.n_cigar = n_cigar;
        out[ti] = res;
    }
}

template <int WPB>
static hipError_t launch_gl(int ring, const bsw_dparams &P, const uint64_t *seq, const bsw_gdtask *tasks, const uint32_t *order,
                            uint32_t n, uint8_t *z, uint32_t *cigars, int max_cigar, bsw_gresult *out, hipStream_t s)
{
    const size_t lds = (size_t)(ring + QWORDS) * sizeof(uint2) * (size_t)WPB;
    static std::atomic<uint64_t> lds_set_on{0};              /* per instantiation (set_lds_ceiling, bsw_band_scan.h) */
    const hipError_t attr = set_lds_ceiling(reinterpret_cast<const void *>(&bsw_global_long_kernel<WPB>), 160 * 1024, lds_set_on);
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL((bsw_global_long_kernel<WPB>), dim3((n + (uint32_t)WPB - 1u) / (uint32_t)WPB), dim3(64 * WPB), lds, s,
                       P, seq, tasks, order, n, ring, z, cigars, max_cigar, out);
    return hipGetLastError();
}

/* Up to 4 096 ring records four wavefronts share a workgroup's LDS (4 x (4 096 + 512) x 8 B = 144 KiB); the 8 192-record
 * class (full width near 8 191 columns, 68 KiB) runs one wavefront per workgroup, two workgroups per CU. */
hipError_t launch_global_long(int cls, const bsw_dparams &P, const uint64_t *seq, const bsw_gdtask *tasks, const uint32_t *order,
                              uint32_t n, uint8_t *z, uint32_t *cigars, int max_cigar, bsw_gresult *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const int ring = 256 << cls;                             /* global_long_class_of (bsw_stage.h) */
    static_assert(256 >= MIN_RING, "the smallest ring must hold a traceback tile");
    if (ring <= 4096) return launch_gl<4>(ring, P, seq, tasks, order, n, z, cigars, max_cigar, out, s);
    return launch_gl<1>(ring, P, seq, tasks, order, n, z, cigars, max_cigar, out, s);
}

}  // namespace bsw
