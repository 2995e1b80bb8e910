/*
 * bsw_c2a_core.h — mem_chain2aln's seed loop for ONE READ, stated once for the device (bsw_c2a_replay_kernel.hip, under hipcc) and
 * for the CPU (the stand-in launcher and tests/c2a_core_model.cpp, under g++ / clang++).  It is bsw_chain2aln.c's c2a_replay_range
 * restated so that a group of lanes can walk it together; its results are that routine's, byte for byte.
 *
 * A policy P hides what differs between the two:
 *     P::W                 lanes that walk one read together (device: a 16-lane DPP row; CPU: 1)
 *     lane()               this lane's index in the group, 0 .. W-1
 *     any(b)               does any lane of the group hold b
 *     max_u64(v), sum_u32(v)   reductions over the group, the result in every lane
 *     clear() / set(i) / get(i)   the per-seed state of the chain at hand, kept by seed i's OWNER, lane i % W
 * Everything outside the strided loops is uniform over the group, so every lane reaches every vote.
 *
 * What is kept exactly:
 *   visit order    srt[] of the host is never built.  The keys (score << 32 | index) are unique, so "the next seed" is the largest
 *                  key below the current one and "visited earlier" is "larger key"; n selections of n / W steps each.
 *   skip mark      bwa's value 0 in srt[] becomes a state per seed: only "extended" is ever asked for (an unvisited seed has a
 *                  smaller key and is filtered by the key test; a skipped one is not extended).  The (score 0, index 0) entry that
 *                  bwa reads as skipped has the smallest key of all: it is visited last and no seed's un-skip test looks below its
 *                  own key, so the quirk cannot be observed and needs no case here.
 *   binary64       len - seedlen0 > seedlen0_frac * l_query and t.len < s.len * ovl_len_frac: ints converted exactly, ONE multiply,
 *                  a compare — no add, so nothing for the compiler to contract; never binary32.  bsw_cal_max_gap as bsw_glue.c
 *                  writes it: an IEEE binary64 division (this unit is built without fast-math), + 1., truncation.
 *   (int)rd        in qd < rd ? qd : (int)rd, kept as written; rb / re / rbeg are 64 bits throughout.
 *   seedcov        a sum over ALL seeds of the chain in uint32 wrap-around arithmetic: any order of the partial sums gives the bits
 *                  of the host's int32 loop.
 * Region j of a read is WRITTEN by lane j % W and only ever READ BACK by that lane (the explains vote strides the same way), and a
 * seed's flag byte is written by its owner alone: every read-after-write through memory is one thread's own.
 */
#ifndef BSW_C2A_CORE_H
#define BSW_C2A_CORE_H

#include <stdint.h>
#include <string.h>

#include "../../include/bwa_sw_mi355.h"

#if defined(__HIPCC__)
#define C2A_HD __host__ __device__
#else
#define C2A_HD
#endif

/* A read with a chain of more seeds than this is replayed on the host (reads are independent, so that is exact).  It protects the
 * per-seed state of a row — one bit per owned seed in ONE 32-bit register per lane, 16 x 32 — and bounds what one row can cost its
 * wavefront: the selection is n^2 / 16 key tests per chain, 16 384 at the cap, while the three other rows of the wavefront wait. */
#define BSW_C2A_DEV_MAX_CHAIN 512

/* compact records of a chunk: indices are LOCAL to the chunk's seeds and chains but for `chain` and `read` */
typedef struct c2a_dchain {
    uint32_t seed0;                  /* the chain's seeds: chunk seeds [seed0, seed0 + n_seeds) */
    int32_t  n_seeds;
    int32_t  l_query;
    int32_t  rid;
    float    frac_rep;
    uint32_t read, chain;            /* global indices, copied into the regions */
    uint32_t _pad;
} c2a_dchain;                        /* 32 bytes */
typedef struct c2a_dread {
    uint32_t chain0, n_chains;       /* chunk chains [chain0, chain0 + n_chains) */
    uint32_t seed0, n_seeds;         /* all seeds of the read; its regions are staged at [seed0, ...) */
    uint32_t host, _pad;             /* 1: a chain above BSW_C2A_DEV_MAX_CHAIN — the host replays the read, the kernel only clears its flags */
} c2a_dread;                         /* 24 bytes */
typedef struct c2a_dpar {            /* what bsw_cal_max_gap reads of bsw_params, and bsw_c2a_opt */
    int32_t a, o_del, e_del, o_ins, e_ins, w;
    double  seedlen0_frac, ovl_len_frac;
} c2a_dpar;

/* One launch: the replay kernel over n_reads rows, then the scan of their counts and the move that leaves the chunk's regions
 * compact and in read order in `out`.  Every pointer is device memory. */
typedef struct c2a_dev_args {
    const c2a_dread *reads;
    uint32_t n_reads;
    const c2a_dchain *chains;
    const bsw_cseed *seeds;          /* the chunk's seeds */
    uint32_t seed_base;              /* global index of the chunk's first seed */
    const void *results;             /* the chunk's result records ... */
    uint32_t stride;                 /* ... 32 (bsw_pair) or 96 (bsw_result) bytes apart: only the head is read */
    c2a_dpar par;
    bsw_creg *stage;                 /* [seeds]: read r's regions from stage[reads[r].seed0] on, in push order */
    bsw_creg *out;                   /* [seeds]: the same, compact */
    uint32_t *counts;                /* [n_reads] */
    uint32_t *offs;                  /* [n_reads + 1]: exclusive prefix sums of counts; offs[n_reads] = the chunk's regions */
    uint8_t *flags;                  /* [seeds]: 1 where bwa runs the extension */
} c2a_dev_args;
/* the table the companion library (or a stand-in) hands to the main one; launch answers a hipError_t as an int */
typedef struct c2a_dev_ops {
    int (*launch)(const c2a_dev_args *a, void *stream);
} c2a_dev_ops;

C2A_HD inline int c2a_cal_max_gap(const c2a_dpar &p, int qlen)
{
    const int l_del = (int)((double)(qlen * p.a - p.o_del) / p.e_del + 1.);
    const int l_ins = (int)((double)(qlen * p.a - p.o_ins) / p.e_ins + 1.);
    int l = l_del > l_ins ? l_del : l_ins;
    if (l < 1) l = 1;
    return l < (p.w << 1) ? l : (p.w << 1);
}

/* does region r explain seed s (bsw_chain2aln.c: c2a_explains) */
C2A_HD inline bool c2a_explains(const c2a_dpar &p, const bsw_creg &r, const bsw_cseed &s, int l_query)
{
    int64_t rd;
    int qd, w, g;
    if (s.rbeg < r.rb || s.rbeg + s.len > r.re || s.qbeg < r.qb || s.qbeg + s.len > r.qe) return false;
    if (p.seedlen0_frac >= 0 && (double)(s.len - r.seedlen0) > p.seedlen0_frac * (double)l_query) return false;
    qd = s.qbeg - r.qb; rd = s.rbeg - r.rb;
    g = c2a_cal_max_gap(p, qd < rd ? qd : (int)rd);
    w = g < r.w ? g : r.w;
    if (qd - rd < w && rd - qd < w) return true;
    qd = r.qe - (s.qbeg + s.len); rd = r.re - (s.rbeg + s.len);
    g = c2a_cal_max_gap(p, qd < rd ? qd : (int)rd);
    w = g < r.w ? g : r.w;
    return qd - rd < w && rd - qd < w;
}

/* may the long seed t, extended earlier, un-skip s */
C2A_HD inline bool c2a_unskips(const c2a_dpar &p, const bsw_cseed &t, const bsw_cseed &s)
{
    if ((double)t.len < (double)s.len * p.ovl_len_frac) return false;
    if (s.qbeg <= t.qbeg && s.qbeg + s.len - t.qbeg >= s.len >> 2 && t.qbeg - s.qbeg != t.rbeg - s.rbeg) return true;
    if (t.qbeg <= s.qbeg && t.qbeg + t.len - s.qbeg >= s.len >> 2 && s.qbeg - t.qbeg != s.rbeg - t.rbeg) return true;
    return false;
}

/* key + 1 of seed i, so that 0 means "none" (scores are >= 0 and below 2^31) */
C2A_HD inline uint64_t c2a_key1(const bsw_cseed *cs, uint32_t i) { return ((uint64_t)(uint32_t)cs[i].score << 32 | i) + 1; }

/* The replay of one read: its chains ch[0 .. n_chains) over the chunk's seeds and records.  Regions go to out[0 ..) in push order;
 * returns their number (the same in every lane).  flags (may be NULL): the chunk's flag bytes; the read's are cleared here. */
template <class P>
C2A_HD inline uint32_t c2a_replay_read(P &pol, const c2a_dpar &par, const c2a_dchain *ch, uint32_t n_chains, const bsw_cseed *seeds, uint32_t seed_base,
                                       const char *results, uint32_t stride, bsw_creg *out, uint8_t *flags)
{
    const uint32_t W = (uint32_t)P::W, lane = pol.lane();
    uint32_t nreg = 0;
    for (uint32_t c = 0; c < n_chains; ++c) {
        const c2a_dchain k = ch[c];
        const bsw_cseed *cs = seeds + k.seed0;
        const uint32_t n = (uint32_t)k.n_seeds;
        uint64_t bound = UINT64_MAX;
        pol.clear();
        if (flags)
            for (uint32_t i = lane; i < n; i += W) flags[k.seed0 + i] = 0;
        for (uint32_t step = 0; step < n; ++step) {
            uint64_t best = 0;
            for (uint32_t i = lane; i < n; i += W) {
                const uint64_t key = c2a_key1(cs, i);
                if (key < bound && key > best) best = key;
            }
            best = pol.max_u64(best);
            if (!best) break;                        /* (n unique keys, n selections: never; it keeps the index below in bounds whatever happens) */
            bound = best;
            const uint32_t si = (uint32_t)(best - 1);
            const bsw_cseed s = cs[si];
            bool hit = false;
            for (uint32_t j = lane; j < nreg; j += W) hit |= c2a_explains(par, out[j], s, k.l_query);
            if (pol.any(hit)) {                      /* explained: unless a long seed visited earlier, and extended, overlaps it on another diagonal */
                bool un = false;
                for (uint32_t i = lane; i < n; i += W)
                    if (c2a_key1(cs, i) > best && pol.get(i)) un |= c2a_unskips(par, cs[i], s);
                if (!pol.any(un)) continue;
            }
            bsw_pair r;
            memcpy(&r, results + (size_t)(k.seed0 + si) * stride, sizeof(r));
            bsw_creg a;
            a.rb = s.rbeg + r.rb;              a.re = s.rbeg + s.len + r.re;
            a.qb = r.qb;                       a.qe = s.qbeg + s.len + r.qe;
            a.score = r.score; a.truesc = r.truesc; a.w = r.w;
            uint32_t cov = 0;
            for (uint32_t i = lane; i < n; i += W)
                if (cs[i].qbeg >= a.qb && cs[i].qbeg + cs[i].len <= a.qe && cs[i].rbeg >= a.rb && cs[i].rbeg + cs[i].len <= a.re) cov += (uint32_t)cs[i].len;
            a.seedcov = (int32_t)pol.sum_u32(cov);
            a.seedlen0 = s.len;
            a.rid = k.rid; a.frac_rep = k.frac_rep;
            a.read = k.read; a.chain = k.chain; a.seed = seed_base + k.seed0 + si;
            if (nreg % W == lane) out[nreg] = a;
            if (si % W == lane) {
                pol.set(si);
                if (flags) flags[k.seed0 + si] = 1;
            }
            ++nreg;
        }
    }
    return nreg;
}

/* the CPU policy: one lane does everything; the state is a byte per seed of the longest chain it may meet */
struct c2a_cpu_policy {
    enum { W = 1 };
    uint8_t *state;
    uint32_t cap;
    uint32_t lane() const { return 0; }
    bool any(bool b) const { return b; }
    uint64_t max_u64(uint64_t v) const { return v; }
    uint32_t sum_u32(uint32_t v) const { return v; }
    void clear() { memset(state, 0, cap); }
    void set(uint32_t i) { state[i] = 1; }
    bool get(uint32_t i) const { return state[i] != 0; }
};

/* a whole launch on the CPU (the stand-in launcher, the model test): what the three kernels leave in a's arrays */
inline void c2a_cpu_launch(const c2a_dev_args *a)
{
    uint8_t state[BSW_C2A_DEV_MAX_CHAIN];
    uint32_t at = 0;
    for (uint32_t r = 0; r < a->n_reads; ++r) {
        const c2a_dread rd = a->reads[r];
        uint32_t cnt = 0;
        if (rd.host) {
            if (a->flags && rd.n_seeds) memset(a->flags + rd.seed0, 0, rd.n_seeds);
        } else {
            c2a_cpu_policy pol{state, BSW_C2A_DEV_MAX_CHAIN};
            cnt = c2a_replay_read(pol, a->par, a->chains + rd.chain0, rd.n_chains, a->seeds, a->seed_base, (const char *)a->results, a->stride,
                                  a->stage + rd.seed0, a->flags);
        }
        a->counts[r] = cnt;
        a->offs[r] = at;
        if (cnt) memmove(a->out + at, a->stage + rd.seed0, (size_t)cnt * sizeof(bsw_creg));
        at += cnt;
    }
    a->offs[a->n_reads] = at;
}

#endif
