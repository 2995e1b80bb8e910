/*
 * bsw_rescue.c — the mate-rescue loop of mem_sam_pe with mem_matesw inside it, as a resumable replay (host, plain C, no context).
 * bwamem_pair.c of bwa 0.7.12 - 0.7.17 restated AS RECALLED: bwa's source is not in this tree; the semantics are
 * spelled out at bsw_rescue_* in the header.
 *
 * Per pair there are two directions; direction i takes its anchors from the INITIAL regions of read i and mutates a private copy
 * ma of read !i's regions, so a direction is indexed by the read its anchors come from, and its ma is what the mate read gets
 * back.  The alignments run on the GPU (the rescue tickets): the engine walks bwa's loop with the results it holds and stops a
 * direction at the first (anchor, r) whose result it lacks.  A result depends on (anchor, r, mate, contigs) alone, so one slot
 * per (anchor, r) holds it and it is never stale.  Nothing is aligned here; the sort-and-dedup pass is bsw_sdp.c's.
 */
#include "bsw_sdp_pass.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void bsw_rescue_default_opt(bsw_rescue_opt *o)
{
    int r;
    if (!o) return;
    for (r = 0; r < 4; ++r) { o->low[r] = o->high[r] = 0; o->failed[r] = 1; }
    o->pen_unpaired = 17;
    o->max_matesw = 50;
    o->min_seed_len = 19;
    o->a = 1;
    o->mask_level_redun = .95f;
    o->max_chain_gap = 10000;
}

enum { SLOT_NONE = 0, SLOT_ASKED = 1, SLOT_HELD = 2 };

typedef struct resc_held {           /* what the loop reads of a bsw_mresult */
    int64_t rb, re;
    int32_t qb, qe, score, csub, seedcov, status;
} resc_held;

typedef struct resc_dir {            /* where bwa's loop stands in one direction: the anchors of read d against ma = read d ^ 1 */
    uint64_t anchor0;                /* its anchors are anchor[anchor0, anchor0 + n_anchor): indices into regs[] */
    uint32_t n_anchor, k;            /* k: the anchor mem_matesw is in */
    int32_t r;                       /* the orientation it stands at; -1: skip[] of anchor k is not made yet */
    int32_t n;                       /* mem_matesw's n of anchor k */
    uint8_t skip[4];
    uint8_t done;
    uint64_t ma0, n_ma;              /* ma = arena[ma0, ma0 + n_ma) (the regions the mate read d ^ 1 ends with) */
} resc_dir;

struct bsw_rescue_eng {
    bsw_params p;
    bsw_rescue_opt opt;
    int64_t l_pac;
    bsw_contig *contigs;
    size_t n_contigs;
    bsw_sreg *regs;                  /* the input, src = the index */
    uint64_t *start;                 /* n_reads + 1 */
    int32_t *lens;
    size_t n_regs, n_reads;
    resc_dir *dir;                   /* n_reads */
    uint32_t *anchor;                /* n_anchor */
    size_t n_anchor;
    uint8_t *slot;                   /* 4 * n_anchor: SLOT_* of (anchor, r) */
    resc_held *held;                 /* 4 * n_anchor */
    bsw_sreg *arena;                 /* n_regs + 4 * n_anchor: every read's ma with room for what its rescues can add */
    uint32_t *src_tmp;               /* the longest ma: scratch of the pass */
    bsw_rd_mtask *req;               /* what the last needs asked for, and the slot of each */
    uint64_t *req_slot;
    size_t n_req;
    int32_t *n_sw;                   /* n_reads / 2 */
    int first, finished, pending;    /* pending: req[] waits for its feed */
    bsw_rescue_stats st;
};

static int resc_fail(char *err, size_t cap, int code, const char *fmt, ...)
{
    if (err && cap) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, cap, fmt, ap);
        va_end(ap);
    }
    return code;
}

/* the contig that holds the forward position fwd, -1: none (the table tiles [0, l_pac), so only outside it) */
static int64_t contig_at(const bsw_rescue_eng *e, int64_t fwd)
{
    size_t lo = 0, hi = e->n_contigs;
    while (lo < hi) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if (fwd < e->contigs[mid].offset) hi = mid;
        else if (fwd >= e->contigs[mid].offset + e->contigs[mid].len) lo = mid + 1;
        else return (int64_t)mid;
    }
    return -1;
}

/* orientation r of an anchor: the window after the contig step -> 1 when the contig and length tests pass (a task exists) */
static int window(const bsw_rescue_eng *e, const bsw_sreg *a, int l_ms, int r, int64_t *rb_, int64_t *re_, int32_t *is_rev)
{
    int64_t rb[4], re[4];
    int32_t rev[4], skip[4];
    bsw_matesw_windows(a->rb, l_ms, e->l_pac, e->opt.low, e->opt.high, e->opt.failed, rb, re, rev, skip);
    if (rb[r] < re[r] && e->n_contigs) {
        const int64_t mid = (rb[r] + re[r]) >> 1;
        const int64_t fwd = mid >= e->l_pac ? (e->l_pac << 1) - 1 - mid : mid;
        const int64_t rid = contig_at(e, fwd);
        int64_t lo, hi;
        if (rid < 0 || rid != a->rid) return 0;
        lo = e->contigs[rid].offset; hi = lo + e->contigs[rid].len;
        if (mid >= e->l_pac) {
            const int64_t t = (e->l_pac << 1) - hi;
            hi = (e->l_pac << 1) - lo; lo = t;
        }
        if (rb[r] < lo) rb[r] = lo;
        if (re[r] > hi) re[r] = hi;
    }
    *rb_ = rb[r]; *re_ = re[r]; *is_rev = rev[r];
    return re[r] - rb[r] >= e->opt.min_seed_len;
}

/* mem_matesw's skip[] of an anchor on the ma as it is -> 1 when all four are set */
static int make_skip(const bsw_rescue_eng *e, const bsw_sreg *a, const bsw_sreg *ma, size_t n_ma, uint8_t skip[4])
{
    size_t i;
    int r;
    for (r = 0; r < 4; ++r) skip[r] = e->opt.failed[r] != 0;
    for (i = 0; i < n_ma; ++i) {
        int64_t dist;
        r = bsw_infer_dir(e->l_pac, a->rb, ma[i].rb, &dist);
        if (dist >= e->opt.low[r] && dist <= e->opt.high[r]) skip[r] = 1;
    }
    return skip[0] && skip[1] && skip[2] && skip[3];
}

/* asks for (anchor slot ak, r) unless it is asked or held already or has no task */
static void request(bsw_rescue_eng *e, uint32_t d, uint64_t ak, int r)
{
    const bsw_sreg *a = &e->regs[e->anchor[ak]];
    const uint32_t mate = d ^ 1u;
    const int l_ms = e->lens[mate];
    bsw_rd_mtask *t;
    int64_t rb, re;
    int32_t is_rev;
    if (e->slot[4 * ak + (uint64_t)r] != SLOT_NONE || !window(e, a, l_ms, r, &rb, &re, &is_rev)) return;
    e->slot[4 * ak + (uint64_t)r] = SLOT_ASKED;
    e->req_slot[e->n_req] = 4 * ak + (uint64_t)r;
    t = &e->req[e->n_req++];
    t->read = mate; t->is_rev = is_rev; t->rb = rb; t->re = re;
    t->xtra = KSW_XSUBO | KSW_XSTART | ((int64_t)l_ms * e->opt.a < 250 ? KSW_XBYTE : 0) | (e->opt.min_seed_len * e->opt.a);
    t->min_score = e->opt.min_seed_len;
}

/* every orientation of the anchors from k on that is not skipped on the ma as it is (anchor k: its own skip[] when `own`) */
static void speculate(bsw_rescue_eng *e, uint32_t d, uint32_t k, const uint8_t *own, int from_r)
{
    const resc_dir *x = &e->dir[d];
    const bsw_sreg *ma = e->arena + x->ma0;
    for (; k < x->n_anchor; ++k, own = NULL, from_r = 0) {
        uint8_t skip[4];
        int r;
        if (own) memcpy(skip, own, 4);
        else if (make_skip(e, &e->regs[e->anchor[x->anchor0 + k]], ma, (size_t)x->n_ma, skip)) continue;
        for (r = from_r; r < 4; ++r)
            if (!skip[r]) request(e, d, x->anchor0 + k, r);
    }
}

static void insert(bsw_rescue_eng *e, resc_dir *x, uint32_t mate, const bsw_sreg *a, const resc_held *h)
{
    bsw_sreg *ma = e->arena + x->ma0, b;
    size_t i, at = (size_t)x->n_ma;
    memset(&b, 0, sizeof(b));
    b.rid = a->rid; b.rb = h->rb; b.re = h->re; b.qb = h->qb; b.qe = h->qe; b.score = h->score; b.csub = h->csub; b.seedcov = h->seedcov;
    b.read = mate; b.src = BSW_RESCUE_NEW | a->src;
    for (i = 0; i < x->n_ma; ++i)
        if (ma[i].score < b.score) { at = i; break; }
    memmove(ma + at + 1, ma + at, ((size_t)x->n_ma - at) * sizeof(*ma));
    ma[at] = b;
    ++x->n_ma;
    ++e->st.pushed;
}

/* bwa's loop from where the direction stands, as far as the held results reach.  Returns 1 when it stalls (the requests are made). */
static int advance(bsw_rescue_eng *e, uint32_t d)
{
    resc_dir *x = &e->dir[d];
    const uint32_t mate = d ^ 1u;
    const int l_ms = e->lens[mate];
    for (; x->k < x->n_anchor; ++x->k, x->r = -1) {
        const uint64_t ak = x->anchor0 + x->k;
        const bsw_sreg *a = &e->regs[e->anchor[ak]];
        if (x->r < 0) {
            x->n = 0; x->r = 0;
            if (make_skip(e, a, e->arena + x->ma0, (size_t)x->n_ma, x->skip)) continue;
        }
        for (; x->r < 4; ++x->r) {
            const int r = x->r;
            int64_t rb, re;
            int32_t is_rev;
            if (x->skip[r]) continue;
            if (window(e, a, l_ms, r, &rb, &re, &is_rev)) {
                const resc_held *h = &e->held[4 * ak + (uint64_t)r];
                if (e->slot[4 * ak + (uint64_t)r] != SLOT_HELD) {   /* stall here; ask for this one and what may follow it */
                    speculate(e, d, x->k, x->skip, r);
                    return 1;
                }
                if (h->status != 1) {
                    ++x->n;
                    if (h->status == 0) insert(e, x, mate, a, h);
                }
            }
            if (x->n > 0) x->n_ma = bsw_sdp_pass0(e->opt.mask_level_redun, e->opt.max_chain_gap, e->arena + x->ma0, (size_t)x->n_ma, e->src_tmp);
        }
        e->n_sw[d >> 1] += x->n;
        e->st.alns_bwa += (uint64_t)x->n;
    }
    x->done = 1;
    return 0;
}

int bsw_rescue_open(const bsw_params *p, const bsw_rescue_opt *opt, int64_t l_pac, const bsw_contig *contigs, size_t n_contigs, const bsw_sreg *regs,
                    size_t n_regs, const uint64_t *reg_start, const int32_t *lens, size_t n_reads, bsw_rescue_eng **eng, char *err, size_t cap)
{
    static const char who[] = "bsw_rescue_open";
    bsw_rescue_opt o;
    bsw_rescue_eng *e;
    size_t r, k, n_anchor = 0, longest = 0, at;
    int q;
    if (eng) *eng = NULL;
    if (!p || !eng || !reg_start || (!regs && n_regs) || (!lens && n_reads) || (!contigs && n_contigs))
        return resc_fail(err, cap, BSW_E_INVAL, "%s: NULL argument", who);
    if (n_regs > 0x7fffffffu) return resc_fail(err, cap, BSW_E_LIMIT, "%s: more than 2^31 - 1 regions (src is 31 bits and a flag)", who);
    if (opt) o = *opt; else bsw_rescue_default_opt(&o);
    if (l_pac < 1) return resc_fail(err, cap, BSW_E_INVAL, "%s: l_pac %lld below 1", who, (long long)l_pac);
    if (n_reads & 1) return resc_fail(err, cap, BSW_E_INVAL, "%s: n_reads %zu is odd (reads 2k and 2k + 1 are mates)", who, n_reads);
    if (o.pen_unpaired < 0 || o.max_matesw < 0 || o.min_seed_len < 0)
        return resc_fail(err, cap, BSW_E_INVAL, "%s: pen_unpaired %d, max_matesw %d or min_seed_len %d below 0", who, o.pen_unpaired, o.max_matesw, o.min_seed_len);
    if (o.a < 1) return resc_fail(err, cap, BSW_E_INVAL, "%s: a %d below 1", who, o.a);
    if ((int64_t)o.min_seed_len * o.a > 0xffff)
        return resc_fail(err, cap, BSW_E_INVAL, "%s: min_seed_len * a = %lld beyond 65535 (the threshold of xtra)", who, (long long)o.min_seed_len * o.a);
    if (o.max_chain_gap < 0 || !(o.mask_level_redun >= 0.f)) return resc_fail(err, cap, BSW_E_INVAL, "%s: max_chain_gap or mask_level_redun below 0", who);
    for (q = 0; q < 4; ++q)
        if (!o.failed[q] && o.low[q] > o.high[q])
            return resc_fail(err, cap, BSW_E_INVAL, "%s: orientation %d: low %d above high %d", who, q, o.low[q], o.high[q]);
    for (k = 0, at = 0; k < n_contigs; ++k) {
        if (contigs[k].len < 1 || contigs[k].offset != (int64_t)at)
            return resc_fail(err, cap, BSW_E_INVAL, "%s: contig %zu: offset %lld, len %lld; the contigs before it end at %zu (they must tile [0, l_pac) in ascending order)", who,
                             k, (long long)contigs[k].offset, (long long)contigs[k].len, at);
        at += (size_t)contigs[k].len;
    }
    if (n_contigs && (int64_t)at != l_pac)
        return resc_fail(err, cap, BSW_E_INVAL, "%s: the contigs end at %zu, l_pac is %lld (they must tile [0, l_pac))", who, at, (long long)l_pac);
    if (reg_start[0] != 0 || reg_start[n_reads] != n_regs)
        return resc_fail(err, cap, BSW_E_INVAL, "%s: reg_start runs from %llu to %llu, regs[] has %zu", who, (unsigned long long)reg_start[0],
                         (unsigned long long)reg_start[n_reads], n_regs);
    for (r = 0; r < n_reads; ++r) {
        if (reg_start[r + 1] < reg_start[r] || reg_start[r + 1] > n_regs)
            return resc_fail(err, cap, BSW_E_INVAL, "%s: reg_start[%zu] = %llu is behind reg_start[%zu] = %llu or beyond the %zu regions", who, r,
                             (unsigned long long)reg_start[r], r + 1, (unsigned long long)reg_start[r + 1], n_regs);
        if (lens[r] < 0) return resc_fail(err, cap, BSW_E_INVAL, "%s: read %zu: length %d below 0", who, r, lens[r]);
        for (k = reg_start[r]; k < reg_start[r + 1]; ++k) {
            const bsw_sreg *g = &regs[k];
            if (g->read != r) return resc_fail(err, cap, BSW_E_INVAL, "%s: region %zu: read %u, reg_start puts it in read %zu", who, k, g->read, r);
            if (g->rb >= g->re) return resc_fail(err, cap, BSW_E_INVAL, "%s: region %zu: rb %lld >= re %lld", who, k, (long long)g->rb, (long long)g->re);
            if (g->qb < 0 || g->qb >= g->qe || g->qe > lens[r])
                return resc_fail(err, cap, BSW_E_INVAL, "%s: region %zu: not 0 <= qb %d < qe %d <= %d, the length of read %zu", who, k, g->qb, g->qe, lens[r], r);
            if (g->w < 0) return resc_fail(err, cap, BSW_E_INVAL, "%s: region %zu: w %d below 0", who, k, g->w);
            if (g->score <= 0) return resc_fail(err, cap, BSW_E_INVAL, "%s: region %zu: score %d is not above 0", who, k, g->score);
            if (n_contigs && (g->rid < 0 || (size_t)g->rid >= n_contigs))
                return resc_fail(err, cap, BSW_E_INVAL, "%s: region %zu: rid %d outside the %zu contigs", who, k, g->rid, n_contigs);
            if (g->score >= regs[reg_start[r]].score - o.pen_unpaired) ++n_anchor;   /* (an upper bound: max_matesw cuts below) */
        }
    }
    e = (bsw_rescue_eng *)calloc(1, sizeof(*e));
    if (e) {
        e->regs = (bsw_sreg *)malloc((n_regs ? n_regs : 1) * sizeof(*e->regs));
        e->start = (uint64_t *)malloc((n_reads + 1) * sizeof(*e->start));
        e->lens = (int32_t *)malloc((n_reads ? n_reads : 1) * sizeof(*e->lens));
        e->contigs = (bsw_contig *)malloc((n_contigs ? n_contigs : 1) * sizeof(*e->contigs));
        e->dir = (resc_dir *)calloc(n_reads ? n_reads : 1, sizeof(*e->dir));
        e->anchor = (uint32_t *)malloc((n_anchor ? n_anchor : 1) * sizeof(*e->anchor));
        e->n_sw = (int32_t *)calloc(n_reads / 2 + 1, sizeof(*e->n_sw));
    }
    if (!e || !e->regs || !e->start || !e->lens || !e->contigs || !e->dir || !e->anchor || !e->n_sw) goto nomem;
    e->p = *p; e->opt = o; e->l_pac = l_pac; e->n_contigs = n_contigs; e->n_regs = n_regs; e->n_reads = n_reads; e->first = 1;
    if (n_regs) memcpy(e->regs, regs, n_regs * sizeof(*e->regs));
    if (n_reads) memcpy(e->lens, lens, n_reads * sizeof(*e->lens));
    if (n_contigs) memcpy(e->contigs, contigs, n_contigs * sizeof(*e->contigs));
    memcpy(e->start, reg_start, (n_reads + 1) * sizeof(*e->start));
    for (k = 0; k < n_regs; ++k) e->regs[k].src = (uint32_t)k;
    /* the anchors of every read: within pen_unpaired of the read's first region, in input order, max_matesw at most */
    for (r = 0, n_anchor = 0; r < n_reads; ++r) {
        resc_dir *x = &e->dir[r];
        x->anchor0 = n_anchor; x->r = -1;
        for (k = e->start[r]; k < e->start[r + 1] && x->n_anchor < (uint32_t)o.max_matesw; ++k)
            if (e->regs[k].score >= e->regs[e->start[r]].score - o.pen_unpaired) { e->anchor[n_anchor++] = (uint32_t)k; ++x->n_anchor; }
    }
    e->n_anchor = n_anchor;
    e->slot = (uint8_t *)calloc(4 * n_anchor + 1, 1);
    e->held = (resc_held *)calloc(4 * n_anchor + 1, sizeof(*e->held));
    e->req = (bsw_rd_mtask *)calloc(4 * n_anchor + 1, sizeof(*e->req));
    e->req_slot = (uint64_t *)malloc((4 * n_anchor + 1) * sizeof(*e->req_slot));
    e->arena = (bsw_sreg *)malloc((n_regs + 4 * n_anchor + 1) * sizeof(*e->arena));
    if (!e->slot || !e->held || !e->req || !e->req_slot || !e->arena) goto nomem;
    /* read m's regions are the ma of direction m ^ 1, with room for the four regions each of that direction's anchors can add */
    for (r = 0, at = 0; r < n_reads; ++r) {
        resc_dir *x = &e->dir[r ^ 1];
        const size_t n = (size_t)(e->start[r + 1] - e->start[r]), room = n + 4 * (size_t)x->n_anchor;
        x->ma0 = at; x->n_ma = n;
        if (n) memcpy(e->arena + at, e->regs + e->start[r], n * sizeof(*e->arena));
        at += room;
        if (room > longest) longest = room;
        if (!x->n_anchor) x->done = 1;
    }
    e->src_tmp = (uint32_t *)malloc((longest ? longest : 1) * sizeof(*e->src_tmp));
    if (!e->src_tmp) goto nomem;
    e->st.pairs = n_reads / 2; e->st.anchors = n_anchor; e->st.regs_in = n_regs;
    *eng = e;
    return BSW_OK;
nomem:
    bsw_rescue_close(e);
    return resc_fail(err, cap, BSW_E_NOMEM, "%s: %zu regions of %zu reads", who, n_regs, n_reads);
}

int bsw_rescue_needs(bsw_rescue_eng *e, const bsw_rd_mtask **tasks, size_t *n)
{
    size_t d;
    if (!e || !tasks || !n) return BSW_E_INVAL;
    *tasks = NULL; *n = 0;
    if (e->pending) { *tasks = e->req; *n = e->n_req; return BSW_OK; }      /* asked again before the feed: the same tasks */
    e->n_req = 0;
    if (e->first)                                               /* the speculation: every anchor's skip[] on the initial ma */
        for (d = 0; d < e->n_reads; ++d)
            if (!e->dir[d].done) speculate(e, (uint32_t)d, 0, NULL, 0);
    if (!e->first || !e->n_req)                                 /* (round 1 with requests: the walk starts when they are answered) */
        for (d = 0; d < e->n_reads; ++d)
            if (!e->dir[d].done) (void)advance(e, (uint32_t)d);
    e->first = 0;
    if (e->n_req) {
        ++e->st.rounds;
        if (e->st.rounds == 1) e->st.tasks_first = e->n_req;
        else e->st.late += e->n_req;
        e->st.tasks += e->n_req;
        e->pending = 1;
    } else
        e->finished = 1;
    *tasks = e->req; *n = e->n_req;
    return BSW_OK;
}

int bsw_rescue_feed(bsw_rescue_eng *e, const bsw_mresult *res, size_t n)
{
    size_t k;
    if (!e || (!res && n) || n != e->n_req || (n && !e->pending)) return BSW_E_INVAL;
    for (k = 0; k < n; ++k) {
        resc_held *h = &e->held[e->req_slot[k]];
        h->rb = res[k].rb; h->re = res[k].re; h->qb = res[k].qb; h->qe = res[k].qe; h->score = res[k].score; h->csub = res[k].csub;
        h->seedcov = res[k].seedcov; h->status = res[k].status;
        e->slot[e->req_slot[k]] = SLOT_HELD;
    }
    e->n_req = 0; e->pending = 0;
    return BSW_OK;
}

static size_t regs_now(const bsw_rescue_eng *e)
{
    size_t r, n = 0;
    for (r = 0; r < e->n_reads; ++r) n += (size_t)e->dir[r ^ 1].n_ma;
    return n;
}

int bsw_rescue_collect(bsw_rescue_eng *e, bsw_sreg *out, size_t *n_out, uint64_t *out_start, int32_t *n_sw, bsw_rescue_stats *stats)
{
    size_t r, at = 0;
    if (n_out) *n_out = 0;
    if (!e || !e->finished || (!out && regs_now(e))) return BSW_E_INVAL;
    for (r = 0; r < e->n_reads; ++r) {
        const resc_dir *x = &e->dir[r ^ 1];
        if (out_start) out_start[r] = at;
        if (x->n_ma) memcpy(out + at, e->arena + x->ma0, (size_t)x->n_ma * sizeof(*out));
        at += (size_t)x->n_ma;
    }
    if (out_start) out_start[e->n_reads] = at;
    if (n_sw && e->n_reads) memcpy(n_sw, e->n_sw, e->n_reads / 2 * sizeof(*n_sw));
    e->st.regs_out = at;
    if (n_out) *n_out = at;
    if (stats) *stats = e->st;
    return BSW_OK;
}

size_t bsw_rescue_out_capacity(const bsw_rescue_eng *e)
{
    return e ? e->n_regs + 4 * e->n_anchor : 0;
}

/* the counts so far and what collect would write now (bsw_rescue_job.hip); regs_out is collect's */
__attribute__((visibility("hidden"))) int bsw_rescue_peek(const bsw_rescue_eng *e, bsw_rescue_stats *stats, size_t *n_out)
{
    if (!e) return BSW_E_INVAL;
    if (stats) *stats = e->st;
    if (n_out) *n_out = regs_now(e);
    return BSW_OK;
}

void bsw_rescue_close(bsw_rescue_eng *e)
{
    if (!e) return;
    free(e->regs); free(e->start); free(e->lens); free(e->contigs); free(e->dir); free(e->anchor); free(e->n_sw);
    free(e->slot); free(e->held); free(e->req); free(e->req_slot); free(e->arena); free(e->src_tmp);
    free(e);
}
