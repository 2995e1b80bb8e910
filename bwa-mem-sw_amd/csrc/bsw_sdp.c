/*
 * bsw_sdp.c — mem_sort_dedup_patch as a resumable replay (host, plain C, no context).  bwamem.c of bwa 0.7.12 - 0.7.17 restated
 * AS RECALLED: bwa's source is not in this tree.
 *
 * bwa's loop is sequential per read and calls mem_patch_reg in the middle: a merge rewrites p and excludes q, and later pairs
 * see that.  The alignment behind mem_patch_reg runs on the GPU (the patch tickets), so the engine walks the loop with the
 * scores it holds and stops a read at the first pair whose score it lacks.  bsw_sdp_needs returns what the stalled reads lack,
 * bsw_sdp_feed takes the answers, and the walk goes on.  A held score is used only for exactly the twelve values it was
 * computed for, so a result that a merge has made stale is never read.  Nothing is aligned here.
 *
 * Both sorts are stable (bwa's ks_introsort is not): equal keys keep their previous order.  A region's input index (src) is
 * unique and ascending, and re is never rewritten, so (re, src) is the order behind the first sort at any later time.
 */
#include "../../include/bwa_sw_mi355.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void bsw_sdp_default_opt(bsw_sdp_opt *o)
{
    if (!o) return;
    o->mask_level_redun = .95f;
    o->max_chain_gap = 10000;
    o->patch = 1;
    o->presorted = 0;
}

int bsw_sdp_from_cregs(const bsw_creg *c, size_t n, bsw_sreg *s)
{
    size_t i;
    if ((!c || !s) && n) return BSW_E_INVAL;
    if ((uint64_t)n >> 32) return BSW_E_LIMIT;
    for (i = 0; i < n; ++i) {
        bsw_sreg *r = &s[i];
        r->rb = c[i].rb; r->re = c[i].re; r->qb = c[i].qb; r->qe = c[i].qe; r->score = c[i].score; r->truesc = c[i].truesc; r->w = c[i].w;
        r->seedcov = c[i].seedcov; r->sub = r->csub = 0; r->rid = c[i].rid; r->n_comp = 0; r->read = c[i].read; r->src = (uint32_t)i;
    }
    return BSW_OK;
}

typedef struct sdp_read {            /* where bwa's loop stands in one read */
    int32_t i, j;                    /* p = a[i]; q = a[j] while `inner` */
    uint8_t inner, done;
    int64_t held;                    /* head of the read's list in held[], -1: none */
} sdp_read;
typedef struct sdp_held {            /* a task with its answer */
    bsw_preg a, b;
    bsw_presult r;
    int64_t next;
} sdp_held;

struct bsw_sdp_eng {
    bsw_params p;
    bsw_sdp_opt opt;
    int64_t l_pac;
    bsw_sreg *a;                     /* the regions, every read's sorted by re */
    uint64_t *start;                 /* n_reads + 1 */
    sdp_read *rd;
    size_t n_regs, n_reads;
    bsw_rd_ptask *req;               /* what the last needs asked for */
    size_t n_req, cap_req;
    sdp_held *held;
    size_t n_held, cap_held;
    int first, finished, nomem;
    bsw_sdp_stats st;
};

static int sdp_fail(char *err, size_t cap, int code, const char *fmt, ...)
{
    if (err && cap) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, cap, fmt, ap);
        va_end(ap);
    }
    return code;
}

static int by_re(const void *x, const void *y)
{
    const bsw_sreg *a = (const bsw_sreg *)x, *b = (const bsw_sreg *)y;
    if (a->re != b->re) return a->re < b->re ? -1 : 1;
    return a->src < b->src ? -1 : a->src > b->src;
}

static int by_score(const void *x, const void *y)      /* mem_ars: score descending, rb, qb ascending; then the order they stood in */
{
    const bsw_sreg *a = (const bsw_sreg *)x, *b = (const bsw_sreg *)y;
    if (a->score != b->score) return a->score > b->score ? -1 : 1;
    if (a->rb != b->rb) return a->rb < b->rb ? -1 : 1;
    if (a->qb != b->qb) return a->qb < b->qb ? -1 : 1;
    return by_re(x, y);
}

/* a read has a handful of regions: insertion below 24 of them (both orders are total, so any correct sort gives the same array) */
static void sort_regs(bsw_sreg *a, size_t n, int (*cmp)(const void *, const void *))
{
    size_t i, j;
    if (n > 24) { qsort(a, n, sizeof(*a), cmp); return; }
    for (i = 1; i < n; ++i) {
        const bsw_sreg t = a[i];
        for (j = i; j > 0 && cmp(&a[j - 1], &t) > 0; --j) a[j] = a[j - 1];
        a[j] = t;
    }
}

static bsw_preg preg_of(const bsw_sreg *r)
{
    bsw_preg g;
    g.rb = r->rb; g.re = r->re; g.qb = r->qb; g.qe = r->qe; g.score = r->score; g.w = r->w;
    return g;
}

static int same_preg(const bsw_preg *x, const bsw_preg *y)
{
    return x->rb == y->rb && x->re == y->re && x->qb == y->qb && x->qe == y->qe && x->score == y->score && x->w == y->w;
}

/* the for statement's condition: it ends the descent */
static int descends(const bsw_sdp_eng *e, const bsw_sreg *p, const bsw_sreg *q)
{
    return p->rid == q->rid && p->rb < q->re + e->opt.max_chain_gap;
}

/* the redundancy test, in binary32 as bwa's float option makes it */
static int redundant(const bsw_sdp_eng *e, const bsw_sreg *p, const bsw_sreg *q)
{
    const int64_t orr = q->re - p->rb;
    const int64_t oq = q->qb < p->qb ? (int64_t)q->qe - p->qb : (int64_t)p->qe - q->qb;
    const int64_t lq = q->re - q->rb, lp = p->re - p->rb;
    const int64_t mr = lq < lp ? lq : lp;
    const int64_t sq = (int64_t)q->qe - q->qb, sp = (int64_t)p->qe - p->qb;
    const int64_t mq = sq < sp ? sq : sp;
    const float f = e->opt.mask_level_redun;
    const float tr = f * (float)mr, tq = f * (float)mq;
    return (float)orr > tr && (float)oq > tq;
}

static const sdp_held *lookup(const bsw_sdp_eng *e, const sdp_read *r, const bsw_preg *a, const bsw_preg *b)
{
    int64_t k;
    for (k = r->held; k >= 0; k = e->held[k].next)
        if (same_preg(&e->held[k].a, a) && same_preg(&e->held[k].b, b)) return &e->held[k];
    return NULL;
}

static void request(bsw_sdp_eng *e, uint32_t read, const bsw_preg *a, const bsw_preg *b)
{
    bsw_rd_ptask *t;
    if (e->n_req == e->cap_req) {
        const size_t cap = e->cap_req ? e->cap_req * 2 : 1024;
        bsw_rd_ptask *m = (bsw_rd_ptask *)realloc(e->req, cap * sizeof(*m));
        if (!m) { e->nomem = 1; return; }
        e->req = m; e->cap_req = cap;
    }
    t = &e->req[e->n_req++];
    t->read = read; t->_pad = 0; t->a = *a; t->b = *b;
}

/* every pair of p = a[i] with q = a[j], j from `from` down, that the descent's condition reaches on the states as they are, that
 * is not redundant, has q.rb < p.rb, passes the pre-tests and is not held already; excluded regions are skipped */
static void speculate(bsw_sdp_eng *e, uint32_t read, const sdp_read *r, const bsw_sreg *a, int32_t i, int32_t from)
{
    const bsw_sreg *p = &a[i];
    const bsw_preg b = preg_of(p);
    int32_t j;
    for (j = from; j >= 0 && descends(e, p, &a[j]); --j) {
        const bsw_sreg *q = &a[j];
        bsw_preg g;
        if (q->qe == q->qb || redundant(e, p, q) || q->rb >= p->rb) continue;
        g = preg_of(q);
        if (!bsw_patch_pretest(&e->p, e->l_pac, &g, &b, NULL) || lookup(e, r, &g, &b)) continue;
        request(e, read, &g, &b);
    }
}

/* bwa's loop from where the read stands, as far as the held scores reach.  Returns 1 when it stalls (the requests are made). */
static int advance(bsw_sdp_eng *e, uint32_t read)
{
    sdp_read *r = &e->rd[read];
    bsw_sreg *a = e->a + e->start[read];
    const int32_t n = (int32_t)(e->start[read + 1] - e->start[read]);
    while (r->i < n) {
        bsw_sreg *p = &a[r->i];
        if (!r->inner) {
            if (p->rid != a[r->i - 1].rid || p->rb >= a[r->i - 1].re + e->opt.max_chain_gap) { ++r->i; continue; }
            r->j = r->i - 1; r->inner = 1;
        }
        for (; r->j >= 0 && descends(e, p, &a[r->j]); --r->j) {
            bsw_sreg *q = &a[r->j];
            int score = 0, w = 0;
            if (q->qe == q->qb) continue;                       /* q was excluded earlier */
            if (redundant(e, p, q)) {
                if (p->score < q->score) { p->qe = p->qb; ++e->st.kills_p; break; }
                q->qe = q->qb; ++e->st.kills_q;
                continue;
            }
            if (q->rb >= p->rb || !e->opt.patch) continue;
            {
                const bsw_preg ga = preg_of(q), gb = preg_of(p);
                const sdp_held *h;
                if (!bsw_patch_pretest(&e->p, e->l_pac, &ga, &gb, &w)) continue;
                h = lookup(e, r, &ga, &gb);
                if (!h) {                                       /* stall here; ask for this pair and what lies below it */
                    request(e, read, &ga, &gb);
                    speculate(e, read, r, a, r->i, r->j - 1);
                    return 1;
                }
                ++e->st.alns_bwa;
                if (h->r.status != 1) { score = bsw_patch_decide(&ga, &gb, h->r.gscore); w = h->r.w; }
            }
            if (score > 0) {
                ++e->st.merges;
                p->n_comp += q->n_comp + 1;
                if (q->seedcov > p->seedcov) p->seedcov = q->seedcov;
                if (q->sub > p->sub) p->sub = q->sub;
                if (q->csub > p->csub) p->csub = q->csub;
                p->qb = q->qb; p->rb = q->rb; p->truesc = p->score = score; p->w = w;
                q->qb = q->qe;
            }
        }
        r->inner = 0; ++r->i;
    }
    r->done = 1;
    return 0;
}

int bsw_sdp_open(const bsw_params *p, const bsw_sdp_opt *opt, int64_t l_pac, const bsw_sreg *regs, size_t n_regs, const uint64_t *reg_start,
                 const int32_t *lens, size_t n_reads, bsw_sdp_eng **eng, char *err, size_t cap)
{
    static const char who[] = "bsw_sdp_open";
    bsw_sdp_eng *e;
    size_t r, k;
    if (eng) *eng = NULL;
    if (!p || !eng || !reg_start || (!regs && n_regs) || (!lens && n_reads)) return sdp_fail(err, cap, BSW_E_INVAL, "%s: NULL argument", who);
    if ((uint64_t)n_regs >> 32) return sdp_fail(err, cap, BSW_E_LIMIT, "%s: more than 2^32 - 1 regions (src is 32 bits)", who);
    if (opt && (opt->max_chain_gap < 0 || !(opt->mask_level_redun >= 0.f)))
        return sdp_fail(err, cap, BSW_E_INVAL, "%s: max_chain_gap or mask_level_redun below 0", who);
    if (p->w < 0) return sdp_fail(err, cap, BSW_E_INVAL, "%s: params.w below 0", who);
    if (reg_start[0] != 0 || reg_start[n_reads] != n_regs)
        return sdp_fail(err, cap, BSW_E_INVAL, "%s: reg_start runs from %llu to %llu, regs[] has %zu", who, (unsigned long long)reg_start[0],
                        (unsigned long long)reg_start[n_reads], n_regs);
    for (r = 0; r < n_reads; ++r) {
        if (reg_start[r + 1] < reg_start[r] || reg_start[r + 1] > n_regs)
            return sdp_fail(err, cap, BSW_E_INVAL, "%s: reg_start[%zu] = %llu is behind reg_start[%zu] = %llu or beyond the %zu regions", who, r,
                            (unsigned long long)reg_start[r], r + 1, (unsigned long long)reg_start[r + 1], n_regs);
        if (reg_start[r + 1] - reg_start[r] > 0x7fffffffu) return sdp_fail(err, cap, BSW_E_LIMIT, "%s: read %zu has more than 2^31 - 1 regions", who, r);
        for (k = reg_start[r]; k < reg_start[r + 1]; ++k) {
            const bsw_sreg *g = &regs[k];
            if (g->read != r) return sdp_fail(err, cap, BSW_E_INVAL, "%s: region %zu: read %u, reg_start puts it in read %zu", who, k, g->read, r);
            if (g->rb >= g->re) return sdp_fail(err, cap, BSW_E_INVAL, "%s: region %zu: rb %lld >= re %lld", who, k, (long long)g->rb, (long long)g->re);
            if (g->qb < 0 || g->qb >= g->qe || g->qe > lens[r])
                return sdp_fail(err, cap, BSW_E_INVAL, "%s: region %zu: not 0 <= qb %d < qe %d <= %d, the length of read %zu", who, k, g->qb, g->qe, lens[r], r);
            if (g->w < 0) return sdp_fail(err, cap, BSW_E_INVAL, "%s: region %zu: w %d below 0", who, k, g->w);
            if (g->score <= 0) return sdp_fail(err, cap, BSW_E_INVAL, "%s: region %zu: score %d is not above 0", who, k, g->score);
            if (opt && opt->presorted && k > reg_start[r] && g->re < regs[k - 1].re)
                return sdp_fail(err, cap, BSW_E_INVAL, "%s: region %zu: presorted, but re %lld is below re %lld of the region before it", who, k,
                                (long long)g->re, (long long)regs[k - 1].re);
        }
    }
    e = (bsw_sdp_eng *)calloc(1, sizeof(*e));
    if (e) {
        e->a = (bsw_sreg *)malloc((n_regs ? n_regs : 1) * sizeof(*e->a));
        e->start = (uint64_t *)malloc((n_reads + 1) * sizeof(*e->start));
        e->rd = (sdp_read *)calloc(n_reads ? n_reads : 1, sizeof(*e->rd));
    }
    if (!e || !e->a || !e->start || !e->rd) {
        bsw_sdp_close(e);
        return sdp_fail(err, cap, BSW_E_NOMEM, "%s: %zu regions of %zu reads", who, n_regs, n_reads);
    }
    e->p = *p; e->l_pac = l_pac; e->n_regs = n_regs; e->n_reads = n_reads; e->first = 1;
    if (opt) e->opt = *opt; else bsw_sdp_default_opt(&e->opt);
    if (n_regs) memcpy(e->a, regs, n_regs * sizeof(*e->a));
    memcpy(e->start, reg_start, (n_reads + 1) * sizeof(*e->start));
    for (k = 0; k < n_regs; ++k) e->a[k].src = (uint32_t)k;
    for (r = 0; r < n_reads; ++r) {
        const size_t n = (size_t)(e->start[r + 1] - e->start[r]);
        sdp_read *s = &e->rd[r];
        s->held = -1; s->i = 1;
        if (n <= 1) { s->done = 1; continue; }                  /* returned untouched, n_comp included */
        if (!e->opt.presorted) sort_regs(e->a + e->start[r], n, by_re);
        for (k = e->start[r]; k < e->start[r + 1]; ++k) e->a[k].n_comp = 1;
    }
    e->st.reads = n_reads; e->st.regs_in = n_regs;
    *eng = e;
    return BSW_OK;
}

int bsw_sdp_needs(bsw_sdp_eng *e, const bsw_rd_ptask **tasks, size_t *n)
{
    size_t r;
    int stalled = 0;
    if (!e || !tasks || !n) return BSW_E_INVAL;
    *tasks = NULL; *n = 0;
    if (e->nomem) return BSW_E_NOMEM;
    e->n_req = 0;
    if (e->first && e->opt.patch) {                             /* the speculation: bwa's descent over the unmodified regions */
        for (r = 0; r < e->n_reads; ++r) {
            const bsw_sreg *a = e->a + e->start[r];
            const int32_t cnt = (int32_t)(e->start[r + 1] - e->start[r]);
            int32_t i;
            for (i = 1; i < cnt; ++i) speculate(e, (uint32_t)r, &e->rd[r], a, i, i - 1);
        }
        stalled = e->n_req > 0;
    }
    if (!e->first || !stalled)                                  /* (round 1 with requests: the walk starts when they are answered) */
        for (r = 0; r < e->n_reads; ++r)
            if (!e->rd[r].done) stalled |= advance(e, (uint32_t)r);
    e->first = 0;
    if (e->nomem) return BSW_E_NOMEM;
    if (e->n_req) {
        ++e->st.rounds;
        if (e->st.rounds == 1) e->st.tasks_first = e->n_req;
        e->st.tasks += e->n_req;
    } else
        e->finished = 1;
    *tasks = e->req; *n = e->n_req;
    return BSW_OK;
}

int bsw_sdp_feed(bsw_sdp_eng *e, const bsw_presult *res, size_t n)
{
    size_t k;
    if (!e || (!res && n) || n != e->n_req) return BSW_E_INVAL;
    if (e->n_held + n > e->cap_held) {
        const size_t cap = (e->n_held + n) * 2;
        sdp_held *m = (sdp_held *)realloc(e->held, cap * sizeof(*m));
        if (!m) { e->nomem = 1; return BSW_E_NOMEM; }
        e->held = m; e->cap_held = cap;
    }
    for (k = 0; k < n; ++k) {
        sdp_held *h = &e->held[e->n_held];
        sdp_read *r = &e->rd[e->req[k].read];
        h->a = e->req[k].a; h->b = e->req[k].b; h->r = res[k];
        h->next = r->held; r->held = (int64_t)e->n_held++;
    }
    e->n_req = 0;
    return BSW_OK;
}

/* what is left of a walked read, in bwa's order, to out[] (which may be a itself) -> how many */
static size_t survivors(const bsw_sreg *a, size_t n, bsw_sreg *out, uint64_t *dups)
{
    size_t k, m, at = 0;
    if (n <= 1) {
        if (n) out[at++] = a[0];
        return at;
    }
    for (k = 0; k < n; ++k)
        if (a[k].qe > a[k].qb) out[at++] = a[k];
    sort_regs(out, at, by_score);
    for (k = m = 0; k < at; ++k) {                              /* against the neighbour, marked or not: the first of a run stays */
        if (k > 0 && out[k].score == out[k - 1].score && out[k].rb == out[k - 1].rb && out[k].qb == out[k - 1].qb) { ++*dups; continue; }
        out[m++] = out[k];                                      /* (m <= k: out[k] itself stays in place for the next comparison) */
    }
    return m;
}

int bsw_sdp_collect(bsw_sdp_eng *e, bsw_sreg *out, size_t *n_out, uint64_t *out_start, bsw_sdp_stats *stats)
{
    size_t r, at = 0;
    if (n_out) *n_out = 0;
    if (!e || !e->finished || (!out && e->n_regs)) return BSW_E_INVAL;
    e->st.dups = 0;
    for (r = 0; r < e->n_reads; ++r) {
        const size_t n = (size_t)(e->start[r + 1] - e->start[r]);
        if (out_start) out_start[r] = at;
        if (n) at += survivors(e->a + e->start[r], n, out + at, &e->st.dups);
    }
    if (out_start) out_start[e->n_reads] = at;
    e->st.regs_out = at;
    if (n_out) *n_out = at;
    if (stats) *stats = e->st;
    return BSW_OK;
}

/* the counts so far (bsw_sdp_job.hip: bsw_sdp_job_stats); regs_out and dups are collect's */
__attribute__((visibility("hidden"))) int bsw_sdp_peek_stats(const bsw_sdp_eng *e, bsw_sdp_stats *stats)
{
    if (!e || !stats) return BSW_E_INVAL;
    *stats = e->st;
    return BSW_OK;
}

/* One read's pass with patch = 0 in place, for mem_matesw's call inside the rescue loop (bsw_rescue.c): the order of a[] on entry
 * is the order behind both sorts' ties; src is carried along untouched (src_tmp: n values of scratch).  -> the regions left */
__attribute__((visibility("hidden"))) size_t bsw_sdp_pass0(float mask_level_redun, int32_t max_chain_gap, bsw_sreg *a, size_t n, uint32_t *src_tmp)
{
    bsw_sdp_eng e;
    sdp_read rd;
    uint64_t start[2], dups = 0;
    size_t k;
    if (n <= 1) return n;                                       /* returned untouched, n_comp included */
    memset(&e, 0, sizeof(e));
    memset(&rd, 0, sizeof(rd));
    e.opt.mask_level_redun = mask_level_redun; e.opt.max_chain_gap = max_chain_gap;
    start[0] = 0; start[1] = n;
    e.a = a; e.start = start; e.rd = &rd; e.n_regs = n; e.n_reads = 1;
    rd.held = -1; rd.i = 1;
    for (k = 0; k < n; ++k) { src_tmp[k] = a[k].src; a[k].src = (uint32_t)k; }
    sort_regs(a, n, by_re);
    for (k = 0; k < n; ++k) a[k].n_comp = 1;
    (void)advance(&e, 0);                                       /* patch = 0: no pair is asked for, the walk never stalls */
    n = survivors(a, n, a, &dups);
    for (k = 0; k < n; ++k) a[k].src = src_tmp[a[k].src];
    return n;
}

void bsw_sdp_close(bsw_sdp_eng *e)
{
    if (!e) return;
    free(e->a); free(e->start); free(e->rd); free(e->req); free(e->held);
    free(e);
}
