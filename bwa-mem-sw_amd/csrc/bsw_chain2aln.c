/*
 * bsw_chain2aln.c — mem_chain2aln's driver around the seed extension (host, plain C): which seeds of a chain bwa extends, in
 * which order, and the region it makes of each.  bwamem.c of bwa 0.7.12 - 0.7.17 restated AS RECALLED: bwa's source is not in this
 * tree.
 *
 * The extension of a seed does not depend on the regions found so far; only the DECISION to run it does.  So bsw_chain2aln_plan
 * makes a task of EVERY seed, the GPU extends them all, and bsw_chain2aln_replay walks bwa's loop with the results at hand: the
 * result of a seed bwa skips is never read, and the list of regions is bwa's, in bwa's push order.
 *
 *   srt[i] = (uint64)score << 32 | i, sorted ascending, visited from the top: highest score first, the larger index first among
 *   equal scores.  A seed is skipped when an earlier region of the read (any chain's) contains it on both axes within that
 *   region's band and no long seed of its chain, visited earlier and not skipped, overlaps it on another diagonal.  The skip mark
 *   is the VALUE 0 in srt[], as in bwa: (score 0, index 0) reads as "skipped" too.  No rescue ever looks at that entry — with
 *   scores >= 0 it sorts to position 0, is visited last, and the rescue of a seed reads only the positions above its own — so the
 *   quirk is kept and cannot be observed; negative scores (where it could) are refused.
 */
#include "../../include/bwa_sw_mi355.h"

#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

void bsw_c2a_default_opt(bsw_c2a_opt *o)
{
    if (!o) return;
    o->seedlen0_frac = .1;
    o->ovl_len_frac = .95;
}

static int c2a_fail(char *err, size_t cap, int code, const char *fmt, ...)
{
    if (err && cap) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, cap, fmt, ap);
        va_end(ap);
    }
    return code;
}

/* what plan and replay both need of the arrays: chains sorted by read and laid over seeds[] without a gap, every seed inside
 * its read */
static int c2a_check(const char *who, const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds, size_t n_seeds, const int32_t *lens,
                     size_t n_reads, char *err, size_t cap)
{
    size_t c, at = 0;
    if ((!chains && n_chains) || (!seeds && n_seeds) || (!lens && n_reads)) return c2a_fail(err, cap, BSW_E_INVAL, "%s: NULL argument", who);
    if ((uint64_t)n_seeds >> 32 || (uint64_t)n_chains >> 32) return c2a_fail(err, cap, BSW_E_LIMIT, "%s: more than 2^32 - 1 seeds or chains (the tag is 32 bits)", who);
    for (c = 0; c < n_chains; ++c) {
        const bsw_chain *ch = &chains[c];
        int32_t k, lq;
        if (ch->read >= n_reads) return c2a_fail(err, cap, BSW_E_INVAL, "%s: chain %zu: read %u is not among the %zu reads", who, c, ch->read, n_reads);
        if (c && ch->read < chains[c - 1].read)
            return c2a_fail(err, cap, BSW_E_INVAL, "%s: chain %zu: the chains of a read are not contiguous (read %u behind read %u)", who, c, ch->read, chains[c - 1].read);
        if (ch->n_seeds < 1) return c2a_fail(err, cap, BSW_E_INVAL, "%s: chain %zu: no seed", who, c);
        if (ch->first_seed != at || (uint64_t)ch->n_seeds > n_seeds - at)
            return c2a_fail(err, cap, BSW_E_INVAL, "%s: chain %zu: its seeds [%llu, +%d) do not follow the previous chain's inside seeds[0, %zu)", who, c,
                            (unsigned long long)ch->first_seed, ch->n_seeds, n_seeds);
        lq = lens[ch->read];
        for (k = 0; k < ch->n_seeds; ++k) {
            const bsw_cseed *s = &seeds[at + (size_t)k];
            if (s->qbeg < 0 || s->len < 1 || s->len > lq || s->qbeg > lq - s->len)
                return c2a_fail(err, cap, BSW_E_INVAL, "%s: seed %zu: [%d, +%d) lies outside its read of %d bases", who, at + (size_t)k, s->qbeg, s->len, lq);
            if (s->score < 0) return c2a_fail(err, cap, BSW_E_INVAL, "%s: seed %zu: negative score", who, at + (size_t)k);
        }
        at += (size_t)ch->n_seeds;
    }
    if (at != n_seeds) return c2a_fail(err, cap, BSW_E_INVAL, "%s: the chains hold %zu seeds, seeds[] has %zu", who, at, n_seeds);
    return BSW_OK;
}

int bsw_chain2aln_plan(const bsw_params *p, int64_t l_pac, const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds, size_t n_seeds,
                       const int32_t *lens, size_t n_reads, const uint8_t *const *reads, bsw_rd_task *rd_tasks, bsw_ref_task *ref_tasks,
                       char *err, size_t err_cap)
{
    static const char who[] = "bsw_chain2aln_plan";
    bsw_seed *tmp = NULL;
    size_t c, tmp_cap = 0;
    int rc;
    if (err && err_cap) err[0] = 0;
    if (!p || l_pac < 1 || p->e_del < 1 || p->e_ins < 1 || (ref_tasks && !reads)) return c2a_fail(err, err_cap, BSW_E_INVAL, "%s: NULL or bad argument", who);
    if ((rc = c2a_check(who, chains, n_chains, seeds, n_seeds, lens, n_reads, err, err_cap))) return rc;
    for (c = 0; c < n_chains && !rc; ++c) {
        const bsw_chain *ch = &chains[c];
        const bsw_cseed *cs = seeds + ch->first_seed;
        const int32_t n = ch->n_seeds, lq = lens[ch->read];
        int64_t rmax[2];
        int32_t k;
        if ((size_t)n > tmp_cap) {
            free(tmp);
            tmp_cap = (size_t)n + 16;
            if (!(tmp = (bsw_seed *)malloc(tmp_cap * sizeof(bsw_seed)))) return c2a_fail(err, err_cap, BSW_E_NOMEM, "%s: %zu bytes", who, tmp_cap * sizeof(bsw_seed));
        }
        for (k = 0; k < n; ++k) {
            if (cs[k].rbeg < 0 || cs[k].rbeg + cs[k].len > l_pac << 1) {
                rc = c2a_fail(err, err_cap, BSW_E_INVAL, "%s: seed %zu: reference position outside [0, 2*l_pac)", who, (size_t)ch->first_seed + (size_t)k);
                break;
            }
            tmp[k].rbeg = cs[k].rbeg; tmp[k].qbeg = cs[k].qbeg; tmp[k].len = cs[k].len;
        }
        if (rc) break;
        if ((rc = bsw_chain_window(p, tmp, n, lq, l_pac, rmax))) { rc = c2a_fail(err, err_cap, rc, "%s: chain %zu: bsw_chain_window", who, c); break; }
        if (ch->rhi > ch->rlo) {                     /* bns_fetch_seq: the window stays inside the chain's contig */
            if (ch->rlo < 0 || ch->rhi > l_pac << 1) { rc = c2a_fail(err, err_cap, BSW_E_INVAL, "%s: chain %zu: contig interval outside [0, 2*l_pac)", who, c); break; }
            if (rmax[0] < ch->rlo) rmax[0] = ch->rlo;
            if (rmax[1] > ch->rhi) rmax[1] = ch->rhi;
        }
        for (k = 0; k < n; ++k) {
            const size_t i = (size_t)ch->first_seed + (size_t)k;
            const int64_t lt = cs[k].rbeg - rmax[0], rt = rmax[1] - (cs[k].rbeg + cs[k].len);
            if (lt < 0 || rt < 0) { rc = c2a_fail(err, err_cap, BSW_E_INVAL, "%s: seed %zu lies outside its chain's window [%lld, %lld)", who, i, (long long)rmax[0], (long long)rmax[1]); break; }
            if (lt > BSW_MAX_TLEN || rt > BSW_MAX_TLEN) { rc = c2a_fail(err, err_cap, BSW_E_LIMIT, "%s: seed %zu: a window side beyond BSW_MAX_TLEN", who, i); break; }
            if (rd_tasks) {
                bsw_rd_task *t = &rd_tasks[i];
                memset(t, 0, sizeof(*t));
                t->read = ch->read; t->init_score = -1; t->seed = tmp[k]; t->rmax0 = rmax[0]; t->rmax1 = rmax[1]; t->tag = (uint32_t)i;
            }
            if (ref_tasks) {
                bsw_ref_task *t = &ref_tasks[i];
                memset(t, 0, sizeof(*t));
                t->query = reads[ch->read]; t->l_query = lq; t->init_score = -1; t->seed = tmp[k]; t->rmax0 = rmax[0]; t->rmax1 = rmax[1]; t->tag = (uint32_t)i;
            }
        }
    }
    free(tmp);
    return rc;
}

static int cmp_u64(const void *a, const void *b)
{
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : x > y;
}

static void sort_u64(uint64_t *a, int n)
{
    int i, j;
    if (n > 24) { qsort(a, (size_t)n, sizeof(uint64_t), cmp_u64); return; }
    for (i = 1; i < n; ++i) {
        const uint64_t x = a[i];
        for (j = i; j > 0 && a[j - 1] > x; --j) a[j] = a[j - 1];
        a[j] = x;
    }
}

/* does region p "explain" seed s (bwa: "the seed is around a previous hit") */
static int c2a_explains(const bsw_params *p, const bsw_c2a_opt *o, const bsw_creg *r, const bsw_cseed *s, int l_query)
{
    int64_t rd;
    int qd, w, g;
    if (s->rbeg < r->rb || s->rbeg + s->len > r->re || s->qbeg < r->qb || s->qbeg + s->len > r->qe) return 0;   /* not fully contained */
    if (o->seedlen0_frac >= 0 && s->len - r->seedlen0 > o->seedlen0_frac * l_query) return 0;              /* this seed may give a better alignment */
    qd = s->qbeg - r->qb; rd = s->rbeg - r->rb;                        /* ahead of the seed */
    g = bsw_cal_max_gap(p, qd < rd ? qd : (int)rd);
    w = g < r->w ? g : r->w;
    if (qd - rd < w && rd - qd < w) return 1;
    qd = r->qe - (s->qbeg + s->len); rd = r->re - (s->rbeg + s->len);  /* behind it */
    g = bsw_cal_max_gap(p, qd < rd ? qd : (int)rd);
    w = g < r->w ? g : r->w;
    return qd - rd < w && rd - qd < w;
}

/* bwa's loop over chains[c0, c1) — whole reads — into regs[0 ..): *n_regs regions; extended[] and reg_cnt[read] (regions per
 * read) are only added to.  Reads are independent, so ranges that share no read may run side by side. */
static int c2a_replay_range(const bsw_params *p, const bsw_c2a_opt *o, const bsw_chain *chains, size_t c0, size_t c1, const bsw_cseed *seeds,
                            const int32_t *lens, const void *results, size_t stride, bsw_creg *regs, size_t *n_regs, uint8_t *extended,
                            uint64_t *reg_cnt)
{
    uint64_t *srt = NULL;
    size_t c, srt_cap = 0, total = 0, base = 0;
    for (c = c0; c < c1; ++c) {
        const bsw_chain *ch = &chains[c];
        const bsw_cseed *cs = seeds + ch->first_seed;
        const int n = ch->n_seeds, lq = lens[ch->read];
        int i, k;
        if (c == c0 || ch->read != chains[c - 1].read) base = total;       /* a new read: its list starts empty */
        if ((size_t)n > srt_cap) {
            free(srt);
            srt_cap = (size_t)n + 16;
            if (!(srt = (uint64_t *)malloc(srt_cap * sizeof(uint64_t)))) return BSW_E_NOMEM;
        }
        for (i = 0; i < n; ++i) srt[i] = (uint64_t)cs[i].score << 32 | (uint32_t)i;
        sort_u64(srt, n);
        for (k = n - 1; k >= 0; --k) {
            const uint32_t si = (uint32_t)srt[k];
            const bsw_cseed *s = &cs[si];
            const size_t gi = (size_t)ch->first_seed + si;
            bsw_pair r;
            bsw_creg *a;
            size_t j;
            for (j = base; j < total; ++j)
                if (c2a_explains(p, o, &regs[j], s, lq)) break;
            if (j < total) {                         /* explained: unless a long seed visited earlier overlaps it on another diagonal */
                for (i = k + 1; i < n; ++i) {
                    const bsw_cseed *t;
                    if (srt[i] == 0) continue;
                    t = &cs[(uint32_t)srt[i]];
                    if (t->len < s->len * o->ovl_len_frac) continue;
                    if (s->qbeg <= t->qbeg && s->qbeg + s->len - t->qbeg >= s->len >> 2 && t->qbeg - s->qbeg != t->rbeg - s->rbeg) break;
                    if (t->qbeg <= s->qbeg && t->qbeg + t->len - s->qbeg >= s->len >> 2 && s->qbeg - t->qbeg != s->rbeg - t->rbeg) break;
                }
                if (i == n) { srt[k] = 0; continue; }
            }
            memcpy(&r, (const char *)results + gi * stride, sizeof(r));      /* (the pair record is the head of the full one) */
            a = &regs[total++];
            a->rb = s->rbeg + r.rb;                a->re = s->rbeg + s->len + r.re;
            a->qb = r.qb;                          a->qe = s->qbeg + s->len + r.qe;
            a->score = r.score; a->truesc = r.truesc; a->w = r.w;
            a->seedcov = 0;
            for (i = 0; i < n; ++i)
                if (cs[i].qbeg >= a->qb && cs[i].qbeg + cs[i].len <= a->qe && cs[i].rbeg >= a->rb && cs[i].rbeg + cs[i].len <= a->re) a->seedcov += cs[i].len;
            a->seedlen0 = s->len;
            a->rid = ch->rid; a->frac_rep = ch->frac_rep;
            a->read = ch->read; a->chain = (uint32_t)c; a->seed = (uint32_t)gi;
            if (extended) extended[gi] = 1;
            if (reg_cnt) ++reg_cnt[ch->read];
        }
    }
    free(srt);
    *n_regs = total;
    return BSW_OK;
}

/* the replay for arrays the plan has accepted, on up to `threads` threads (the job: bsw_chain2aln_job.hip); not part of the C ABI */
__attribute__((visibility("hidden")))
int bsw_c2a_replay_planned(const bsw_params *p, const bsw_c2a_opt *opt, const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds,
                           size_t n_seeds, const int32_t *lens, size_t n_reads, const void *results, int result_format, bsw_creg *regs,
                           size_t *n_regs, uint8_t *extended, uint64_t *reg_start, int threads);

int bsw_chain2aln_replay(const bsw_params *p, const bsw_c2a_opt *opt, const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds,
                         size_t n_seeds, const int32_t *lens, size_t n_reads, const void *results, int result_format, bsw_creg *regs,
                         size_t *n_regs, uint8_t *extended, uint64_t *reg_start)
{
    int rc;
    if ((rc = c2a_check("bsw_chain2aln_replay", chains, n_chains, seeds, n_seeds, lens, n_reads, NULL, 0))) return rc;
    return bsw_c2a_replay_planned(p, opt, chains, n_chains, seeds, n_seeds, lens, n_reads, results, result_format, regs, n_regs, extended, reg_start, 1);
}

#define C2A_MAX_THREADS 64
#define C2A_MIN_SEEDS_PER_THREAD 1024            /* ~50 us of replay: what starting a thread costs */
struct c2a_part {
    const bsw_params *p; const bsw_c2a_opt *o; const bsw_chain *chains; const bsw_cseed *seeds; const int32_t *lens; const void *results;
    size_t c0, c1, stride, count;
    bsw_creg *out;
    uint8_t *extended;
    uint64_t *reg_cnt;
    int rc;
};
static void *c2a_part_run(void *arg)
{
    struct c2a_part *q = (struct c2a_part *)arg;
    q->rc = c2a_replay_range(q->p, q->o, q->chains, q->c0, q->c1, q->seeds, q->lens, q->results, q->stride, q->out, &q->count, q->extended, q->reg_cnt);
    return NULL;
}

int bsw_c2a_replay_planned(const bsw_params *p, const bsw_c2a_opt *opt, const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds,
                           size_t n_seeds, const int32_t *lens, size_t n_reads, const void *results, int result_format, bsw_creg *regs,
                           size_t *n_regs, uint8_t *extended, uint64_t *reg_start, int threads)
{
    bsw_c2a_opt o;
    struct c2a_part part[C2A_MAX_THREADS];
    pthread_t th[C2A_MAX_THREADS];
    size_t c, total = 0, T, t, np = 0;
    int rc = BSW_OK;
    const size_t stride = result_format == BSW_RESULT_PAIR ? sizeof(bsw_pair) : sizeof(bsw_result);
    if (!p || !n_regs || (n_seeds && (!results || !regs)) || p->e_del < 1 || p->e_ins < 1) return BSW_E_INVAL;
    if (result_format != BSW_RESULT_FULL && result_format != BSW_RESULT_PAIR) return BSW_E_INVAL;
    if (opt) o = *opt; else bsw_c2a_default_opt(&o);
    if (extended && n_seeds) memset(extended, 0, n_seeds);
    if (reg_start) memset(reg_start, 0, (n_reads + 1) * sizeof(uint64_t));
    T = threads > 1 ? (size_t)threads : 1;
    if (T > C2A_MAX_THREADS) T = C2A_MAX_THREADS;
    if (T > n_seeds / C2A_MIN_SEEDS_PER_THREAD) T = n_seeds / C2A_MIN_SEEDS_PER_THREAD;
    if (T < 1) T = 1;
    /* parts of about n_seeds / T seeds, cut between two reads.  Part t writes its regions where its first seed's would go:
     * a part has at most as many regions as seeds, so the parts' outputs cannot meet; they are moved together afterwards */
    for (c = 0; c < n_chains && np < T; ) {
        struct c2a_part *q = &part[np];
        const size_t stop = np + 1 == T ? n_seeds : n_seeds * (np + 1) / T;
        size_t e = c + 1;
        while (e < n_chains && (chains[e].first_seed < stop || chains[e].read == chains[e - 1].read)) ++e;
        if (np + 1 == T) e = n_chains;
        q->p = p; q->o = &o; q->chains = chains; q->seeds = seeds; q->lens = lens; q->results = results; q->stride = stride;
        q->c0 = c; q->c1 = e; q->count = 0; q->out = regs + chains[c].first_seed; q->extended = extended; q->reg_cnt = reg_start ? reg_start + 1 : NULL; q->rc = BSW_OK;
        ++np;
        c = e;
    }
    for (t = 1; t < np; ++t)
        if (pthread_create(&th[t], NULL, c2a_part_run, &part[t]) != 0) break;
    {
        const size_t started = t;
        for (t = started; t < np; ++t) c2a_part_run(&part[t]);          /* (threads that could not be started: here, in turn) */
        if (np) c2a_part_run(&part[0]);
        for (t = 1; t < started; ++t) pthread_join(th[t], NULL);
    }
    for (t = 0; t < np; ++t) {
        if (part[t].rc && !rc) rc = part[t].rc;
        if (part[t].out != regs + total) memmove(regs + total, part[t].out, part[t].count * sizeof(bsw_creg));
        total += part[t].count;
    }
    if (reg_start) for (c = 0; c < n_reads; ++c) reg_start[c + 1] += reg_start[c];       /* counts -> starts */
    *n_regs = rc ? 0 : total;
    return rc;
}

/* ---- for the device replay (bsw_c2a_device.hip); not part of the C ABI ---- */
/* bsw_chain2aln_replay's pass over the arrays under another name, with the text */
__attribute__((visibility("hidden")))
int bsw_c2a_check_arrays(const char *who, const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds, size_t n_seeds, const int32_t *lens,
                         size_t n_reads, char *err, size_t err_cap)
{
    if (err && err_cap) err[0] = 0;
    return c2a_check(who, chains, n_chains, seeds, n_seeds, lens, n_reads, err, err_cap);
}
/* the host's loop over chains[c0, c1) — whole reads — into regs[0 .. *n_regs); indices in the regions are global; extended[] (may be
 * NULL) is only added to */
__attribute__((visibility("hidden")))
int bsw_c2a_replay_chains(const bsw_params *p, const bsw_c2a_opt *o, const bsw_chain *chains, size_t c0, size_t c1, const bsw_cseed *seeds,
                          const int32_t *lens, const void *results, size_t stride, bsw_creg *regs, size_t *n_regs, uint8_t *extended)
{
    return c2a_replay_range(p, o, chains, c0, c1, seeds, lens, results, stride, regs, n_regs, extended, NULL);
}
