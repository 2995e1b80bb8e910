/*
 * ksw_extend_rtl_ref.c — CPU reference for the three recurrence variants (test infrastructure, NOT product code).
 *
 * The oracle's side and pair loop (oracle/ksw_extend_ref.c: extend2_core, side_ref, bsw_pair_ref) with a variant
 * switch in which only two blocks of the row loop depend on BSW_VARIANT_RTL:
 *   K4  column 0 on every row, whatever beg is (sw_pe_array_sw_extend.v:1795-1796,1835,849; int32, the RTL's
 *       8-bit wrap is not reproduced);
 *   K8  the next row is trimmed to the run of non-zero eh[].h around mj, e ignored (:1767,1769,1779,1790,1872).
 * Everything else — the cell, first row, band clamp, row tail, m == 0 stop, zdrop, epilogue, MAX_BAND_TRY with fresh
 * state per pass, wlim, the pair decision and the cell count — is the oracle's, so for H and M this file computes the
 * oracle's bytes (tests/test_variant_rtl_cpu.py checks that).  Built by its test module with the system C compiler.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "bwa_sw_mi355.h"

typedef struct { int32_t h, e; } eh_t;

static int extend2_core(int qlen, const uint8_t *query, int tlen, const uint8_t *target,
                        int m, const int8_t *mat, int o_del, int e_del, int o_ins, int e_ins,
                        int w, int end_bonus, int zdrop, int h0,
                        int *qle_, int *tle_, int *gtle_, int *gscore_, int *max_off_,
                        int variant, uint64_t *cells_, int wlim)
{
    const int oe_del = o_del + e_del, oe_ins = o_ins + e_ins;
    eh_t *eh = (eh_t *)calloc((size_t)qlen + 2, sizeof(eh_t));
    int i, j, k, beg, end, max, max_i, max_j, max_ie, gscore, max_off, max_ins, max_del;
    uint64_t cells = 0;

    /* K2 first row */
    eh[0].h = h0;
    if (qlen >= 1) eh[1].h = h0 > oe_ins ? h0 - oe_ins : 0;
    for (j = 2; j <= qlen && eh[j - 1].h > e_ins; ++j) eh[j].h = eh[j - 1].h - e_ins;

    /* band clamp by the longest useful gap, or by the host's limit */
    for (i = 0, max = 0, k = m * m; i < k; ++i) max = max > mat[i] ? max : mat[i];
    max_ins = (int)((double)(qlen * max + end_bonus - o_ins) / e_ins + 1.);
    if (max_ins < 1) max_ins = 1;
    max_del = (int)((double)(qlen * max + end_bonus - o_del) / e_del + 1.);
    if (max_del < 1) max_del = 1;
    if (wlim > 0) max_ins = max_del = wlim;
    if (w > max_ins) w = max_ins;
    if (w > max_del) w = max_del;

    max = h0; max_i = max_j = -1; max_ie = -1; gscore = -1; max_off = 0;
    beg = 0; end = qlen;

    for (i = 0; i < tlen; ++i) {
        int f = 0, h1, mrow = 0, mj = -1;
        const int8_t *srow = &mat[target[i] * m];
        /* K3 band clamp */
        if (beg < i - w) beg = i - w;
        if (end > i + w + 1) end = i + w + 1;
        if (end > qlen) end = qlen;
        /* K4 column 0: H and M only while beg == 0, RTL on every row */
        if (beg == 0 || variant == BSW_VARIANT_RTL) {
            h1 = h0 - (o_del + e_del * (i + 1));
            if (h1 < 0) h1 = 0;
        } else h1 = 0;
        if (end > beg) cells += (uint64_t)(end - beg);
        for (j = beg; j < end; ++j) {                    /* K5 cell */
            eh_t *p = &eh[j];
            int h = p->h, e = p->e, s = srow[query[j]], t, base;
            p->h = h1;
            if (variant == BSW_VARIANT_M) {
                int M = h ? h + s : 0;
                h = M > e ? M : e;
                h = h > f ? h : f;
                base = M;
            } else {                                     /* H and RTL: the RTL's cell */
                h += s;
                h = h > e ? h : e;
                h = h > f ? h : f;
                base = h;
            }
            h1 = h;
            mj = mrow > h ? mj : j;
            mrow = mrow > h ? mrow : h;
            t = base - oe_del; if (t < 0) t = 0;
            e -= e_del; if (e < t) e = t;
            p->e = e;
            t = base - oe_ins; if (t < 0) t = 0;
            f -= e_ins; if (f < t) f = t;
        }
        eh[end].h = h1; eh[end].e = 0;                   /* K7 row tail */
        if (j == qlen) {
            max_ie = gscore > h1 ? max_ie : i;
            gscore = gscore > h1 ? gscore : h1;
        }
        if (mrow == 0) break;
        if (mrow > max) {
            int off = mj - i; if (off < 0) off = -off;
            max = mrow; max_i = i; max_j = mj;
            if (off > max_off) max_off = off;
        } else if (zdrop > 0) {
            if (i - max_i > mj - max_j) {
                if (max - mrow - ((i - max_i) - (mj - max_j)) * e_del > zdrop) break;
            } else {
                if (max - mrow - ((mj - max_j) - (i - max_i)) * e_ins > zdrop) break;
            }
        }
        if (variant == BSW_VARIANT_RTL) {
            /* K8, RTL: eh[j].h = H(i, j-1) here, eh[end].h = H(i, end-1); end may become end + 1 (K3 clamps it) */
            for (j = mj; j >= beg && eh[j].h; --j) {}
            beg = j + 1;
            for (j = mj + 2; j <= end && eh[j].h; ++j) {}
            end = j;
        } else {
            /* K8, CPU semantics */
            for (j = beg; j < end && eh[j].h == 0 && eh[j].e == 0; ++j) {}
            beg = j;
            for (j = end; j >= beg && eh[j].h == 0 && eh[j].e == 0; --j) {}
            end = j + 2 < qlen ? j + 2 : qlen;
        }
    }
    free(eh);
    if (qle_) *qle_ = max_j + 1;
    if (tle_) *tle_ = max_i + 1;
    if (gtle_) *gtle_ = max_ie + 1;
    if (gscore_) *gscore_ = gscore;
    if (max_off_) *max_off_ = max_off;
    if (cells_) *cells_ += cells;
    return max;
}

/* one plain ksw_extend2 call (m = 5), every output plus the cell count */
int rtl_ref_extend2(int qlen, const uint8_t *query, int tlen, const uint8_t *target, const int8_t *mat,
                    int o_del, int e_del, int o_ins, int e_ins, int w, int end_bonus, int zdrop, int h0,
                    int variant, int wlim, int32_t *out6, uint64_t *cells)
{
    int32_t *o = out6;
    *cells = 0;
    o[0] = extend2_core(qlen, query, tlen, target, 5, mat, o_del, e_del, o_ins, e_ins, w, end_bonus, zdrop, h0,
                        &o[1], &o[2], &o[3], &o[4], &o[5], variant, cells, wlim);
    return o[0];
}

static int side_ref(const bsw_params *p, int qlen, const uint8_t *q, int tlen, const uint8_t *t,
                    int end_bonus, int h0, int prev_score, int wlim, bsw_ext *x)
{
    int k, score = prev_score, tries = p->max_band_try > 0 ? p->max_band_try : 1;
    uint64_t cells = 0;
    memset(x, 0, sizeof(*x));
    for (k = 0; k < tries; ++k) {
        int prev = score, aw = p->w << k;
        score = extend2_core(qlen, q, tlen, t, 5, p->mat, p->o_del, p->e_del, p->o_ins, p->e_ins,
                             aw, end_bonus, p->zdrop, h0,
                             &x->qle, &x->tle, &x->gtle, &x->gscore, &x->max_off, p->variant, &cells, wlim);
        x->aw = aw;
        if (score == prev || x->max_off < (aw >> 1) + (aw >> 2)) break;
    }
    x->score = score;
    x->cells = (uint32_t)cells;
    return score;
}

static void pair_ref(const bsw_params *p, const bsw_task *t, bsw_result *r)
{
    int score = t->init_score, sc0;
    memset(r, 0, sizeof(*r));
    r->tag = t->tag;
    r->left.aw = r->right.aw = p->w;
    if (t->lqlen > 0) {
        score = side_ref(p, t->lqlen, t->lquery, t->ltlen, t->ltarget, p->pen_clip5, t->h0, score, t->wlim_l, &r->left);
        if (r->left.gscore <= 0 || r->left.gscore <= score - p->pen_clip5) {
            r->qb = t->qbeg - r->left.qle; r->rb = -r->left.tle; r->truesc = score;
        } else {
            r->qb = 0; r->rb = -r->left.gtle; r->truesc = r->left.gscore;
        }
    } else {
        score = r->truesc = t->h0; r->qb = 0; r->rb = 0;
    }
    sc0 = score;
    if (t->rqlen > 0) {
        score = side_ref(p, t->rqlen, t->rquery, t->rtlen, t->rtarget, p->pen_clip3, sc0, score, t->wlim_r, &r->right);
        if (r->right.gscore <= 0 || r->right.gscore <= score - p->pen_clip3) {
            r->qe = r->right.qle; r->re = r->right.tle; r->truesc += score - sc0;
        } else {
            r->qe = t->rqlen; r->re = r->right.gtle; r->truesc += r->right.gscore - sc0;
        }
    } else {
        r->qe = 0; r->re = 0;
    }
    r->score = score;
    r->w = r->left.aw > r->right.aw ? r->left.aw : r->right.aw;
}

void rtl_ref_pair_batch(const bsw_params *p, const bsw_task *tasks, size_t n, bsw_result *out)
{
    size_t i;
    for (i = 0; i < n; ++i) pair_ref(p, &tasks[i], &out[i]);
}

/* bsw_extend_batch's tasks: one ksw_extend2 pass each (no band retry), aw = the task's w */
void rtl_ref_ext_batch(const bsw_params *p, const bsw_ext_task *tasks, size_t n, bsw_ext *out)
{
    size_t i;
    for (i = 0; i < n; ++i) {
        const bsw_ext_task *t = &tasks[i];
        bsw_ext *x = &out[i];
        uint64_t cells = 0;
        memset(x, 0, sizeof(*x));
        x->score = extend2_core(t->qlen, t->query, t->tlen, t->target, 5, p->mat, p->o_del, p->e_del, p->o_ins, p->e_ins,
                                t->w, t->end_bonus, p->zdrop, t->h0,
                                &x->qle, &x->tle, &x->gtle, &x->gscore, &x->max_off, p->variant, &cells, 0);
        x->aw = t->w; x->cells = (uint32_t)cells;
    }
}
