/* bsw_cigar.hip — host of bsw_cigar_ref_batch: bwa_gen_cigar2 (bwa.c), inside mem_reg2aln's band-widening loop (bwamem.c),
 * against the device-resident reference (part of the host side of libbwasw_mi355.so).  Spans, class lists, routing, staging,
 * read-back and the sub-batch cutter are bsw_f4_host.h's; host-specific here, per chunk of tasks:
 *   1. how a task is laid out for bsw_pack_kernel: a forward-strand interval is a right-side-only seed (read forwards, target
 *      upwards from rb); a reverse-strand one a left-side-only seed (read backwards from its last base, target downwards from
 *      re - 1): that is bwa's reversal of both, for free;
 *   2. the tries: each runs the global kernels on the tasks still in the loop, with their band and a fresh slice of the backtrack
 *      matrix; only the scores come back between tries, the packed sequences stay where they are.  A try whose band (after bwa's
 *      formula) equals the previous one's would return the previous score and end the loop on "score == last": it is counted, not run;
 *   3. bsw_cigar_md_kernel derives NM and MD once per task from its final CIGAR, and settles bwa's no-gap shortcut.
 * A chunk runs on a LANE (f4_lane, bsw_internal.h): the context's own for bsw_cigar_ref_batch, a pipeline slot's for the chunks of
 * bsw_cigar_ref_submit_t (bsw_batch.hip), which reads back into pinned memory in front of the watchdog's wait.
 * Behind it, in the second half of the file: mem_patch_reg (bsw_patch_ref_batch and its ticket forms), which is one try of the
 * above for its score alone, between two pieces of host arithmetic. */
#include "bsw_f4_host.h"

#include <climits>

/* bwa_gen_cigar2's band for a try with w_ (the no-gap shortcut aside) */
static int gen_cigar_band(const bsw_params &p, int l_query, int rlen, int w_)
{
    const int max_ins = (int)((double)(((l_query + 1) >> 1) * p.mat[0] - p.o_ins) / p.e_ins + 1.);
    const int max_del = (int)((double)(((l_query + 1) >> 1) * p.mat[0] - p.o_del) / p.e_del + 1.);
    int max_gap = max_ins > max_del ? max_ins : max_del;
    max_gap = max_gap > 1 ? max_gap : 1;
    const int d = abs(rlen - l_query);
    int w = (max_gap + d + 1) >> 1;
    w = w < w_ ? w : w_;
    return w > d + 3 ? w : d + 3;
}

/* the pack kernel reads a word of a sequence as 20 bytes from the dword below its first byte: forwards up to 16 + 3 bytes past
 * a read's end, backwards (reverse strand) down to 15 + 3 bytes before its start */
static_assert(RAW_FRONT >= 18 && RAW_SLACK >= 20, "raw slack of the reads");

struct cstate {                       /* one task's place in mem_reg2aln's loop */
    int w2, wcap, last, tries, band;
    bool live;                        /* still has a try to run */
};

/* task i of a chunk in the pointer form's terms: the caller's record, or the one a resident-read task stands for (query stays
 * NULL: the bases are on the device already; l_query = qe - qb, checked at submit) */
static inline bsw_ctask ctask_of(const bsw_ctask *tasks, const bsw_rd_ctask *rtasks, size_t i)
{
    if (!rtasks) return tasks[i];
    const bsw_rd_ctask &r = rtasks[i];
    bsw_ctask t;
    t.query = nullptr; t.l_query = r.qe - r.qb; t.w = r.w; t.rb = r.rb; t.re = r.re; t.w_cap = r.w_cap; t.min_score = r.min_score;
    t.max_tries = r.max_tries; t._pad = 0;
    return t;
}

/* rd != NULL: the chunk's tasks are rtasks[0..n) and name reads of the resident block (tasks is NULL then): the per-task work is
 * the device records plus a base position — no span, no registration test, no gather, no raw bytes */
static int cigar_chunk(bsw_ctx *ctx, errs &e, f4_lane &L, const bsw_params &pp, const bsw_dparams &dp, const bsw_ref *ref, const bsw_ctask *tasks,
                       size_t n, int max_cigar, uint32_t *cigars, int max_md, char *md, bsw_cresult *res,
                       const bsw_reads *rd, const bsw_rd_ctask *rtasks)
{
    stage_t &st = *L.st;
    hipStream_t s = L.s;
    const int64_t l_pac = ref->l_pac;
    int rc = stage_records(e, st, n, true);
    if (rc) return rc;
    std::vector<bsw_gdtask> gt(n);
    std::vector<bsw_cdtask> cd(n);
    std::vector<cstate> cs(n);
    uint64_t acc = 0;
    raw_span sp;
    for (size_t i = 0; i < n; ++i) {
        const bsw_ctask t = ctask_of(tasks, rtasks, i);
        bsw_cdtask &c = cd[i];
        memset(&c, 0, sizeof(c));
        cstate &q = cs[i];
        q = cstate{0, 0, -(1 << 30), 0, 0, false};
        q.wcap = t.w_cap ? t.w_cap : t.w;
        q.w2 = t.w < q.wcap ? t.w : q.wcap;
        /* bwa: no alignment for an empty read, an empty or bridging interval, or one bns_get_seq cannot return whole */
        if (t.l_query == 0 || t.rb >= t.re || (t.rb < l_pac && t.re > l_pac) || t.rb < 0 || t.re > 2 * l_pac) {
            c.flags = BSW_CD_STATUS;
            clear_records(st, i);
            continue;
        }
        const int rlen = (int)(t.re - t.rb);
        const bool rev = t.rb >= l_pac;           /* the reverse strand: a left-side-only seed */
        /* where the slice starts: a byte offset into the raw bytes, or (resident reads) the position of base qb of its read */
        const uint32_t at = rd ? rd->pos(rtasks[i].read) + (uint32_t)rtasks[i].qb : (uint32_t)sp.bytes;
        const interval_words iw = lay_interval(st, i, t.l_query, rlen, rev, at, t.rb, t.re, acc);
        const uint32_t qw = iw.qw, tw = iw.tw;
        if (!rd) sp.add(t.query, (size_t)t.l_query);
        c.q_off = qw; c.t_off = tw; c.qlen = t.l_query; c.tlen = rlen;
        c.flags = rev ? BSW_CD_REV : 0u;
        if (t.l_query == rlen && q.w2 == 0) {            /* the no-gap shortcut: the NM / MD kernel does it */
            c.flags |= BSW_CD_NOGAP;
            c.min_score = t.min_score;
            c.more = (q.wcap != 0 && (t.max_tries > 1)) ? 1 : 0;     /* a second try: same band, same score, then "score == last" */
            q.tries = 1;
            continue;
        }
        q.band = gen_cigar_band(pp, t.l_query, rlen, q.w2);
        q.live = true;
        bsw_gdtask &g = gt[i];
        g.q_off = qw; g.t_off = tw; g.qlen = t.l_query; g.tlen = rlen; g.w = q.band; g.pad = 0; g.z_off = 0;
    }
    /* the reads: either way a reverse-strand read's offset names its LAST byte and the pack kernel reads it backwards */
    staged_raw raw;
    rc = stage_raw(e, st, n, sp, acc, true, false, 1, [&](size_t i, int) {
        if (cd[i].flags & BSW_CD_STATUS) return raw_piece{nullptr, 0, &bsw_rawoff::rq, false};
        const bool rev = (cd[i].flags & BSW_CD_REV) != 0;
        return raw_piece{tasks[i].query, (size_t)tasks[i].l_query, rev ? &bsw_rawoff::lq : &bsw_rawoff::rq, rev};
    }, &raw);
    if (rc) return rc;
    /* backtrack room: the widest band any try can reach is the formula's own (w_ only caps it) */
    uint64_t zmax = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!cs[i].live) continue;
        const int wmax = gen_cigar_band(pp, cd[i].qlen, cd[i].tlen, INT_MAX);
        zmax += (uint64_t)std::min(cd[i].qlen, 2 * wmax + 1) * (uint64_t)cd[i].tlen;
    }
    if ((rc = reserve_all(e, "device staging", {{L.b->g_tasks, n + 1}, {L.b->g_order, n + 1}, {L.b->g_res, n + 1}, {L.b->g_z, (size_t)zmax + 64}, {L.b->g_cig, n * (size_t)max_cigar + 1},
                                                {L.b->c_tasks, n + 1}, {L.b->c_res, n + 1}, {L.b->c_md, n * (size_t)max_md + 1, md != nullptr}})) != BSW_OK) return rc;
    /* a slot reads back into pinned memory: the scores of a try, then results | CIGARs | MD slots */
    const size_t cigb = cigars ? n * (size_t)max_cigar * sizeof(uint32_t) : 0, mdb = md ? n * (size_t)max_md : 0;
    const size_t in_gt = (n + 1) * sizeof(bsw_cdtask), in_order = in_gt + (n + 1) * sizeof(bsw_gdtask);
    if (L.h_back && (rc = reserve_all(e, "pinned staging", {{*L.h_back, std::max(n * sizeof(bsw_cresult) + cigb + mdb, n * sizeof(bsw_gresult)) + 16},
                                                            {*L.h_in, in_order + (n + 1) * sizeof(uint32_t)}})) != BSW_OK) return rc;
    /* what the tries need (declared here: the guard behind them is destroyed first) */
    std::vector<bsw_gresult> gr(L.h_back ? 0 : n);
    const bsw_gresult *grp = L.h_back ? (const bsw_gresult *)L.h_back->p : gr.data();
    class_lists cl;
    const global_route route;
    std::vector<uint32_t> cls, live;
    drain_on_failure drain(ctx, s, L.ev);
    if ((rc = stage_upload(e, L, raw, n)) != BSW_OK) return rc;
    HIPCHK(e, hipMemcpyAsync(L.b->c_tasks.p, L.dma_src(cd.data(), n * sizeof(bsw_cdtask), 0), n * sizeof(bsw_cdtask), hipMemcpyHostToDevice, s));
    L.h2d += n * sizeof(bsw_cdtask);
    if ((rc = stage_pack(e, L, n, BSW_PACK_REV_LEFT, ref, rd)) != BSW_OK) return rc;

    /* the tries: each launches the global kernels on the tasks still in the loop, then reads their scores */
    for (size_t i = 0; i < n; ++i) if (cs[i].live) live.push_back((uint32_t)i);
    while (!live.empty()) {
        if (L.abort && L.abort->load()) return fail(e, BSW_E_HIP, "aborted: another chunk failed");
        cls.assign(live.size(), 0u);
        uint64_t zacc = 0;
        for (size_t k = 0; k < live.size(); ++k) {
            bsw_gdtask &g = gt[live[k]];
            g.w = cs[live[k]].band;
            g.z_off = zacc;
            const int n_col = g.qlen < 2 * g.w + 1 ? g.qlen : 2 * g.w + 1;
            zacc += (uint64_t)n_col * (uint64_t)g.tlen;
            cls[k] = (uint32_t)route(g.qlen, n_col);     /* bsw_global_batch's routing */
        }
        cl.build(route.classes(), cls.data(), live.data(), live.size());
        if ((rc = upload_launch_global(e, L, cl, dp, gt.data(), n, in_gt, in_order, L.b->g_z.p, L.b->g_cig.p, max_cigar)) != BSW_OK) return rc;
        if ((rc = lane_read_back(ctx, e, L, {{L.h_back ? nullptr : gr.data(), L.b->g_res.p, n * sizeof(bsw_gresult)}})) != BSW_OK) return rc;
        /* mem_reg2aln: if (score == last || w2 == w_cap) break; last = score; w2 <<= 1; } while (++i < max_tries && score < min_score) */
        std::vector<uint32_t> next;
        for (uint32_t i : live) {
            cstate &q = cs[i];
            const bsw_ctask t = ctask_of(tasks, rtasks, i);
            const int score = grp[i].score;
            ++q.tries;
            q.live = false;
            if (score == q.last || q.w2 == q.wcap) continue;
            q.last = score;
            const int max_tries = t.max_tries ? t.max_tries : 1;
            if (!(q.tries < max_tries && score < t.min_score)) continue;
            q.w2 = std::min(q.w2 << 1, q.wcap);
            const int band = gen_cigar_band(pp, cd[i].qlen, cd[i].tlen, q.w2);
            if (band == q.band) {         /* the same alignment again: its score equals `last` and the loop ends there */
                ++q.tries;
                continue;
            }
            q.band = band;
            q.live = true;
            next.push_back(i);
        }
        live.swap(next);
    }
    HIPCHK(e, bsw::launch_cigar_md(dp, st.d_seq.p, L.b->c_tasks.p, (uint32_t)n, L.b->g_cig.p, max_cigar, L.b->g_res.p,
                                   md ? L.b->c_md.p : nullptr, max_md, L.b->c_res.p, s));
    rc = lane_read_back(ctx, e, L, {{res, L.b->c_res.p, n * sizeof(bsw_cresult)}, {cigars, L.b->g_cig.p, cigb}, {md, L.b->c_md.p, mdb}});
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) {
        bsw_cresult &r = res[i];
        if (cd[i].flags & BSW_CD_STATUS) {
            r = bsw_cresult{0, 0, -1, 0, cs[i].w2, 1, 1, 0};
            continue;
        }
        r.w = cs[i].w2;
        if (!(cd[i].flags & BSW_CD_NOGAP)) r.tries = cs[i].tries;
        r.status = 0;
        r._pad = 0;
    }
    drain.done();
    return BSW_OK;
}

/* what both entry points check before anything runs or is queued: the parameters (the band is per task: pp gets w = 0), then
 * the tasks in order — the first malformed one rejects the call */
static int cigar_validate(errs &e, const bsw_params *p, const bsw_ctask *tasks, size_t n, bsw_params *pp, bsw_dparams *dp,
                          const bsw_reads *rd = nullptr, const bsw_rd_ctask *rtasks = nullptr)
{
    *pp = *p;
    pp->w = 0;                                        /* the band is per task here */
    int rc = check_params(e, pp, dp);
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) {
        if (rd) {                                     /* the slice lies inside its read: nothing else may reach the kernel */
            const bsw_rd_ctask &r = rtasks[i];
            if (r.read >= rd->rd.size()) return fail(e, BSW_E_INVAL, "cigar task %zu: read %u is not in the block of %zu reads", i, r.read, rd->rd.size());
            if (r.qb < 0 || r.qe < r.qb || r.qe > rd->rd[r.read].len)
                return fail(e, BSW_E_INVAL, "cigar task %zu: [qb, qe) = [%d, %d) is not inside read %u of %d bases", i, r.qb, r.qe, r.read, rd->rd[r.read].len);
        }
        const bsw_ctask t = ctask_of(tasks, rtasks, i);
        if (t.l_query < 0 || t.w < 0 || t.w_cap < 0 || t.max_tries < 0 || t.max_tries > 3)
            return fail(e, BSW_E_INVAL, "cigar task %zu: negative length or band, or max_tries outside 0..3", i);
        if (t.l_query && !t.query && !rd) return fail(e, BSW_E_INVAL, "cigar task %zu: NULL read", i);
        if (t.l_query > BSW_GLOBAL_MAX_QLEN || t.w > BSW_MAX_TLEN || t.w_cap > BSW_MAX_TLEN || (t.re > t.rb && t.re - t.rb > BSW_MAX_TLEN))
            return fail(e, BSW_E_LIMIT, "cigar task %zu: beyond BSW_GLOBAL_MAX_QLEN / BSW_MAX_TLEN", i);
    }
    return BSW_OK;
}

/* backtrack bytes (its widest band) and sequence bytes one task adds to a sub-batch */
static void cigar_task_cost(const bsw_params &pp, const bsw_ctask &t, uint64_t &nz, uint64_t &ns)
{
    nz = ns = 0;
    if (t.l_query > 0 && t.re > t.rb && t.re - t.rb <= BSW_MAX_TLEN) {
        const int rlen = (int)(t.re - t.rb), wmax = gen_cigar_band(pp, t.l_query, rlen, INT_MAX);
        nz = (uint64_t)std::min(t.l_query, 2 * wmax + 1) * (uint64_t)rlen;
        ns = (uint64_t)t.l_query + (uint64_t)rlen;
    }
}

extern "C" int bsw_cigar_ref_batch(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_ctask *tasks, size_t n,
                                   int max_cigar, uint32_t *cigars, int max_md, char *md, bsw_cresult *res)
{
    if (!ctx) return BSW_E_INVAL;
    errs &e = ctx->err;
    int rc = ref_entry_check(ctx, "bsw_cigar_ref_batch", !p || !ref || (!tasks && n) || (!res && n) || max_cigar < 1 || (md && max_md < 1), ref, false);
    if (rc) return rc;
    bsw_params pp;
    bsw_dparams dp;
    rc = cigar_validate(e, p, tasks, n, &pp, &dp);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(ctx->device0()));
    f4_lane L = ctx_lane(ctx);
    /* sub-batches: bounded backtrack memory (the widest band of any try) and sequence arena, as bsw_global_batch */
    const std::vector<chunk_span> spans = cut_spans(n, [&](size_t i) {
        uint64_t nz, ns;
        cigar_task_cost(pp, tasks[i], nz, ns);
        return span_cost{nz, ns, 0, 0, nz, 0};
    }, span_caps());
    for (const chunk_span &c : spans) {
        rc = cigar_chunk(ctx, e, L, pp, dp, ref, tasks + c.base, c.cnt, max_cigar, cigars ? cigars + c.base * (size_t)max_cigar : nullptr, max_md,
                         md ? md + c.base * (size_t)max_md : nullptr, res + c.base, nullptr, nullptr);
        if (rc) return rc;
    }
    return BSW_OK;
}

/* The work target of a CIGAR chunk, in cells (min(l_query, 2 w + 1) x (re - rb) with the widest band a try can reach, summed
 * over its tasks — the chunk's backtrack bytes), from the sweep of tools/f4_stream_rate.py ("sweep_cigar" of
 * profiles/f4_stream_rate.json): 65 536 alignments of 150 bases take 13.5 / 14.7 / 8.1 / 9.6 / 9.1 / 8.6 / 9.3 ms at
 * 2^24 .. 2^30, runs of one cut differing by up to 15 %; 2^28 (~25 k alignments a chunk) is on the plateau and two steps from the
 * cliff at 2^25.  BSW_F4_CIGAR_WORK overrides it (tests, measurements). */
#define F4_CIGAR_CHUNK_WORK (1ull << 28)
#define F4_CIGAR_OUT_MAX (1ull << 30)                  /* CIGAR words and MD slots of a chunk: 1 GiB each at the most */
static uint64_t cigar_chunk_work()
{
    static const uint64_t v = chunk_work_env("BSW_F4_CIGAR_WORK", F4_CIGAR_CHUNK_WORK);
    return v;
}

/* bsw_cigar_ref_batch as a ticket of the context's pipeline: the same checks in the caller's thread, then chunks of about
 * cigar_chunk_work() cells (within the batch call's bounds, and F4_CIGAR_OUT_MAX bytes of CIGAR / MD room) through the slots
 * of every device, chunk k on device k mod n_devices against that device's copy of the reference. */
/* both ticket forms: tasks (pointer form) or rd + rtasks (resident reads) */
static int cigar_submit(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_ctask *tasks, const bsw_reads *rd, const bsw_rd_ctask *rtasks,
                        size_t n, int max_cigar, uint32_t *cigars, int max_md, char *md, bsw_cresult *res, bsw_ticket *ticket, const char *what)
{
    if (!ctx) return BSW_E_INVAL;
    if (ticket) *ticket = 0;
    int rc = ref_entry_check(ctx, what, !p || !ref || (!tasks && !rtasks && n) || (!res && n) || max_cigar < 1 || (md && max_md < 1), ref, true);
    if (rc) return rc;
    errs e;                                          /* (several threads may submit at once: the context's text is set under its lock) */
    bsw_params pp;
    bsw_dparams dp;
    rc = cigar_validate(e, p, tasks, n, &pp, &dp, rd, rtasks);
    if (rc) return ctx_fail(ctx, e, rc);
    f4_submit f;
    f.name = "cigar"; f.rd = rd;
    f.run = [=](bsw_ctx *cx, errs &ce, f4_lane &L, chunk_span c) {
        return cigar_chunk(cx, ce, L, pp, dp, ref, tasks ? tasks + c.base : nullptr, c.cnt, max_cigar, cigars ? cigars + c.base * (size_t)max_cigar : nullptr, max_md,
                           md ? md + c.base * (size_t)max_md : nullptr, res + c.base, rd, rd ? rtasks + c.base : nullptr);
    };
    std::vector<uint64_t> nz(n), ns(n);               /* one walk over the tasks: the band formula is the cost of this pass */
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) { cigar_task_cost(pp, ctask_of(tasks, rtasks, i), nz[i], ns[i]); total += nz[i]; }
    span_caps caps;                                   /* the batch call's bounds, the room of the outputs, and the work of a chunk */
    caps.work = std::min<uint64_t>(f4_chunk_work(ctx, total, cigar_chunk_work()), 4ull << 30);
    caps.out_per_task = std::max<uint64_t>((uint64_t)max_cigar * sizeof(uint32_t), md ? (uint64_t)max_md : 0);
    caps.out = F4_CIGAR_OUT_MAX;
    f.spans = cut_spans(n, [&](size_t i) { return span_cost{nz[i], ns[i], 0, nz[i], nz[i], 0}; }, caps);
    return pipeline_submit_f4(ctx, std::move(f), ticket, what);
}

extern "C" int bsw_cigar_ref_submit_t(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_ctask *tasks, size_t n,
                                      int max_cigar, uint32_t *cigars, int max_md, char *md, bsw_cresult *res, bsw_ticket *ticket)
{
    return cigar_submit(ctx, p, ref, tasks, nullptr, nullptr, n, max_cigar, cigars, max_md, md, res, ticket, "bsw_cigar_ref_submit");
}

/* the same against a resident read block: a task names its read by index and the slice by [qb, qe) */
extern "C" int bsw_cigar_reads_submit_t(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_reads *rd, const bsw_rd_ctask *tasks,
                                        size_t n, int max_cigar, uint32_t *cigars, int max_md, char *md, bsw_cresult *res, bsw_ticket *ticket)
{
    return reads_submit(ctx, rd, ticket, "bsw_cigar_reads_submit",
                        [&] { return cigar_submit(ctx, p, ref, nullptr, rd, tasks, n, max_cigar, cigars, max_md, md, res, ticket, "bsw_cigar_reads_submit"); });
}

/* ======== mem_patch_reg (bwamem.c, bwa >= 0.7.10; restated as recalled): bsw_patch_ref_batch and its ticket forms ========
 * The two halves around the alignment run on the host: the pre-tests before a task is staged, the 0.90 test once its score is
 * back.  Between them a chunk is a cigar_chunk of one try without its outputs: the same records for bsw_pack_kernel (the slice
 * starts at base a.qb of the read), ONE round of the global kernels with z == NULL and cigars == NULL, and 8 bytes per task back.
 * The few tasks of bwa's no-gap shortcut are gathered into records of their own for bsw_cigar_md_kernel, which sums their matrix
 * entries (its one CIGAR word per such task is the only CIGAR room a chunk reserves; no MD slot, no backtrack matrix). */

/* everything before bwa_gen_cigar2; 64-bit where bwa's int would overflow on values no aligner produces */
static int patch_pretest(const bsw_params &p, int64_t l_pac, const bsw_preg &a, const bsw_preg &b, int *w_out)
{
    if (a.rb < l_pac && b.rb >= l_pac) return 0;                                    /* different strands */
    if (a.qb >= b.qb || a.qe >= b.qe || a.re >= b.re) return 0;                     /* not colinear */
    int64_t w = (a.re - b.rb) - ((int64_t)a.qe - b.qb);
    w = w > 0 ? w : -w;
    double r = (double)(a.re - b.rb) / (double)(b.re - a.rb) - (double)(a.qe - b.qb) / (double)(b.qe - a.qb);
    r = r > 0. ? r : -r;
    const int64_t ow = p.w;
    if (a.re < b.rb || a.qe < b.qb) {                                               /* a gap between them: the tighter limits */
        if (w > ow << 1 || r >= 0.05f) return 0;
    } else if (w > ow << 2 || r >= 0.05f * 2) return 0;
    w += (int64_t)a.w + b.w;
    w = w < ow << 2 ? w : ow << 2;
    if (w_out) *w_out = (int)std::min<int64_t>(w, INT_MAX);
    return 1;
}

/* everything behind it: the return value */
static int patch_decide(const bsw_preg &a, const bsw_preg &b, int score)
{
    const double sum = (double)((int64_t)b.score + a.score);
    const double qd = (double)(b.qe - a.qb) / (double)(((int64_t)b.qe - b.qb) + ((int64_t)a.qe - a.qb)) * sum + .499;
    const double rd = (double)(b.re - a.rb) / (double)((b.re - b.rb) + (a.re - a.rb)) * sum + .499;
    auto to_int = [](double v) { return v >= 2147483647. ? INT_MAX : v > -2147483648. ? (int)v : INT_MIN; };   /* (out of int's range, NaN: as x86's conversion answers) */
    const int q_s = to_int(qd), r_s = to_int(rd);
    if ((double)score / (double)(q_s > r_s ? q_s : r_s) < 0.90f) return 0;
    return score;
}

extern "C" int bsw_patch_pretest(const bsw_params *p, int64_t l_pac, const bsw_preg *a, const bsw_preg *b, int *w)
{
    if (w) *w = 0;
    if (!p || !a || !b) return 0;
    return patch_pretest(*p, l_pac, *a, *b, w);
}
extern "C" int bsw_patch_decide(const bsw_preg *a, const bsw_preg *b, int gscore)
{
    if (!a || !b) return 0;
    return patch_decide(*a, *b, gscore);
}

/* task i in the pointer form's terms (resident reads: query stays NULL, l_query is the read's length) */
static inline bsw_ptask ptask_of(const bsw_ptask *tasks, const bsw_reads *rd, const bsw_rd_ptask *rtasks, size_t i)
{
    if (!rtasks) return tasks[i];
    const bsw_rd_ptask &r = rtasks[i];
    bsw_ptask t;
    t.query = nullptr; t.l_query = r.read < rd->rd.size() ? rd->rd[r.read].len : -1; t._pad = 0; t.a = r.a; t.b = r.b;
    return t;
}

/* does task t reach the GPU?  Its band w_, and whether bwa_gen_cigar2 has an alignment for [a.rb, b.re) at all */
static inline bool patch_runs(const bsw_params &pp, int64_t l_pac, const bsw_ptask &t, int *w_)
{
    if (!patch_pretest(pp, l_pac, t.a, t.b, w_)) return false;
    const int64_t rb = t.a.rb, re = t.b.re;
    return !((rb < l_pac && re > l_pac) || rb < 0 || re > 2 * l_pac);
}

/* pp.w is opt->w here, not taken out as for the other two stages; rd / rtasks as for cigar_chunk */
static int patch_chunk(bsw_ctx *ctx, errs &e, f4_lane &L, const bsw_params &pp, const bsw_dparams &dp, const bsw_ref *ref, const bsw_ptask *tasks,
                       size_t n, bsw_presult *res, const bsw_reads *rd, const bsw_rd_ptask *rtasks)
{
    stage_t &st = *L.st;
    hipStream_t s = L.s;
    const int64_t l_pac = ref->l_pac;
    int rc = stage_records(e, st, n, true);
    if (rc) return rc;
    std::vector<bsw_gdtask> gt(n);
    std::vector<bsw_cdtask> cd;                       /* the no-gap shortcut's tasks, gathered */
    std::vector<uint32_t> live, cd_of, cls;
    std::vector<uint8_t> rev(n, 0);
    const global_route route;
    uint64_t acc = 0;
    raw_span sp;
    for (size_t i = 0; i < n; ++i) {
        const bsw_ptask t = ptask_of(tasks, rd, rtasks, i);
        memset(&gt[i], 0, sizeof(bsw_gdtask));
        res[i] = bsw_presult{0, 0, 0, 1};
        int w_ = 0;
        if (!patch_runs(pp, l_pac, t, &w_)) {
            clear_records(st, i);
            continue;
        }
        const int lq = t.b.qe - t.a.qb, rlen = (int)(t.b.re - t.a.rb);
        rev[i] = t.a.rb >= l_pac;         /* the reverse strand: a left-side-only seed */
        /* where the slice starts: a byte offset into the raw bytes, or (resident reads) the position of base a.qb of its read */
        const uint32_t at = rd ? rd->pos(rtasks[i].read) + (uint32_t)t.a.qb : (uint32_t)sp.bytes;
        const interval_words iw = lay_interval(st, i, lq, rlen, rev[i] != 0, at, t.a.rb, t.b.re, acc);
        const uint32_t qw = iw.qw, tw = iw.tw;
        if (!rd) sp.add(t.query + t.a.qb, (size_t)lq);
        res[i].w = w_;
        res[i].status = 0;                /* (runs: settled below) */
        if (lq == rlen && w_ == 0) {      /* the no-gap shortcut: the NM / MD kernel sums the matrix entries */
            bsw_cdtask c;
            memset(&c, 0, sizeof(c));
            c.q_off = qw; c.t_off = tw; c.qlen = lq; c.tlen = rlen;
            c.flags = BSW_CD_NOGAP | (rev[i] ? BSW_CD_REV : 0u);
            cd.push_back(c);
            cd_of.push_back((uint32_t)i);
            continue;
        }
        bsw_gdtask &g = gt[i];
        g.q_off = qw; g.t_off = tw; g.qlen = lq; g.tlen = rlen; g.w = gen_cigar_band(pp, lq, rlen, w_);
        const int n_col = g.qlen < 2 * g.w + 1 ? g.qlen : 2 * g.w + 1;
        live.push_back((uint32_t)i);
        cls.push_back((uint32_t)route(g.qlen, n_col));
    }
    if (live.empty() && cd.empty()) return BSW_OK;    /* nothing passed the pre-tests: no HIP call */
    staged_raw raw;
    rc = stage_raw(e, st, n, sp, acc, true, false, 1, [&](size_t i, int) {
        if (res[i].status) return raw_piece{nullptr, 0, &bsw_rawoff::rq, false};
        return raw_piece{tasks[i].query + tasks[i].a.qb, (size_t)(tasks[i].b.qe - tasks[i].a.qb), rev[i] ? &bsw_rawoff::lq : &bsw_rawoff::rq, rev[i] != 0};
    }, &raw);
    if (rc) return rc;
    const size_t nc = cd.size();
    if ((rc = reserve_all(e, "device staging", {{L.b->g_tasks, n + 1}, {L.b->g_order, n + 1}, {L.b->g_res, n + 1},
                                                {L.b->c_tasks, nc + 1, nc != 0}, {L.b->c_res, nc + 1, nc != 0}, {L.b->g_cig, nc + 1, nc != 0}})) != BSW_OK) return rc;
    /* a slot reads back into pinned memory: the scores | the shortcut's records */
    const size_t in_gt = (nc + 1) * sizeof(bsw_cdtask), in_order = in_gt + (n + 1) * sizeof(bsw_gdtask);
    if (L.h_back && (rc = reserve_all(e, "pinned staging", {{*L.h_back, n * sizeof(bsw_gresult) + nc * sizeof(bsw_cresult) + 16}, {*L.h_in, in_order + (n + 1) * sizeof(uint32_t)}})) != BSW_OK)
        return rc;
    std::vector<bsw_gresult> gr(live.empty() ? 0 : n);
    std::vector<bsw_cresult> cr(nc);
    class_lists cl;
    cl.build(route.classes(), cls.data(), live.data(), live.size());
    drain_on_failure drain(ctx, s, L.ev);
    if ((rc = stage_upload(e, L, raw, n)) != BSW_OK) return rc;
    if ((rc = stage_pack(e, L, n, BSW_PACK_REV_LEFT, ref, rd)) != BSW_OK) return rc;
    if (!live.empty() && (rc = upload_launch_global(e, L, cl, dp, gt.data(), n, in_gt, in_order, nullptr, nullptr, 0)) != BSW_OK) return rc;
    if (nc) {
        HIPCHK(e, hipMemcpyAsync(L.b->c_tasks.p, L.dma_src(cd.data(), nc * sizeof(bsw_cdtask), 0), nc * sizeof(bsw_cdtask), hipMemcpyHostToDevice, s));
        L.h2d += nc * sizeof(bsw_cdtask);
        HIPCHK(e, bsw::launch_cigar_md(dp, st.d_seq.p, L.b->c_tasks.p, (uint32_t)nc, L.b->g_cig.p, 1, L.b->g_res.p, nullptr, 0, L.b->c_res.p, s));
    }
    rc = lane_read_back(ctx, e, L, {{gr.data(), L.b->g_res.p, gr.size() * sizeof(bsw_gresult)}, {cr.data(), L.b->c_res.p, nc * sizeof(bsw_cresult)}});
    if (rc) return rc;
    for (uint32_t i : live) res[i].gscore = gr[i].score;
    for (size_t k = 0; k < nc; ++k) res[cd_of[k]].gscore = cr[k].score;
    for (size_t i = 0; i < n; ++i) {
        if (res[i].status) continue;
        const bsw_ptask t = ptask_of(tasks, rd, rtasks, i);
        res[i].score = patch_decide(t.a, t.b, res[i].gscore);
        res[i].status = res[i].score > 0 ? 0 : 2;
    }
    drain.done();
    return BSW_OK;
}

/* what all three entry points check before anything runs or is queued; *pp keeps p->w (opt->w).  cells[i] (may be NULL):
 * the banded cells of task i, 0 for one that does not reach the GPU; seqb[i]: its sequence bytes */
static int patch_validate(errs &e, const bsw_params *p, const bsw_ref *ref, const bsw_ptask *tasks, const bsw_reads *rd, const bsw_rd_ptask *rtasks,
                          size_t n, bsw_params *pp, bsw_dparams *dp, std::vector<uint64_t> &cells, std::vector<uint64_t> &seqb)
{
    bsw_params p0 = *p;
    p0.w = 0;                                         /* (the kernels' band is per task) */
    int rc = check_params(e, &p0, dp);
    if (rc) return rc;
    if (p->w < 0) return fail(e, BSW_E_INVAL, "patch: negative band w = %d", p->w);
    *pp = *p;
    cells.assign(n, 0);
    seqb.assign(n, 0);
    for (size_t i = 0; i < n; ++i) {
        if (rd && rtasks[i].read >= rd->rd.size())
            return fail(e, BSW_E_INVAL, "patch task %zu: read %u is not in the block of %zu reads", i, rtasks[i].read, rd->rd.size());
        const bsw_ptask t = ptask_of(tasks, rd, rtasks, i);
        if (t.l_query < 0) return fail(e, BSW_E_INVAL, "patch task %zu: negative length", i);
        if (t.l_query && !t.query && !rd) return fail(e, BSW_E_INVAL, "patch task %zu: NULL read", i);
        for (const bsw_preg *g : {&t.a, &t.b}) {
            if (g->rb >= g->re) return fail(e, BSW_E_INVAL, "patch task %zu: region with rb >= re", i);
            if (g->qb < 0 || g->qb >= g->qe || g->qe > t.l_query)
                return fail(e, BSW_E_INVAL, "patch task %zu: [qb, qe) = [%d, %d) is not a slice of the read of %d bases", i, g->qb, g->qe, t.l_query);
            if (g->w < 0) return fail(e, BSW_E_INVAL, "patch task %zu: negative band", i);
        }
        if (t.a.rb > t.b.rb) return fail(e, BSW_E_INVAL, "patch task %zu: a.rb > b.rb (bwa asserts a.rb <= b.rb)", i);
        if ((int64_t)t.a.score + t.b.score <= 0) return fail(e, BSW_E_INVAL, "patch task %zu: a.score + b.score <= 0", i);
        int w_ = 0;
        if (!patch_runs(*pp, ref->l_pac, t, &w_)) continue;
        const int64_t lq = (int64_t)t.b.qe - t.a.qb, rlen = t.b.re - t.a.rb;
        if (lq > BSW_GLOBAL_MAX_QLEN || rlen > BSW_MAX_TLEN)
            return fail(e, BSW_E_LIMIT, "patch task %zu: beyond BSW_GLOBAL_MAX_QLEN / BSW_MAX_TLEN", i);
        const int band = gen_cigar_band(*pp, (int)lq, (int)rlen, w_);
        cells[i] = (uint64_t)std::min<int64_t>(lq, 2 * (int64_t)band + 1) * (uint64_t)rlen;
        seqb[i] = (uint64_t)(lq + rlen);
    }
    return BSW_OK;
}

/* The work target of a patch chunk, in banded cells (min(l_query, 2 w + 1) x (re - rb) under the task's band, summed), from the
 * sweep of tools/patch_rate.py ("sweep" of profiles/patch_rate.json), submit + wait of one ticket at 2^24 .. 2^30:
 * 65 536 pairs of 150 bases 3.9 / 3.4 / 3.2 / 3.3 / 3.5 / 3.4 / 3.5 ms (from 2^28 on the same four chunks: a submit is spread over
 * the slots first); 4 096 pairs of 2 000 bases 218 / 116 / 61 / 36 / 19 / 12 / 12 ms — a chunk of 2^28 cells holds only 512
 * such alignments, too few to fill the device, and the chunks of a ticket add up.  2^30 is where the long shape levels off and the
 * short one is unchanged; F4_CIGAR_CHUNK_WORK (2^28, where this started) loses 1.6 x at the long shape, beyond the runs' ranges.
 * BSW_F4_PATCH_WORK overrides it (tests, measurements). */
#define F4_PATCH_CHUNK_WORK (1ull << 30)
#define PATCH_BATCH_WORK (4ull << 30)                  /* a sub-batch of the synchronous call: as many cells as bsw_cigar_ref_batch's hold backtrack bytes */
static uint64_t patch_work_switch()                   /* BSW_F4_PATCH_WORK, 0: not set */
{
    static const uint64_t v = chunk_work_env("BSW_F4_PATCH_WORK", 0);
    return v;
}
static uint64_t patch_chunk_work() { return patch_work_switch() ? patch_work_switch() : F4_PATCH_CHUNK_WORK; }

extern "C" int bsw_patch_ref_batch(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_ptask *tasks, size_t n, bsw_presult *res)
{
    if (!ctx) return BSW_E_INVAL;
    errs &e = ctx->err;
    int rc = ref_entry_check(ctx, "bsw_patch_ref_batch", !p || !ref || (!tasks && n) || (!res && n), ref, false);
    if (rc) return rc;
    bsw_params pp;
    bsw_dparams dp;
    std::vector<uint64_t> cells, seqb;
    rc = patch_validate(e, p, ref, tasks, nullptr, nullptr, n, &pp, &dp, cells, seqb);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(ctx->device0()));
    f4_lane L = ctx_lane(ctx);
    /* sub-batches run one after the other, so they are large: the sequence arena's bound and PATCH_BATCH_WORK banded cells (no
     * backtrack term), or what BSW_F4_PATCH_WORK says */
    span_caps caps;
    caps.work = patch_work_switch() ? patch_work_switch() : PATCH_BATCH_WORK;
    const std::vector<chunk_span> spans = cut_spans(n, [&](size_t i) { return span_cost{0, seqb[i], 0, cells[i], 0, 0}; }, caps);
    for (const chunk_span &c : spans) {
        rc = patch_chunk(ctx, e, L, pp, dp, ref, tasks + c.base, c.cnt, res + c.base, nullptr, nullptr);
        if (rc) return rc;
    }
    return BSW_OK;
}

/* both ticket forms: tasks (pointer form) or rd + rtasks (resident reads) */
static int patch_submit(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_ptask *tasks, const bsw_reads *rd, const bsw_rd_ptask *rtasks,
                        size_t n, bsw_presult *res, bsw_ticket *ticket, const char *what)
{
    if (!ctx) return BSW_E_INVAL;
    if (ticket) *ticket = 0;
    int rc = ref_entry_check(ctx, what, !p || !ref || (!tasks && !rtasks && n) || (!res && n), ref, true);
    if (rc) return rc;
    errs e;                                          /* (several threads may submit at once: the context's text is set under its lock) */
    bsw_params pp;
    bsw_dparams dp;
    std::vector<uint64_t> cells, seqb;
    rc = patch_validate(e, p, ref, tasks, rd, rtasks, n, &pp, &dp, cells, seqb);
    if (rc) return ctx_fail(ctx, e, rc);
    f4_submit f;
    f.name = "patch"; f.rd = rd;
    f.run = [=](bsw_ctx *cx, errs &ce, f4_lane &L, chunk_span c) {
        return patch_chunk(cx, ce, L, pp, dp, ref, tasks ? tasks + c.base : nullptr, c.cnt, res + c.base, rd, rd ? rtasks + c.base : nullptr);
    };
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) total += cells[i];
    span_caps caps;
    caps.work = std::max<uint64_t>(f4_chunk_work(ctx, total, patch_chunk_work()), 1);
    f.spans = cut_spans(n, [&](size_t i) { return span_cost{0, seqb[i], 0, cells[i], 0, 0}; }, caps);
    return pipeline_submit_f4(ctx, std::move(f), ticket, what);
}

extern "C" int bsw_patch_ref_submit_t(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_ptask *tasks, size_t n, bsw_presult *res,
                                      bsw_ticket *ticket)
{
    return patch_submit(ctx, p, ref, tasks, nullptr, nullptr, n, res, ticket, "bsw_patch_ref_submit");
}

extern "C" int bsw_patch_reads_submit_t(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_reads *rd, const bsw_rd_ptask *tasks,
                                        size_t n, bsw_presult *res, bsw_ticket *ticket)
{
    return reads_submit(ctx, rd, ticket, "bsw_patch_reads_submit", [&] { return patch_submit(ctx, p, ref, nullptr, rd, tasks, n, res, ticket, "bsw_patch_reads_submit"); });
}
