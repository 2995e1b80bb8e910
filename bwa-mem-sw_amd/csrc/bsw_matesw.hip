/* bsw_matesw.hip — host of bsw_matesw_ref_batch: mem_matesw's ksw_align2 (bwamem_pair.c) against the device-resident
 * reference (part of the host side of libbwasw_mi355.so).  Spans, class lists, routing, staging, read-back and the sub-batch
 * cutter are bsw_f4_host.h's; host-specific here, per chunk of tasks:
 *   1. how a task is laid out for bsw_pack_kernel: the mate as the caller holds it, in read order, neither reversed nor
 *      complemented; every task is a right-side-only seed, the mate read forwards and the target fetched upwards from rb, which is
 *      bns_get_seq on both strands;
 *   2. bsw_align_kernel (bsw_align_batch's classes) runs once per class; a task with is_rev carries BSW_AD_QRC and the kernel
 *      builds its query profile from the reverse complement of the stored mate, in the main pass and in the KSW_XSTART pass, so
 *      one launch per class serves both orientations;
 *   3. mem_matesw's mapping of kswr_t to the region and its keep decision run here on the copied-back results.
 * A chunk runs on a LANE (f4_lane, bsw_internal.h): the context's own for bsw_matesw_ref_batch, a pipeline slot's for the chunks
 * of bsw_matesw_ref_submit_t (bsw_batch.hip: process_f4). */
#include "bsw_f4_host.h"

/* the pack kernel reads a word of a sequence as 20 bytes from the dword below its first byte: forwards up to 16 + 3 bytes past
 * a mate's end */
static_assert(RAW_FRONT >= 4 && RAW_SLACK >= 20, "raw slack of the mates");

/* bwa: nothing is aligned for an empty mate, an empty window, or one bns_get_seq cannot return whole */
static bool mtask_runs(const bsw_mtask &t, int64_t l_pac)
{
    return t.l_ms > 0 && t.rb < t.re && !(t.rb < l_pac && t.re > l_pac) && t.rb >= 0 && t.re <= 2 * l_pac;
}

/* task i of a chunk in the pointer form's terms: the caller's record, or the one a resident-read task stands for (mate stays
 * NULL: the bases are on the device already) */
static inline bsw_mtask mtask_of(const bsw_mtask *tasks, const bsw_reads *rd, const bsw_rd_mtask *rtasks, size_t i)
{
    if (!rd) return tasks[i];
    const bsw_rd_mtask &r = rtasks[i];
    bsw_mtask t;
    t.mate = nullptr; t.l_ms = rd->rd[r.read].len; t.is_rev = r.is_rev; t.rb = r.rb; t.re = r.re; t.xtra = r.xtra; t.min_score = r.min_score;
    return t;
}

/* rd != NULL: the chunk's tasks are rtasks[0..n) and name mates of the resident block (tasks is NULL then) */
static int matesw_chunk(bsw_ctx *ctx, errs &e, f4_lane &L, const bsw_dparams &dp, const bsw_ref *ref, const bsw_mtask *tasks, size_t n,
                        bsw_mresult *res, const bsw_reads *rd, const bsw_rd_mtask *rtasks, int al_mode)
{
    stage_t &st = *L.st;
    hipStream_t s = L.s;
    const int64_t l_pac = ref->l_pac;
    int rc = stage_records(e, st, n, true);
    if (rc) return rc;
    std::vector<bsw_adtask> at(n);
    std::vector<uint8_t> runs(n);
    const int ncls = bsw::align_class_count();
    const align_long_ops *alo = al_mode ? align_long_registered() : nullptr;       /* (al_mode: the call's or the submit's snapshot) */
    const int nall = ncls + (alo ? alo->class_count() : 0);
    std::vector<uint32_t> cls, ids;                  /* of the tasks that run */
    class_lists cl;
    uint64_t acc = 0, bacc = 0;
    raw_span sp;
    for (size_t i = 0; i < n; ++i) {
        const bsw_mtask t = mtask_of(tasks, rd, rtasks, i);
        runs[i] = mtask_runs(t, l_pac) ? 1 : 0;
        if (!runs[i]) {
            clear_records(st, i);
            continue;
        }
        const int tlen = (int)(t.re - t.rb);
        /* the forward layout on both strands; the mate starts at its first base in the store, or at the next byte of the raw bytes */
        const interval_words iw = lay_interval(st, i, t.l_ms, tlen, false, rd ? rd->pos(rtasks[i].read) : (uint32_t)sp.bytes, t.rb, t.re, acc);
        if (!rd) sp.add(t.mate, (size_t)t.l_ms);
        bsw_adtask &a = at[i];
        a.q_off = iw.qw; a.t_off = iw.tw; a.qlen = t.l_ms; a.tlen = tlen; a.xtra = t.xtra;
        a.pad = t.is_rev ? BSW_AD_QRC : 0u;
        a.b_off = bacc;
        if (t.xtra & KSW_XSUBO) bacc += (uint64_t)tlen;
        const int c = align_route(al_mode, t.l_ms, (t.xtra & KSW_XBYTE) != 0, ncls, nall);
        if (c < 0) return fail(e, BSW_E_LIMIT, "mate task %zu: no kernel class takes %d bases", i, t.l_ms);
        cls.push_back((uint32_t)c);
        ids.push_back((uint32_t)i);
    }
    cl.build(nall, cls.data(), ids.data(), ids.size());
    staged_raw raw;
    rc = stage_raw(e, st, n, sp, acc, true, false, 1, [&](size_t i, int) {
        return raw_piece{runs[i] ? tasks[i].mate : nullptr, runs[i] ? (size_t)tasks[i].l_ms : 0, &bsw_rawoff::rq, false};
    }, &raw);
    if (rc) return rc;
    if ((rc = reserve_all(e, "device staging", {{L.b->a_tasks, n + 1}, {L.b->g_order, n + 1}, {L.b->a_res, n + 1}, {L.b->a_bl, (size_t)bacc + 64}})) != BSW_OK) return rc;
    const size_t in_order = (n + 1) * sizeof(bsw_adtask);
    if (L.h_back && (rc = reserve_all(e, "pinned staging", {{*L.h_back, n * sizeof(bsw_kswr) + 16}, {*L.h_in, in_order + (n + 1) * sizeof(uint32_t)}})) != BSW_OK) return rc;
    std::vector<bsw_kswr> aln(L.h_back ? 0 : n);
    const bsw_kswr *alnp = L.h_back ? (const bsw_kswr *)L.h_back->p : aln.data();      /* a slot reads back into pinned memory */
    drain_on_failure drain(ctx, s, L.ev);
    if (!cl.order.empty()) {
        if ((rc = stage_upload(e, L, raw, n)) != BSW_OK) return rc;
        HIPCHK(e, hipMemcpyAsync(L.b->a_tasks.p, L.dma_src(at.data(), n * sizeof(bsw_adtask), 0), n * sizeof(bsw_adtask), hipMemcpyHostToDevice, s));
        HIPCHK(e, hipMemcpyAsync(L.b->g_order.p, L.dma_src(cl.order.data(), cl.order.size() * sizeof(uint32_t), in_order), cl.order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        L.h2d += n * sizeof(bsw_adtask) + cl.order.size() * sizeof(uint32_t);
        if ((rc = stage_pack(e, L, n, 0, ref, rd)) != BSW_OK) return rc;
        if ((rc = launch_align_lists(e, cl, alo, dp, st.d_seq.p, L.b->a_tasks.p, L.b->g_order.p, L.b->a_bl.p, L.b->a_res.p, s)) != BSW_OK) return rc;
        if ((rc = lane_read_back(ctx, e, L, {{L.h_back ? nullptr : aln.data(), L.b->a_res.p, n * sizeof(bsw_kswr)}})) != BSW_OK) return rc;
    }
    /* mem_matesw: if (aln.score >= opt->min_seed_len && aln.qb >= 0) { b.qb = is_rev? l_ms - (aln.qe + 1) : aln.qb; ... } */
    for (size_t i = 0; i < n; ++i) {
        const bsw_mtask t = mtask_of(tasks, rd, rtasks, i);
        bsw_mresult &m = res[i];
        memset(&m, 0, sizeof(m));
        if (!runs[i]) {
            m.aln = bsw_kswr{0, -1, -1, -1, -1, -1, -1};
            m.status = 1;
            continue;
        }
        const bsw_kswr &a = alnp[i];
        m.aln = a;
        if (!(a.score >= t.min_score && a.qb >= 0)) {
            m.status = 2;
            continue;
        }
        const bool rev = t.is_rev != 0;
        m.qb = rev ? t.l_ms - (a.qe + 1) : a.qb;
        m.qe = rev ? t.l_ms - a.qb : a.qe + 1;
        m.rb = rev ? (l_pac << 1) - (t.rb + a.te + 1) : t.rb + a.tb;
        m.re = rev ? (l_pac << 1) - (t.rb + a.tb) : t.rb + a.te + 1;
        m.score = a.score;
        m.csub = a.score2;
        const int64_t rl = m.re - m.rb, ql = m.qe - m.qb;
        m.seedcov = (int32_t)((rl < ql ? rl : ql) >> 1);
    }
    drain.done();
    return BSW_OK;
}

/* what one task adds to a sub-batch: sequence bytes, a list slice under KSW_XSUBO (the bound is probed with the window either
 * way), l_ms x (re - rb) cells of work */
static span_cost mtask_cost(const bsw_mtask &t)
{
    const uint64_t tl = t.re > t.rb ? (uint64_t)(t.re - t.rb) : 0;
    return span_cost{0, (uint64_t)t.l_ms + tl, (t.xtra & KSW_XSUBO) ? tl : 0, (uint64_t)t.l_ms * tl, 0, tl};
}

/* what both entry points check before anything runs or is queued: the parameters (band and variant are the call's own), then
 * the tasks in order — the first malformed one rejects the call */
static int matesw_validate(errs &e, const bsw_params *p, const bsw_mtask *tasks, size_t n, const char *what, bsw_dparams *dp, int al_mode,
                           const bsw_reads *rd = nullptr, const bsw_rd_mtask *rtasks = nullptr)
{
    const int qmax = al_mode ? BSW_ALIGN_LONG_MAX_QLEN : BSW_ALIGN_MAX_QLEN;
    bsw_params pp = *p;
    pp.w = 0; pp.variant = BSW_VARIANT_H;
    int rc = check_params(e, &pp, dp);
    if (rc) return rc;
    int mxs = 0;
    for (int i = 0; i < 25; ++i) mxs = std::max(mxs, (int)p->mat[i]);
    if (mxs <= 0) return fail(e, BSW_E_INVAL, "%s: the scoring matrix has no positive score", what);
    for (size_t i = 0; i < n; ++i) {
        if (rd && rtasks[i].read >= rd->rd.size()) return fail(e, BSW_E_INVAL, "mate task %zu: read %u is not in the block of %zu reads", i, rtasks[i].read, rd->rd.size());
        const bsw_mtask t = mtask_of(tasks, rd, rtasks, i);
        if (t.l_ms < 0) return fail(e, BSW_E_INVAL, "mate task %zu: negative length", i);
        if (t.l_ms && !t.mate && !rd) return fail(e, BSW_E_INVAL, "mate task %zu: NULL mate", i);
        if (t.is_rev != 0 && t.is_rev != 1) return fail(e, BSW_E_INVAL, "mate task %zu: is_rev is neither 0 nor 1", i);
        if (t.xtra & ~(0xffff | KSW_XBYTE | KSW_XSTOP | KSW_XSUBO | KSW_XSTART)) return fail(e, BSW_E_INVAL, "mate task %zu: unknown xtra flag", i);
        if ((rc = align_byte_mode_check(e, p, t.xtra, "mate", i)) != BSW_OK) return rc;
        if (t.l_ms > qmax || (t.re > t.rb && t.re - t.rb > BSW_MAX_TLEN))
            return fail(e, BSW_E_LIMIT, "mate task %zu: beyond %s / BSW_MAX_TLEN", i, al_mode ? "BSW_ALIGN_LONG_MAX_QLEN" : "BSW_ALIGN_MAX_QLEN");
    }
    return BSW_OK;
}

extern "C" int bsw_matesw_ref_batch(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_mtask *tasks, size_t n,
                                    bsw_mresult *res)
{
    if (!ctx) return BSW_E_INVAL;
    errs &e = ctx->err;
    int rc = ref_entry_check(ctx, "bsw_matesw_ref_batch", !p || !ref || (!tasks && n) || (!res && n), ref, false);
    if (rc) return rc;
    bsw_dparams dp;
    const int al_mode = align_long_snapshot();        /* the switch as this call finds it */
    rc = matesw_validate(e, p, tasks, n, "bsw_matesw_ref_batch", &dp, al_mode);
    if (rc) return rc;
    HIPCHK(e, hipSetDevice(ctx->device0()));
    f4_lane L = ctx_lane(ctx);
    /* sub-batches: bsw_align_batch's bounds on the sequence arena and b[] scratch */
    const std::vector<chunk_span> spans = cut_spans(n, [&](size_t i) { return mtask_cost(tasks[i]); }, span_caps());
    for (const chunk_span &c : spans) {
        rc = matesw_chunk(ctx, e, L, dp, ref, tasks + c.base, c.cnt, res + c.base, nullptr, nullptr, al_mode);
        if (rc) return rc;
    }
    return BSW_OK;
}

/* The work target of a rescue chunk, in cells (l_ms x (re - rb) summed over its tasks), from the sweep of tools/f4_stream_rate.py
 * ("sweep_matesw" of profiles/f4_stream_rate.json): 262 144 windows of 150 x 550 take 176 / 77 / 66 / 82 / 50.5 /
 * 47.6 / 51.5 ms at 2^27 .. 2^33; 2^31 is the smallest target of the plateau (~26 k windows a chunk), which leaves the most chunks
 * for slots and devices.  BSW_F4_MATESW_WORK overrides it (tests, measurements). */
#define F4_MATESW_CHUNK_WORK (1ull << 31)
static uint64_t matesw_chunk_work()
{
    static const uint64_t v = chunk_work_env("BSW_F4_MATESW_WORK", F4_MATESW_CHUNK_WORK);
    return v;
}

/* bsw_matesw_ref_batch as a ticket of the context's pipeline: the same checks in the caller's thread, then chunks of about
 * matesw_chunk_work() cells (and within the batch call's bounds) through the slots of every device, chunk k on device
 * k mod n_devices against that device's copy of the reference.  Collected by bsw_wait_ticket / bsw_wait. */
/* both ticket forms: tasks (pointer form) or rd + rtasks (resident reads) */
static int matesw_submit(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_mtask *tasks, const bsw_reads *rd,
                         const bsw_rd_mtask *rtasks, size_t n, bsw_mresult *res, bsw_ticket *ticket, const char *what)
{
    if (!ctx) return BSW_E_INVAL;
    if (ticket) *ticket = 0;
    int rc = ref_entry_check(ctx, what, !p || !ref || (!tasks && !rtasks && n) || (!res && n), ref, true);
    if (rc) return rc;
    errs e;                                          /* (several threads may submit at once: the context's text is set under its lock) */
    bsw_dparams dp;
    const int al_mode = align_long_snapshot();        /* in the submitting thread; the chunks run later on slot threads and route by this, never by the switch */
    rc = matesw_validate(e, p, tasks, n, what, &dp, al_mode, rd, rtasks);
    if (rc) return ctx_fail(ctx, e, rc);
    f4_submit f;
    f.name = "matesw"; f.rd = rd;
    f.run = [=](bsw_ctx *cx, errs &ce, f4_lane &L, chunk_span c) {
        return matesw_chunk(cx, ce, L, dp, ref, tasks ? tasks + c.base : nullptr, c.cnt, res + c.base, rd, rd ? rtasks + c.base : nullptr, al_mode);
    };
    uint64_t total = 0;
    for (size_t i = 0; i < n; ++i) total += mtask_cost(mtask_of(tasks, rd, rtasks, i)).work;
    span_caps caps;                                   /* the batch call's bounds, and the work of a chunk */
    caps.work = f4_chunk_work(ctx, total, matesw_chunk_work());
    f.spans = cut_spans(n, [&](size_t i) { return mtask_cost(mtask_of(tasks, rd, rtasks, i)); }, caps);
    return pipeline_submit_f4(ctx, std::move(f), ticket, what);
}

extern "C" int bsw_matesw_ref_submit_t(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_mtask *tasks, size_t n,
                                       bsw_mresult *res, bsw_ticket *ticket)
{
    return matesw_submit(ctx, p, ref, tasks, nullptr, nullptr, n, res, ticket, "bsw_matesw_ref_submit");
}

/* the same against a resident read block: a task names its mate by index, and only the 32-byte task records' worth of
 * coordinates cross PCIe (the device records built from them: 76 + 32 + 4 bytes a task) */
extern "C" int bsw_matesw_reads_submit_t(bsw_ctx *ctx, const bsw_params *p, const bsw_ref *ref, const bsw_reads *rd, const bsw_rd_mtask *tasks,
                                         size_t n, bsw_mresult *res, bsw_ticket *ticket)
{
    return reads_submit(ctx, rd, ticket, "bsw_matesw_reads_submit", [&] { return matesw_submit(ctx, p, ref, nullptr, rd, tasks, n, res, ticket, "bsw_matesw_reads_submit"); });
}
