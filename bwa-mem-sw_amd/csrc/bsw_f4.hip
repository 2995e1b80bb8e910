/* bsw_f4.hip — hosts of the two other Smith-Waterman users of bwa: bsw_global_batch / ksw_global2 / ksw_global and
 * bsw_align_batch / ksw_align2 / ksw_align, and the bodies of what they share with bsw_cigar.hip and bsw_matesw.hip (bsw_f4_host.h:
 * spans, class lists, routing, launch loops, staging, read-back, the sub-batch cutter).  Host-specific here: the device records
 * (bsw_gdtask with its slice of the backtrack matrix, bsw_adtask with its slice of the sub-optimal list scratch) and the checks of
 * the entry points.  (part of the host side of libbwasw_mi355.so) */
#include "bsw_f4_host.h"

/* ---- bsw_f4_host.h: the shared bodies ---- */
BSW_LOCAL bool global_force_long()
{
    static const bool on = [] { const char *v = getenv("BSW_GLOBAL_LONG"); return v && atoi(v) != 0; }();
    return on;
}

BSW_LOCAL int ref_entry_check(bsw_ctx *ctx, const char *what, bool bad_args, const bsw_ref *ref, bool ticket_form)
{
    errs local;
    errs &e = ticket_form ? local : ctx->err;
    int rc = BSW_OK;
    if (bad_args) rc = fail(e, BSW_E_INVAL, "%s: bad argument", what);
    else if (ref->d_pac.size() != ctx->devs.size() || !ref->d_pac[0]) rc = fail(e, BSW_E_INVAL, "%s: the reference was uploaded through another context", what);
    else if (!ticket_form) return busy_check(ctx, what);
    else if (ctx->dead) rc = fail(e, BSW_E_HIP, "%s: context is dead (an earlier wait for the GPU timed out)", what);
    return rc && ticket_form ? ctx_fail(ctx, e, rc) : rc;
}

BSW_LOCAL uint64_t chunk_work_env(const char *name, uint64_t dflt)
{
    const char *v = getenv(name);
    return v && atof(v) >= 1.0 ? (uint64_t)atof(v) : dflt;
}

BSW_LOCAL int launch_global_lists(errs &e, const class_lists &cl, const bsw_dparams &dp, const uint64_t *seq, const bsw_gdtask *tasks, const uint32_t *d_order,
                                  uint8_t *z, uint32_t *cigars, int max_cigar, bsw_gresult *out, hipStream_t s)
{
    for (int c = 0; c < cl.classes(); ++c)
        if (cl.count(c)) HIPCHK(e, bsw::launch_global(c, dp, seq, tasks, d_order + cl.begin(c), cl.count(c), z, cigars, max_cigar, out, s));
    return BSW_OK;
}

BSW_LOCAL int launch_align_lists(errs &e, const class_lists &cl, const align_long_ops *alo, const bsw_dparams &dp, const uint64_t *seq, const bsw_adtask *tasks,
                                 const uint32_t *d_order, unsigned long long *blist, bsw_kswr *out, hipStream_t s)
{
    const int ncls = bsw::align_class_count();
    for (int c = 0; c < cl.classes(); ++c) {
        if (!cl.count(c)) continue;
        if (c < ncls) HIPCHK(e, bsw::launch_align(c, dp, seq, tasks, d_order + cl.begin(c), cl.count(c), blist, out, s));
        else HIPCHK(e, alo->launch(c - ncls, dp, seq, tasks, d_order + cl.begin(c), cl.count(c), blist, out, s));
    }
    return BSW_OK;
}

BSW_LOCAL int upload_launch_global(errs &e, f4_lane &L, const class_lists &cl, const bsw_dparams &dp, const bsw_gdtask *gt, size_t n, size_t in_gt, size_t in_order,
                                   uint8_t *z, uint32_t *cigars, int max_cigar)
{
    const size_t gtb = n * sizeof(bsw_gdtask), orderb = cl.order.size() * sizeof(uint32_t);
    HIPCHK(e, hipMemcpyAsync(L.b->g_tasks.p, L.dma_src(gt, gtb, in_gt), gtb, hipMemcpyHostToDevice, L.s));
    HIPCHK(e, hipMemcpyAsync(L.b->g_order.p, L.dma_src(cl.order.data(), orderb, in_order), orderb, hipMemcpyHostToDevice, L.s));
    L.h2d += gtb + orderb;
    return launch_global_lists(e, cl, dp, L.st->d_seq.p, L.b->g_tasks.p, L.b->g_order.p, z, cigars, max_cigar, L.b->g_res.p, L.s);
}

BSW_LOCAL int stage_records(errs &e, stage_t &st, size_t n, bool desc)
{
    return reserve_all(e, "pinned staging", {{st.h_tasks, n + 1}, {st.h_roff, n + 1}, {st.h_desc, n + 1, desc}});
}

BSW_LOCAL int stage_upload(errs &e, f4_lane &L, const staged_raw &r, size_t n)
{
    stage_t &st = *L.st;
    if (r.bytes) HIPCHK(e, hipMemcpyAsync(st.d_raw.p + RAW_FRONT, r.src, r.bytes, hipMemcpyHostToDevice, L.s));
    HIPCHK(e, hipMemcpyAsync(st.d_tasks.p, st.h_tasks.p, n * sizeof(bsw_dtask), hipMemcpyHostToDevice, L.s));
    HIPCHK(e, hipMemcpyAsync(st.d_roff.p, st.h_roff.p, n * sizeof(bsw_rawoff), hipMemcpyHostToDevice, L.s));
    if (r.desc) HIPCHK(e, hipMemcpyAsync(st.d_desc.p, st.h_desc.p, n * sizeof(bsw_refx), hipMemcpyHostToDevice, L.s));
    L.h2d += r.bytes + n * (sizeof(bsw_dtask) + sizeof(bsw_rawoff) + (r.desc ? sizeof(bsw_refx) : 0));
    return BSW_OK;
}

BSW_LOCAL int stage_pack(errs &e, f4_lane &L, size_t n, int flags, const bsw_ref *ref, const bsw_reads *rd)
{
    stage_t &st = *L.st;
    if (rd) { const int orc = reads_order(e, rd, L.dev, L.s); if (orc) return orc; }       /* (an upload in flight: the stream waits for this device's copy) */
    HIPCHK(e, bsw::launch_pack(rd ? (const uint8_t *)rd->dev(L.dev) : st.d_raw.p + RAW_FRONT, st.d_tasks.p, st.d_roff.p, 0u, (uint32_t)n,
                               flags | (rd ? BSW_PACK_STORE : 0), ref ? ref->d_pac[L.dev] : nullptr, ref ? ref->l_pac : 0, ref ? st.d_desc.p : nullptr,
                               st.d_seq.p, nullptr, L.s));
    return BSW_OK;
}

BSW_LOCAL int lane_read_back(bsw_ctx *ctx, errs &e, f4_lane &L, std::initializer_list<back_copy> list)
{
    size_t off = 0;
    for (const back_copy &c : list) {
        if (L.h_back && c.bytes) HIPCHK(e, hipMemcpyAsync(L.h_back->p + off, c.src, c.bytes, hipMemcpyDeviceToHost, L.s));
        off += c.bytes;
    }
    const int rc = sync_stream(ctx, e, L.s, L.ev);
    if (rc) return rc;
    off = 0;
    for (const back_copy &c : list) {
        if (L.h_back) { if (c.bytes && c.dst) memcpy(c.dst, L.h_back->p + off, c.bytes); }
        else if (c.bytes) HIPCHK(e, hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost));
        off += c.bytes;
    }
    L.d2h += off;
    return BSW_OK;
}

/* ---- both hosts of this file: task i as a right-side-only seed of the query and target the caller holds, so that the byte-per-base
 * sequences travel and are packed exactly like extension tasks ---- */
static inline const bsw_dtask &stage_pair(stage_t &st, size_t i, uint64_t &acc, raw_span &sp, const uint8_t *query, int qlen, const uint8_t *target, int tlen)
{
    bsw_dtask &d = st.h_tasks.p[i];
    bsw_rawoff &r = st.h_roff.p[i];
    memset(&d, 0, sizeof(d));
    memset(&r, 0, sizeof(r));
    d.rq_off = (uint32_t)acc; acc += nwords(qlen);
    d.rt_off = (uint32_t)acc; acc += nwords(tlen);
    d.rqlen = (uint16_t)qlen; d.rtlen = (uint16_t)tlen;
    r.rq = (uint32_t)sp.bytes; sp.add(query, (size_t)qlen);
    r.rt = (uint32_t)sp.bytes; sp.add(target, (size_t)tlen);
    return d;
}
template <class T>
static inline raw_piece pair_piece(const T &t, int k)
{
    return k ? raw_piece{t.target, (size_t)t.tlen, &bsw_rawoff::rt, false} : raw_piece{t.query, (size_t)t.qlen, &bsw_rawoff::rq, false};
}

/* ---- banded global alignment with CIGAR (bwa ksw_global2) ------------------------------
 * Host side: give every alignment its slice of the backtrack matrix, sort by class (global_route), launch bsw_global_kernel /
 * bsw_global_long_kernel, bring scores and CIGARs back. */
static int global_chunk(bsw_ctx *ctx, errs &e, const bsw_dparams &dp, const bsw_gtask *tasks, size_t n, int max_cigar,
                        bsw_gresult *res, uint32_t *cigars)
{
    f4_lane L = ctx_lane(ctx);
    stage_t &st = *L.st;
    int rc = stage_records(e, st, n, false);
    if (rc) return rc;
    std::vector<bsw_gdtask> gt(n);
    std::vector<uint32_t> cls(n);
    class_lists cl;
    const global_route route;
    uint64_t acc = 0, zacc = 0;
    raw_span sp;
    for (size_t i = 0; i < n; ++i) {
        const bsw_gtask &t = tasks[i];
        const bsw_dtask &d = stage_pair(st, i, acc, sp, t.query, t.qlen, t.target, t.tlen);
        bsw_gdtask &g = gt[i];
        g.q_off = d.rq_off; g.t_off = d.rt_off; g.qlen = t.qlen; g.tlen = t.tlen; g.w = t.w; g.pad = 0; g.z_off = zacc;
        const int n_col = t.qlen < 2 * t.w + 1 ? t.qlen : 2 * t.w + 1;
        if (cigars) zacc += (uint64_t)n_col * (uint64_t)t.tlen;
        cls[i] = (uint32_t)route(t.qlen, n_col);
    }
    cl.build(route.classes(), cls.data(), nullptr, n);
    staged_raw raw;
    if ((rc = stage_raw(e, st, n, sp, acc, false, true, 2, [&](size_t i, int k) { return pair_piece(tasks[i], k); }, &raw)) != BSW_OK) return rc;
    if ((rc = reserve_all(e, "device staging", {{L.b->g_tasks, n + 1}, {L.b->g_order, n + 1}, {L.b->g_res, n + 1}, {L.b->g_z, (size_t)zacc + 64, cigars != nullptr},
                                                {L.b->g_cig, n * (size_t)max_cigar + 1, cigars != nullptr}})) != BSW_OK) return rc;
    drain_on_failure drain(ctx, L.s, L.ev);
    if ((rc = stage_upload(e, L, raw, n)) != BSW_OK) return rc;
    HIPCHK(e, hipMemcpyAsync(L.b->g_tasks.p, gt.data(), n * sizeof(bsw_gdtask), hipMemcpyHostToDevice, L.s));
    HIPCHK(e, hipMemcpyAsync(L.b->g_order.p, cl.order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, L.s));
    if ((rc = stage_pack(e, L, n, 0, nullptr, nullptr)) != BSW_OK) return rc;
    if ((rc = launch_global_lists(e, cl, dp, st.d_seq.p, L.b->g_tasks.p, L.b->g_order.p, cigars ? L.b->g_z.p : nullptr, cigars ? L.b->g_cig.p : nullptr, max_cigar,
                                  L.b->g_res.p, L.s)) != BSW_OK) return rc;
    const size_t cigb = cigars ? n * (size_t)max_cigar * sizeof(uint32_t) : 0;
    if ((rc = lane_read_back(ctx, e, L, {{res, L.b->g_res.p, n * sizeof(bsw_gresult)}, {cigars, L.b->g_cig.p, cigb}})) != BSW_OK) return rc;
    drain.done();
    return BSW_OK;
}

extern "C" int bsw_global_batch(bsw_ctx *ctx, const bsw_params *p, const bsw_gtask *tasks, size_t n, int max_cigar,
                                bsw_gresult *res, uint32_t *cigars)
{
    if (!ctx) return BSW_E_INVAL;
    errs &e = ctx->err;
    if (!p || (!tasks && n) || (!res && n) || (cigars && max_cigar < 1)) return fail(e, BSW_E_INVAL, "bsw_global_batch: bad argument");
    int rc = busy_check(ctx, "bsw_global_batch");
    if (rc) return rc;
    bsw_params pp = *p;
    pp.w = 0;                                         /* the band is per task here */
    bsw_dparams dp;
    rc = check_params(e, &pp, &dp);
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) {
        const bsw_gtask &t = tasks[i];
        if (t.qlen < 0 || t.tlen < 0 || t.w < 0) return fail(e, BSW_E_INVAL, "global task %zu: negative length or band", i);
        if (t.qlen > BSW_GLOBAL_MAX_QLEN || t.tlen > BSW_MAX_TLEN || t.w > BSW_MAX_TLEN) return fail(e, BSW_E_LIMIT, "global task %zu: beyond BSW_GLOBAL_MAX_QLEN/BSW_MAX_TLEN", i);
        if ((t.qlen && !t.query) || (t.tlen && !t.target)) return fail(e, BSW_E_INVAL, "global task %zu: NULL sequence pointer", i);
    }
    HIPCHK(e, hipSetDevice(ctx->device0()));
    /* sub-batches: bounded backtrack memory (1 byte per banded cell) and sequence arena; the largest single task
     * (8 191 x 65 535 bytes of z, 73 726 sequence bytes) fits both bounds on its own */
    const std::vector<chunk_span> spans = cut_spans(n, [&](size_t i) {
        const bsw_gtask &t = tasks[i];
        const uint64_t nz = (uint64_t)(t.qlen < 2 * t.w + 1 ? t.qlen : 2 * t.w + 1) * (uint64_t)t.tlen;
        return span_cost{cigars ? nz : 0, (uint64_t)(t.qlen + t.tlen), 0, 0, nz, 0};
    }, span_caps());
    for (const chunk_span &c : spans) {
        rc = global_chunk(ctx, e, dp, tasks + c.base, c.cnt, max_cigar, res + c.base, cigars ? cigars + c.base * (size_t)max_cigar : nullptr);
        if (rc) return rc;
    }
    return BSW_OK;
}

/* drop-in scalar ABI through the process-wide context: calls from concurrent threads share device round trips exactly
 * as ksw_extend2's do (one bsw_global_batch per trip and scoring).  Failure contract as ksw_extend2: message on stderr,
 * *n_cigar = 0, return -1. */
extern "C" int ksw_global2(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat,
                           int o_del, int e_del, int o_ins, int e_ins, int w, int *n_cigar_, uint32_t **cigar_)
{
    if (n_cigar_) *n_cigar_ = 0;
    if (cigar_) *cigar_ = nullptr;
    if (m != 5 || !mat || qlen < 0 || tlen < 0 || (qlen > 0 && !query) || (tlen > 0 && !target)) {
        fprintf(stderr, "ksw_global2(libbwasw_mi355): unsupported arguments (m must be 5)\n");
        return -1;
    }
    scalar_req req;
    req.kind = 2;
    bsw_default_params(&req.p);
    memcpy(req.p.mat, mat, 25);
    req.p.o_del = o_del; req.p.e_del = e_del; req.p.o_ins = o_ins; req.p.e_ins = e_ins;
    memset(&req.gt, 0, sizeof(req.gt));
    req.gt.query = query; req.gt.target = target; req.gt.qlen = qlen; req.gt.tlen = tlen; req.gt.w = w < 0 ? 0 : w;
    const bool want = n_cigar_ && cigar_;
    req.cap = want ? qlen + tlen + 2 : 0;
    scalar_call(req);                                  /* coalesced with whatever other threads have queued */
    int score = -1;
    if (!req.rc) {
        score = req.gr.score;
        if (want && req.gr.n_cigar > 0) {
            *cigar_ = (uint32_t *)malloc((size_t)req.gr.n_cigar * sizeof(uint32_t));
            if (*cigar_) { memcpy(*cigar_, req.cg.data(), (size_t)req.gr.n_cigar * sizeof(uint32_t)); *n_cigar_ = req.gr.n_cigar; }
        }
    }
    return score;
}

extern "C" int ksw_global(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat,
                          int gapo, int gape, int w, int *n_cigar_, uint32_t **cigar_)
{
    return ksw_global2(qlen, query, tlen, target, m, mat, gapo, gape, gapo, gape, w, n_cigar_, cigar_);
}

/* ---- local alignment with start / second-best search (bwa ksw_align2, mate rescue) -----------
 * Host side as for the global alignment; every alignment gets its slice of the sub-optimal list scratch, tasks are sorted by
 * kernel class (align_route), bsw_align_kernel runs per class.
 * Under bsw_set_align_long a query of more than BSW_ALIGN_MAX_QLEN bases (mode 2: every query) is sorted into the classes of
 * bsw_align_long_kernel, which follow the ten of bsw_align_kernel in g_order; the route is the call's snapshot al_mode, and a chunk
 * without such a task makes the HIP calls it made before the route existed. */
static std::atomic<const align_long_ops *> g_align_long_ops{nullptr};
BSW_LOCAL void align_long_register(const align_long_ops *ops) { g_align_long_ops.store(ops, std::memory_order_release); }
BSW_LOCAL const align_long_ops *align_long_registered() { return g_align_long_ops.load(std::memory_order_acquire); }

static int align_chunk(bsw_ctx *ctx, errs &e, const bsw_dparams &dp, const bsw_atask *tasks, size_t n, bsw_kswr *out, int al_mode)
{
    f4_lane L = ctx_lane(ctx);
    stage_t &st = *L.st;
    int rc = stage_records(e, st, n, false);
    if (rc) return rc;
    std::vector<bsw_adtask> at(n);
    const int ncls = bsw::align_class_count();
    const align_long_ops *alo = al_mode ? align_long_registered() : nullptr;
    const int nall = ncls + (alo ? alo->class_count() : 0);
    std::vector<uint32_t> cls(n);
    class_lists cl;
    uint64_t acc = 0, bacc = 0;
    raw_span sp;
    for (size_t i = 0; i < n; ++i) {
        const bsw_atask &t = tasks[i];
        const bsw_dtask &d = stage_pair(st, i, acc, sp, t.query, t.qlen, t.target, t.tlen);
        bsw_adtask &a = at[i];
        a.q_off = d.rq_off; a.t_off = d.rt_off; a.qlen = t.qlen; a.tlen = t.tlen; a.xtra = t.xtra; a.pad = 0; a.b_off = bacc;
        if (t.xtra & KSW_XSUBO) bacc += (uint64_t)t.tlen;
        const int c = align_route(al_mode, t.qlen, (t.xtra & KSW_XBYTE) != 0, ncls, nall);
        if (c < 0) return fail(e, BSW_E_LIMIT, "align task %zu: no kernel class takes %d query bases", i, t.qlen);
        cls[i] = (uint32_t)c;
    }
    cl.build(nall, cls.data(), nullptr, n);
    staged_raw raw;
    if ((rc = stage_raw(e, st, n, sp, acc, false, true, 2, [&](size_t i, int k) { return pair_piece(tasks[i], k); }, &raw)) != BSW_OK) return rc;
    if ((rc = reserve_all(e, "device staging", {{L.b->a_tasks, n + 1}, {L.b->g_order, n + 1}, {L.b->a_res, n + 1}, {L.b->a_bl, (size_t)bacc + 64}})) != BSW_OK) return rc;
    drain_on_failure drain(ctx, L.s, L.ev);
    if ((rc = stage_upload(e, L, raw, n)) != BSW_OK) return rc;
    HIPCHK(e, hipMemcpyAsync(L.b->a_tasks.p, at.data(), n * sizeof(bsw_adtask), hipMemcpyHostToDevice, L.s));
    HIPCHK(e, hipMemcpyAsync(L.b->g_order.p, cl.order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, L.s));
    if ((rc = stage_pack(e, L, n, 0, nullptr, nullptr)) != BSW_OK) return rc;
    if ((rc = launch_align_lists(e, cl, alo, dp, st.d_seq.p, L.b->a_tasks.p, L.b->g_order.p, L.b->a_bl.p, L.b->a_res.p, L.s)) != BSW_OK) return rc;
    if ((rc = lane_read_back(ctx, e, L, {{out, L.b->a_res.p, n * sizeof(bsw_kswr)}})) != BSW_OK) return rc;
    drain.done();
    return BSW_OK;
}

extern "C" int bsw_align_batch(bsw_ctx *ctx, const bsw_params *p, const bsw_atask *tasks, size_t n, bsw_kswr *out)
{
    return align_batch_mode(ctx, p, tasks, n, out, align_long_snapshot());     /* the switch as this call finds it */
}

BSW_LOCAL int align_batch_mode(bsw_ctx *ctx, const bsw_params *p, const bsw_atask *tasks, size_t n, bsw_kswr *out, int al_mode)
{
    if (!ctx) return BSW_E_INVAL;
    if (!align_long_registered()) al_mode = 0;
    const int qmax = al_mode ? BSW_ALIGN_LONG_MAX_QLEN : BSW_ALIGN_MAX_QLEN;
    errs &e = ctx->err;
    if (!p || (!tasks && n) || (!out && n)) return fail(e, BSW_E_INVAL, "bsw_align_batch: NULL argument");
    int rc = busy_check(ctx, "bsw_align_batch");
    if (rc) return rc;
    bsw_params pp = *p;
    pp.w = 0; pp.variant = BSW_VARIANT_H;
    bsw_dparams dp;
    rc = check_params(e, &pp, &dp);
    if (rc) return rc;
    int mxs = 0;
    for (int i = 0; i < 25; ++i) mxs = std::max(mxs, (int)p->mat[i]);
    if (mxs <= 0) return fail(e, BSW_E_INVAL, "bsw_align_batch: the scoring matrix has no positive score");
    for (size_t i = 0; i < n; ++i) {
        const bsw_atask &t = tasks[i];
        if (t.qlen < 0 || t.tlen < 0) return fail(e, BSW_E_INVAL, "align task %zu: negative length", i);
        if (t.qlen > qmax || t.tlen > BSW_MAX_TLEN)
            return fail(e, BSW_E_LIMIT, "align task %zu: beyond %s/BSW_MAX_TLEN", i, al_mode ? "BSW_ALIGN_LONG_MAX_QLEN" : "BSW_ALIGN_MAX_QLEN");
        if ((t.qlen && !t.query) || (t.tlen && !t.target)) return fail(e, BSW_E_INVAL, "align task %zu: NULL sequence pointer", i);
        if (t.xtra & ~(0xffff | KSW_XBYTE | KSW_XSTOP | KSW_XSUBO | KSW_XSTART)) return fail(e, BSW_E_INVAL, "align task %zu: unknown xtra flag", i);
        if ((rc = align_byte_mode_check(e, p, t.xtra, "align", i)) != BSW_OK) return rc;
    }
    HIPCHK(e, hipSetDevice(ctx->device0()));
    /* sub-batches: bounded sequence arena and sub-optimal list scratch */
    const std::vector<chunk_span> spans = cut_spans(n, [&](size_t i) {
        const bsw_atask &t = tasks[i];
        return span_cost{0, (uint64_t)(t.qlen + t.tlen), (t.xtra & KSW_XSUBO) ? (uint64_t)t.tlen : 0, 0, 0, (uint64_t)t.tlen};
    }, span_caps());
    for (const chunk_span &c : spans) {
        rc = align_chunk(ctx, e, dp, tasks + c.base, c.cnt, out + c.base, al_mode);
        if (rc) return rc;
    }
    return BSW_OK;
}

static kswr_t align_scalar(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat,
                           int o_del, int e_del, int o_ins, int e_ins, int xtra)
{
    kswr_t r = {0, -1, -1, -1, -1, -1, -1};
    if (m != 5 || !mat || (qlen > 0 && !query) || (tlen > 0 && !target) || qlen < 0 || tlen < 0) {
        fprintf(stderr, "ksw_align2(libbwasw_mi355): unsupported arguments (m must be 5)\n");
        r.score = -1;
        return r;
    }
    scalar_req req;
    req.kind = 1;
    bsw_default_params(&req.p);
    memcpy(req.p.mat, mat, 25);
    req.p.o_del = o_del; req.p.e_del = e_del; req.p.o_ins = o_ins; req.p.e_ins = e_ins;
    memset(&req.at, 0, sizeof(req.at));
    req.at.query = query; req.at.target = target; req.at.qlen = qlen; req.at.tlen = tlen; req.at.xtra = xtra;
    req.al_mode = align_long_snapshot();               /* in the caller's thread: the trip's leader may be another one */
    scalar_call(req);                                  /* coalesced with whatever other threads have queued */
    r.score = -1;
    if (!req.rc) { r.score = req.ar.score; r.te = req.ar.te; r.qe = req.ar.qe; r.score2 = req.ar.score2; r.te2 = req.ar.te2; r.tb = req.ar.tb; r.qb = req.ar.qb; }
    return r;
}

extern "C" kswr_t ksw_align2(int qlen, uint8_t *query, int tlen, uint8_t *target, int m, const int8_t *mat,
                             int o_del, int e_del, int o_ins, int e_ins, int xtra, void **qry)
{
    (void)qry;
    return align_scalar(qlen, query, tlen, target, m, mat, o_del, e_del, o_ins, e_ins, xtra);
}

extern "C" kswr_t ksw_align(int qlen, uint8_t *query, int tlen, uint8_t *target, int m, const int8_t *mat,
                            int gapo, int gape, int xtra, void **qry)
{
    (void)qry;
    return align_scalar(qlen, query, tlen, target, m, mat, gapo, gape, gapo, gape, xtra);
}

