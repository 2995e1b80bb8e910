/*
 * bsw_rescue_job.hip — mem_sam_pe's mate-rescue loop as one job around the rescue tickets (part of the host side of
 * libbwasw_mi355.so; no kernel here): bsw_rescue_ref_start / _reads_start open the engine (bsw_rescue.c), copy what it needs into
 * DMA-able memory and hand it to bsw_matesw_ref_submit_t / bsw_matesw_reads_submit_t; bsw_rescue_test and bsw_rescue_finish collect
 * a round's ticket, feed the engine and submit the next round until the engine needs nothing more.
 *
 * The job uses the context only through the ticket calls and the error channel, so it may be driven from several threads as
 * they may; one job belongs to one thread at a time.
 */
#include "bsw_internal.h"
#include "bsw_sdp_pass.h"

struct bsw_rescue_job {
    bsw_ctx *ctx = nullptr;
    bsw_params p{};
    const bsw_ref *ref = nullptr;
    const bsw_reads *rd = nullptr;    /* the reads form */
    const uint8_t *const *reads = nullptr;
    const int32_t *lens = nullptr;
    std::vector<int32_t> own_lens;    /* the reads form: the lengths of the block */
    bsw_rescue_eng *eng = nullptr;
    void *tasks = nullptr;            /* bsw_host_alloc: bsw_mtask[cap] or bsw_rd_mtask[cap] */
    bsw_mresult *results = nullptr;   /* bsw_host_alloc */
    size_t cap = 0, n = 0;            /* room of the two arrays; tasks of the round that is staged or in flight */
    bool starting = false;            /* inside the start call: no place among the submits refuses the job */
    bool staged = false;              /* tasks[0, n) wait for a place among the submits (BSW_E_BUSY) */
    bool done = false;                /* the engine needs nothing more */
    int failed = BSW_OK;
    bsw_ticket ticket = 0;            /* 0: no round in flight */
};

static void job_free(bsw_rescue_job *j, bool abandon)
{
    if (!abandon) {                                  /* (a dead context's device may still write the arrays: they stay) */
        if (j->tasks) bsw_host_free(j->tasks);
        if (j->results) bsw_host_free(j->results);
    }
    bsw_rescue_close(j->eng);
    delete j;
}

static int job_fail(bsw_rescue_job *j, int rc, const char *fmt, ...)
{
    if (fmt) {
        errs e;
        char buf[400];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof(buf), fmt, ap);
        va_end(ap);
        ctx_fail(j->ctx, e, fail(e, rc, "%s", buf));
    }
    j->failed = rc;
    return rc;
}

/* the engine's next needs into the pinned arrays: 1 staged, 0 nothing needed (done), < 0 failed */
static int stage_round(bsw_rescue_job *j, const char *who)
{
    const bsw_rd_mtask *t = nullptr;
    size_t n = 0;
    int rc = bsw_rescue_needs(j->eng, &t, &n);
    if (rc) return job_fail(j, rc, "%s: bsw_rescue_needs", who);
    if (!n) { j->done = true; return 0; }
    if (j->starting && bsw_inflight(j->ctx) >= BSW_MAX_INFLIGHT)
        return job_fail(j, BSW_E_BUSY, "%s: %d submits in flight already (BSW_MAX_INFLIGHT)", who, BSW_MAX_INFLIGHT);
    const size_t tsz = j->rd ? sizeof(bsw_rd_mtask) : sizeof(bsw_mtask);
    if (n > j->cap) {                                /* (no ticket is in flight here: nothing reads the old arrays) */
        if (j->tasks) bsw_host_free(j->tasks);
        if (j->results) bsw_host_free(j->results);
        j->cap = 0;
        j->tasks = bsw_host_alloc(n * tsz);
        j->results = (bsw_mresult *)bsw_host_alloc(n * sizeof(bsw_mresult));
        if (!j->tasks || !j->results) return job_fail(j, BSW_E_NOMEM, "%s: %zu bytes of DMA-able host memory", who, n * (tsz + sizeof(bsw_mresult)));
        j->cap = n;
    }
    if (j->rd)
        memcpy(j->tasks, t, n * sizeof(*t));
    else {
        bsw_mtask *o = (bsw_mtask *)j->tasks;
        for (size_t i = 0; i < n; ++i) {
            o[i].mate = j->reads[t[i].read]; o[i].l_ms = j->lens[t[i].read]; o[i].is_rev = t[i].is_rev; o[i].rb = t[i].rb; o[i].re = t[i].re;
            o[i].xtra = t[i].xtra; o[i].min_score = t[i].min_score;
        }
    }
    j->n = n; j->staged = true;
    return 1;
}

/* 1 submitted, BSW_E_BUSY no place (the round stays staged), another code: failed (the submit wrote the text) */
static int submit_round(bsw_rescue_job *j)
{
    const int rc = j->rd ? bsw_matesw_reads_submit_t(j->ctx, &j->p, j->ref, j->rd, (const bsw_rd_mtask *)j->tasks, j->n, j->results, &j->ticket)
                         : bsw_matesw_ref_submit_t(j->ctx, &j->p, j->ref, (const bsw_mtask *)j->tasks, j->n, j->results, &j->ticket);
    if (rc == BSW_E_BUSY) { j->ticket = 0; return rc; }
    if (rc) { j->ticket = 0; return job_fail(j, rc, nullptr); }
    j->staged = false;
    return 1;
}

/* Drives the rounds: 1 the engine has finished, 0 a round is in flight (wait == false only), BSW_E_BUSY a staged round found no
 * place, another code: the job has failed */
static int drive(bsw_rescue_job *j, bool wait, const char *who)
{
    for (;;) {
        if (j->failed) return j->failed;
        if (j->done) return 1;
        if (j->ticket) {
            if (!wait) {
                const int t = bsw_test(j->ctx, j->ticket);
                if (t == 0) return 0;
                if (t < 0) return job_fail(j, BSW_E_INVAL, "%s: the job's ticket was collected by another call (bsw_wait?)", who);
            }
            const int rc = bsw_wait_ticket(j->ctx, j->ticket);   /* (complete already when wait == false) */
            j->ticket = 0;
            if (rc) return job_fail(j, rc, nullptr);
            const int fr = bsw_rescue_feed(j->eng, j->results, j->n);
            if (fr) return job_fail(j, fr, "%s: bsw_rescue_feed", who);
            j->n = 0;
        }
        if (!j->staged) {
            const int s = stage_round(j, who);
            if (s <= 0) { if (s < 0) return s; continue; }
        }
        const int rc = submit_round(j);
        if (rc != 1) return rc;
    }
}

static int rescue_start(const char *who, bsw_ctx *ctx, const bsw_params *p, const bsw_rescue_opt *opt, const bsw_ref *ref, const bsw_reads *rd,
                        const uint8_t *const *reads, const int32_t *lens, size_t n_reads, const bsw_contig *contigs, size_t n_contigs,
                        const bsw_sreg *regs, size_t n_regs, const uint64_t *reg_start, bsw_rescue_job **job)
{
    if (!ctx) return BSW_E_INVAL;
    errs e;
    if (job) *job = nullptr;
    if (!job || !p || !ref || (!rd && (!reads || !lens) && n_reads)) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "%s: NULL argument", who));
    if (rd && rd->owner != ctx) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "%s: the read block was uploaded through another context", who));
    std::unique_ptr<bsw_rescue_job> j(new bsw_rescue_job());
    j->ctx = ctx; j->p = *p; j->ref = ref; j->rd = rd; j->reads = reads;
    if (rd) {
        j->own_lens.resize(rd->rd.size());
        for (size_t i = 0; i < rd->rd.size(); ++i) j->own_lens[i] = rd->rd[i].len;
        j->lens = j->own_lens.data(); n_reads = rd->rd.size();
    } else
        j->lens = lens;
    char text[400] = "";
    int rc = bsw_rescue_open(p, opt, ref->l_pac, contigs, n_contigs, regs, n_regs, reg_start, j->lens, n_reads, &j->eng, text, sizeof(text));
    if (rc) {
        job_free(j.release(), false);
        return ctx_fail(ctx, e, fail(e, rc, "%s: %s", who, text));
    }
    /* the first round: a start that the submit would refuse allocates no pinned arrays (stage_round; another thread may still take
     * the last place in between: the submit then answers, and everything is given back) */
    j->starting = true;
    rc = stage_round(j.get(), who);
    j->starting = false;
    if (rc == 1) rc = submit_round(j.get());
    if (rc < 0) {                                    /* BSW_E_BUSY included: nothing is queued (the texts are written) */
        job_free(j.release(), false);
        return rc;
    }
    *job = j.release();
    return BSW_OK;
}

extern "C" int bsw_rescue_ref_start(bsw_ctx *ctx, const bsw_params *p, const bsw_rescue_opt *opt, const bsw_ref *ref, const uint8_t *const *reads,
                                    const int32_t *lens, size_t n_reads, const bsw_contig *contigs, size_t n_contigs, const bsw_sreg *regs,
                                    size_t n_regs, const uint64_t *reg_start, bsw_rescue_job **job)
{
    return rescue_start("bsw_rescue_ref_start", ctx, p, opt, ref, nullptr, reads, lens, n_reads, contigs, n_contigs, regs, n_regs, reg_start, job);
}

extern "C" int bsw_rescue_reads_start(bsw_ctx *ctx, const bsw_params *p, const bsw_rescue_opt *opt, const bsw_ref *ref, const bsw_reads *rd,
                                      const bsw_contig *contigs, size_t n_contigs, const bsw_sreg *regs, size_t n_regs, const uint64_t *reg_start,
                                      bsw_rescue_job **job)
{
    if (ctx && !rd) {
        errs e;
        if (job) *job = nullptr;
        return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "bsw_rescue_reads_start: NULL argument"));
    }
    return rescue_start("bsw_rescue_reads_start", ctx, p, opt, ref, rd, nullptr, nullptr, 0, contigs, n_contigs, regs, n_regs, reg_start, job);
}

extern "C" int bsw_rescue_test(bsw_rescue_job *job)
{
    if (!job) return BSW_E_INVAL;
    const int rc = drive(job, false, "bsw_rescue_test");
    return rc == BSW_E_BUSY && !job->failed ? 0 : rc;
}

extern "C" int bsw_rescue_job_stats(const bsw_rescue_job *job, bsw_rescue_stats *stats)
{
    if (!job || !stats) return BSW_E_INVAL;
    return bsw_rescue_peek(job->eng, stats, nullptr);
}

extern "C" size_t bsw_rescue_job_out_capacity(const bsw_rescue_job *job)
{
    return job ? bsw_rescue_out_capacity(job->eng) : 0;
}

extern "C" int bsw_rescue_finish(bsw_rescue_job *job, bsw_sreg *out, size_t out_cap, size_t *n_out, uint64_t *out_start, int32_t *n_sw,
                                 bsw_rescue_stats *stats)
{
    if (!job) return BSW_E_INVAL;
    bsw_ctx *ctx = job->ctx;
    if (n_out) *n_out = 0;
    int rc = drive(job, true, "bsw_rescue_finish");
    if (rc == BSW_E_BUSY && !job->failed) return rc; /* the job stays: its next round is staged, a later call submits it */
    if (rc == 1) {
        size_t need = 0;
        errs e;
        bsw_rescue_peek(job->eng, nullptr, &need);
        if (need && (!out || out_cap < need))
            rc = ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "bsw_rescue_finish: out has room for %zu regions, the job ends with %zu", out ? out_cap : (size_t)0, need));
        else
            rc = bsw_rescue_collect(job->eng, out, n_out, out_start, n_sw, stats);
    }
    job_free(job, ctx->dead);
    return rc;
}
