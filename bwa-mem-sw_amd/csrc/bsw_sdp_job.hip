/*
 * bsw_sdp_job.hip — mem_sort_dedup_patch as one job around the patch tickets (part of the host side of libbwasw_mi355.so; no
 * kernel here): bsw_sdp_ref_start / _reads_start open the engine (bsw_sdp.c), copy what it needs into DMA-able memory and hand it
 * to bsw_patch_ref_submit_t / bsw_patch_reads_submit_t; bsw_sdp_test and bsw_sdp_finish collect a round's ticket, feed the engine
 * and submit the next round until the engine needs nothing more.
 *
 * The job uses the context only through the ticket calls and the error channel, so it may be driven from several threads as
 * they may; one job belongs to one thread at a time.
 */
#include "bsw_internal.h"

struct bsw_sdp_job {
    bsw_ctx *ctx = nullptr;
    bsw_params p{};
    const bsw_ref *ref = nullptr;
    const bsw_reads *rd = nullptr;    /* the reads form */
    const uint8_t *const *reads = nullptr;
    const int32_t *lens = nullptr;
    std::vector<int32_t> own_lens;    /* the reads form: the lengths of the block */
    bsw_sdp_eng *eng = nullptr;
    void *tasks = nullptr;            /* bsw_host_alloc: bsw_ptask[cap] or bsw_rd_ptask[cap] */
    bsw_presult *results = nullptr;   /* bsw_host_alloc */
    size_t cap = 0, n = 0;            /* room of the two arrays; tasks of the round that is staged or in flight */
    bool starting = false;            /* inside the start call: no place among the submits refuses the job */
    bool staged = false;              /* tasks[0, n) wait for a place among the submits (BSW_E_BUSY) */
    bool done = false;                /* the engine needs nothing more */
    int failed = BSW_OK;
    bsw_ticket ticket = 0;            /* 0: no round in flight */
};

static void job_free(bsw_sdp_job *j, bool abandon)
{
    if (!abandon) {                                  /* (a dead context's device may still write the arrays: they stay) */
        if (j->tasks) bsw_host_free(j->tasks);
        if (j->results) bsw_host_free(j->results);
    }
    bsw_sdp_close(j->eng);
    delete j;
}

static int job_fail(bsw_sdp_job *j, int rc, const char *fmt, ...)
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
static int stage_round(bsw_sdp_job *j, const char *who)
{
    const bsw_rd_ptask *t = nullptr;
    size_t n = 0;
    int rc = bsw_sdp_needs(j->eng, &t, &n);
    if (rc) return job_fail(j, rc, "%s: bsw_sdp_needs: out of memory", who);
    if (!n) { j->done = true; return 0; }
    if (j->starting && bsw_inflight(j->ctx) >= BSW_MAX_INFLIGHT)
        return job_fail(j, BSW_E_BUSY, "%s: %d submits in flight already (BSW_MAX_INFLIGHT)", who, BSW_MAX_INFLIGHT);
    const size_t tsz = j->rd ? sizeof(bsw_rd_ptask) : sizeof(bsw_ptask);
    if (n > j->cap) {                                /* (no ticket is in flight here: nothing reads the old arrays) */
        if (j->tasks) bsw_host_free(j->tasks);
        if (j->results) bsw_host_free(j->results);
        j->cap = 0;
        j->tasks = bsw_host_alloc(n * tsz);
        j->results = (bsw_presult *)bsw_host_alloc(n * sizeof(bsw_presult));
        if (!j->tasks || !j->results) return job_fail(j, BSW_E_NOMEM, "%s: %zu bytes of DMA-able host memory", who, n * (tsz + sizeof(bsw_presult)));
        j->cap = n;
    }
    if (j->rd)
        memcpy(j->tasks, t, n * sizeof(*t));
    else {
        bsw_ptask *o = (bsw_ptask *)j->tasks;
        for (size_t i = 0; i < n; ++i) {
            o[i].query = j->reads[t[i].read]; o[i].l_query = j->lens[t[i].read]; o[i]._pad = 0; o[i].a = t[i].a; o[i].b = t[i].b;
        }
    }
    j->n = n; j->staged = true;
    return 1;
}

/* 1 submitted, BSW_E_BUSY no place (the round stays staged), another code: failed (the submit wrote the text) */
static int submit_round(bsw_sdp_job *j)
{
    const int rc = j->rd ? bsw_patch_reads_submit_t(j->ctx, &j->p, j->ref, j->rd, (const bsw_rd_ptask *)j->tasks, j->n, j->results, &j->ticket)
                         : bsw_patch_ref_submit_t(j->ctx, &j->p, j->ref, (const bsw_ptask *)j->tasks, j->n, j->results, &j->ticket);
    if (rc == BSW_E_BUSY) { j->ticket = 0; return rc; }
    if (rc) { j->ticket = 0; return job_fail(j, rc, nullptr); }
    j->staged = false;
    return 1;
}

/* Drives the rounds: 1 the engine has finished, 0 a round is in flight (wait == false only), BSW_E_BUSY a staged round found no
 * place, another code: the job has failed */
static int drive(bsw_sdp_job *j, bool wait, const char *who)
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
            const int fr = bsw_sdp_feed(j->eng, j->results, j->n);
            if (fr) return job_fail(j, fr, "%s: bsw_sdp_feed", who);
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

static int sdp_start(const char *who, bsw_ctx *ctx, const bsw_params *p, const bsw_sdp_opt *opt, const bsw_ref *ref, const bsw_reads *rd,
                     const uint8_t *const *reads, const int32_t *lens, size_t n_reads, const bsw_sreg *regs, size_t n_regs, const uint64_t *reg_start,
                     bsw_sdp_job **job)
{
    if (!ctx) return BSW_E_INVAL;
    errs e;
    if (job) *job = nullptr;
    if (!job || !p || !ref || (!rd && (!reads || !lens) && n_reads)) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "%s: NULL argument", who));
    if (rd && rd->owner != ctx) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "%s: the read block was uploaded through another context", who));
    std::unique_ptr<bsw_sdp_job> j(new bsw_sdp_job());
    j->ctx = ctx; j->p = *p; j->ref = ref; j->rd = rd; j->reads = reads;
    if (rd) {
        j->own_lens.resize(rd->rd.size());
        for (size_t i = 0; i < rd->rd.size(); ++i) j->own_lens[i] = rd->rd[i].len;
        j->lens = j->own_lens.data(); n_reads = rd->rd.size();
    } else
        j->lens = lens;
    char text[400] = "";
    int rc = bsw_sdp_open(p, opt, ref->l_pac, regs, n_regs, reg_start, j->lens, n_reads, &j->eng, text, sizeof(text));
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

extern "C" int bsw_sdp_ref_start(bsw_ctx *ctx, const bsw_params *p, const bsw_sdp_opt *opt, const bsw_ref *ref, const uint8_t *const *reads,
                                 const int32_t *lens, size_t n_reads, const bsw_sreg *regs, size_t n_regs, const uint64_t *reg_start, bsw_sdp_job **job)
{
    return sdp_start("bsw_sdp_ref_start", ctx, p, opt, ref, nullptr, reads, lens, n_reads, regs, n_regs, reg_start, job);
}

extern "C" int bsw_sdp_reads_start(bsw_ctx *ctx, const bsw_params *p, const bsw_sdp_opt *opt, const bsw_ref *ref, const bsw_reads *rd,
                                   const bsw_sreg *regs, size_t n_regs, const uint64_t *reg_start, bsw_sdp_job **job)
{
    if (ctx && !rd) {
        errs e;
        if (job) *job = nullptr;
        return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "bsw_sdp_reads_start: NULL argument"));
    }
    return sdp_start("bsw_sdp_reads_start", ctx, p, opt, ref, rd, nullptr, nullptr, 0, regs, n_regs, reg_start, job);
}

extern "C" int bsw_sdp_test(bsw_sdp_job *job)
{
    if (!job) return BSW_E_INVAL;
    const int rc = drive(job, false, "bsw_sdp_test");
    return rc == BSW_E_BUSY && !job->failed ? 0 : rc;
}

extern "C" int bsw_sdp_job_stats(const bsw_sdp_job *job, bsw_sdp_stats *stats)
{
    if (!job || !stats) return BSW_E_INVAL;
    return bsw_sdp_peek_stats(job->eng, stats);
}

extern "C" int bsw_sdp_finish(bsw_sdp_job *job, bsw_sreg *out, size_t *n_out, uint64_t *out_start, bsw_sdp_stats *stats)
{
    if (!job) return BSW_E_INVAL;
    bsw_ctx *ctx = job->ctx;
    if (n_out) *n_out = 0;
    int rc = drive(job, true, "bsw_sdp_finish");
    if (rc == BSW_E_BUSY && !job->failed) return rc; /* the job stays: its next round is staged, a later call submits it */
    if (rc == 1) {
        rc = bsw_sdp_collect(job->eng, out, n_out, out_start, stats);
        if (rc) {
            errs e;
            ctx_fail(ctx, e, fail(e, rc, "bsw_sdp_finish: NULL out"));
        }
    }
    job_free(job, ctx->dead);
    return rc;
}
