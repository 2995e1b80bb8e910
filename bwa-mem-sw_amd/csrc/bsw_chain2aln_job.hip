/*
 * bsw_chain2aln_job.hip — mem_chain2aln as one job of the ticket pipeline (part of the host side of libbwasw_mi355.so; no kernel
 * here): bsw_chain2aln_ref_start / _reads_start plan a task per seed (bsw_chain2aln.c) into DMA-able memory and hand it to
 * bsw_submit_ref_t / bsw_submit_reads_t; bsw_chain2aln_finish collects the ticket and replays bwa's loop over the results.
 *
 * The job uses the context only through the ticket calls and the error channel, so it may be driven from several threads as
 * they may; one job belongs to one thread at a time.
 */
#include "bsw_internal.h"

struct bsw_c2a_job {
    bsw_ctx *ctx = nullptr;
    bsw_params p{};
    bsw_c2a_opt opt{};
    const bsw_chain *chains = nullptr;
    const bsw_cseed *seeds = nullptr;
    const int32_t *lens = nullptr;
    size_t n_chains = 0, n_seeds = 0, n_reads = 0;
    std::vector<int32_t> own_lens;    /* the reads form: the lengths of the block */
    void *tasks = nullptr, *results = nullptr;       /* bsw_host_alloc */
    int format = BSW_RESULT_FULL;
    bsw_ticket ticket = 0;            /* 0: nothing was submitted (no seed) */
};

static void job_free(bsw_c2a_job *j, bool abandon)
{
    if (!abandon) {                                  /* (a dead context's device may still write the arrays: they stay.  A ticket that merely
                                                        failed has left nothing on a stream when its wait returns: bsw_batch.hip) */
        if (j->tasks) bsw_host_free(j->tasks);
        if (j->results) bsw_host_free(j->results);
    }
    delete j;
}

static int c2a_start(const char *who, bsw_ctx *ctx, const bsw_params *p, const bsw_c2a_opt *opt, const bsw_ref *ref, const bsw_reads *rd,
                     const uint8_t *const *reads, const int32_t *lens, size_t n_reads, const bsw_chain *chains, size_t n_chains,
                     const bsw_cseed *seeds, size_t n_seeds, bsw_c2a_job **job)
{
    if (!ctx) return BSW_E_INVAL;
    errs e;
    if (job) *job = nullptr;
    if (!job || !p || !ref || (!rd && !reads && n_reads)) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "%s: NULL argument", who));
    if (rd && rd->owner != ctx) return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "%s: the read block was uploaded through another context", who));
    /* a start that the submit would refuse costs nothing: no pinned arrays, no plan (another thread may still take the last place
     * in between: the submit below then answers, and everything is given back) */
    if (n_seeds && bsw_inflight(ctx) >= BSW_MAX_INFLIGHT)
        return ctx_fail(ctx, e, fail(e, BSW_E_BUSY, "%s: %d submits in flight already (BSW_MAX_INFLIGHT)", who, BSW_MAX_INFLIGHT));
    std::unique_ptr<bsw_c2a_job> j(new bsw_c2a_job());
    j->ctx = ctx; j->p = *p;
    if (opt) j->opt = *opt; else bsw_c2a_default_opt(&j->opt);
    j->chains = chains; j->seeds = seeds; j->n_chains = n_chains; j->n_seeds = n_seeds;
    if (rd) {
        j->own_lens.resize(rd->rd.size());
        for (size_t i = 0; i < rd->rd.size(); ++i) j->own_lens[i] = rd->rd[i].len;
        j->lens = j->own_lens.data(); j->n_reads = rd->rd.size();
    } else {
        j->lens = lens; j->n_reads = n_reads;
    }
    j->format = ctx->cfg.result_format == BSW_RESULT_PAIR ? BSW_RESULT_PAIR : BSW_RESULT_FULL;
    const size_t tsz = rd ? sizeof(bsw_rd_task) : sizeof(bsw_ref_task), rsz = j->format == BSW_RESULT_PAIR ? sizeof(bsw_pair) : sizeof(bsw_result);
    if (n_seeds) {
        j->tasks = bsw_host_alloc(n_seeds * tsz);
        j->results = bsw_host_alloc(n_seeds * rsz);
        if (!j->tasks || !j->results) {
            job_free(j.release(), false);
            return ctx_fail(ctx, e, fail(e, BSW_E_NOMEM, "%s: %zu bytes of DMA-able host memory", who, n_seeds * (tsz + rsz)));
        }
    }
    char text[400];
    int rc = bsw_chain2aln_plan(p, ref->l_pac, chains, n_chains, seeds, n_seeds, j->lens, j->n_reads, rd ? nullptr : reads,
                                rd ? (bsw_rd_task *)j->tasks : nullptr, rd ? nullptr : (bsw_ref_task *)j->tasks, text, sizeof(text));
    if (rc) {
        job_free(j.release(), false);
        return ctx_fail(ctx, e, fail(e, rc, "%s", text));
    }
    if (n_seeds) {
        rc = rd ? bsw_submit_reads_t(ctx, p, ref, rd, (const bsw_rd_task *)j->tasks, n_seeds, (bsw_result *)j->results, &j->ticket)
                : bsw_submit_ref_t(ctx, p, ref, (const bsw_ref_task *)j->tasks, n_seeds, (bsw_result *)j->results, &j->ticket);
        if (rc) {                                    /* (the submit wrote the text; nothing is queued) */
            job_free(j.release(), false);
            return rc;
        }
    }
    *job = j.release();
    return BSW_OK;
}

extern "C" int bsw_chain2aln_ref_start(bsw_ctx *ctx, const bsw_params *p, const bsw_c2a_opt *opt, const bsw_ref *ref, const uint8_t *const *reads,
                                       const int32_t *lens, size_t n_reads, const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds,
                                       size_t n_seeds, bsw_c2a_job **job)
{
    return c2a_start("bsw_chain2aln_ref_start", ctx, p, opt, ref, nullptr, reads, lens, n_reads, chains, n_chains, seeds, n_seeds, job);
}

extern "C" int bsw_chain2aln_reads_start(bsw_ctx *ctx, const bsw_params *p, const bsw_c2a_opt *opt, const bsw_ref *ref, const bsw_reads *rd,
                                         const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds, size_t n_seeds, bsw_c2a_job **job)
{
    if (ctx && !rd) {
        errs e;
        if (job) *job = nullptr;
        return ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "bsw_chain2aln_reads_start: NULL argument"));
    }
    return c2a_start("bsw_chain2aln_reads_start", ctx, p, opt, ref, rd, nullptr, nullptr, 0, chains, n_chains, seeds, n_seeds, job);
}

extern "C" int bsw_chain2aln_test(bsw_c2a_job *job)
{
    if (!job) return BSW_E_INVAL;
    return job->ticket ? bsw_test(job->ctx, job->ticket) : 1;
}

static void job_stats(const bsw_c2a_job *j, uint64_t regs, bsw_c2a_stats *s)
{
    s->seeds_gpu = j->n_seeds; s->seeds_bwa = regs; s->regs = regs; s->chains = j->n_chains; s->reads = j->n_reads;
}

extern "C" int bsw_chain2aln_stats(const bsw_c2a_job *job, bsw_c2a_stats *stats)
{
    if (!job || !stats) return BSW_E_INVAL;
    job_stats(job, 0, stats);
    return BSW_OK;
}

extern "C" int bsw_chain2aln_finish(bsw_c2a_job *job, bsw_creg *regs, size_t *n_regs, uint8_t *extended, uint64_t *reg_start, bsw_c2a_stats *stats)
{
    if (!job) return BSW_E_INVAL;
    bsw_ctx *ctx = job->ctx;
    if (n_regs) *n_regs = 0;
    int rc = job->ticket ? bsw_wait_ticket(ctx, job->ticket) : BSW_OK;
    if (rc == BSW_OK) {
        size_t n = 0;
        /* (the plan checked the chains and seeds at start, and they are the caller's to leave unchanged until now; reads are
         * independent, so the block's reads are split over the context's helper threads: pack_threads, a part per 1 024 seeds at most) */
        rc = bsw_c2a_replay_planned(&job->p, &job->opt, job->chains, job->n_chains, job->seeds, job->n_seeds, job->lens, job->n_reads, job->results,
                                    job->format, regs, &n, extended, reg_start, ctx->cfg.pack_threads);
        if (rc) {
            errs e;
            ctx_fail(ctx, e, fail(e, rc, "bsw_chain2aln_finish: NULL regs"));
        } else {
            if (n_regs) *n_regs = n;
            if (stats) job_stats(job, n, stats);
        }
    }
    job_free(job, ctx->dead);
    return rc;
}
