/*
 * bsw_chain2aln_job.hip — mem_chain2aln as one job of the ticket pipeline (part of the host side of libbwasw_mi355.so; no kernel
 * here): bsw_chain2aln_ref_start / _reads_start plan a task per seed (bsw_chain2aln.c) into DMA-able memory and hand it to
 * bsw_submit_ref_t / bsw_submit_reads_t; bsw_chain2aln_finish collects the ticket and replays bwa's loop over the results — on the
 * host, or, when bsw_c2a_device() was on at start, as a second ticket on the GPU (bsw_c2a_device.hip; job_advance below).
 *
 * The job uses the context only through the ticket calls and the error channel, so it may be driven from several threads as
 * they may; one job belongs to one thread at a time.
 */
#include "bsw_internal.h"

static std::atomic<const c2a_job_ops *> g_c2a_job_ops{nullptr};
BSW_LOCAL void c2a_job_register(const c2a_job_ops *ops) { g_c2a_job_ops.store(ops, std::memory_order_release); }

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
    /* bsw_c2a_device() at start: the replay runs as a second ticket behind the extension's (bsw_c2a_device.hip) into arrays of the
     * job's own — test() may submit it, and only finish() knows the caller's */
    int dev = 0;
    int stage = 0;                    /* 0: the extension ticket is in flight; 1: it is collected, the replay ticket is wanted (rticket == 0) or in flight; 2: over */
    int rc = 0;                       /* stage 2: the failure of either ticket */
    bsw_ticket rticket = 0;
    std::unique_ptr<bsw_creg[]> d_regs;
    std::unique_ptr<uint8_t[]> d_ext;
    std::unique_ptr<uint64_t[]> d_start;
    size_t d_n = 0;
    bsw_c2a_dev_stats d_stats{};
};

static void job_free(bsw_c2a_job *j, bool abandon)
{
    if (!abandon) {                                  /* (a dead context's device may still write the arrays: they stay.  A ticket that merely
                                                        failed has left nothing on a stream when its wait returns: bsw_batch.hip) */
        if (j->tasks) bsw_host_free(j->tasks);
        if (j->results) bsw_host_free(j->results);
    } else {
        (void)j->d_regs.release(); (void)j->d_ext.release(); (void)j->d_start.release();
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
    const c2a_job_ops *dops = g_c2a_job_ops.load(std::memory_order_acquire);
    j->dev = n_seeds && dops && dops->on() == 1;      /* the switch, once per job, in the caller's thread (a job without a seed has nothing to replay) */
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

/* The two-stage job (the switch was on at start) one step further: 1 over (job->rc: how), 0 in flight, < 0 an answer that leaves the
 * job as it is — bsw_test's own failure, or, blocking, BSW_E_BUSY of the replay submit (the four places are other tickets').  Not
 * blocking, that BSW_E_BUSY is 0: the next call tries again. */
static int job_advance(bsw_c2a_job *j, bool block)
{
    bsw_ctx *ctx = j->ctx;
    if (j->stage == 0) {
        if (!block) {
            const int t = bsw_test(ctx, j->ticket);
            if (t <= 0) return t;
        }
        const int rc = bsw_wait_ticket(ctx, j->ticket);
        j->ticket = 0;
        j->stage = rc ? 2 : 1;
        j->rc = rc;
    }
    if (j->stage == 1 && !j->rticket) {
        /* the poll asks first: a refused submit would leave its text in the context, and BSW_E_BUSY is not the poll's error (another
         * thread may still take the place in between: the submit's own answer below is handled the same way) */
        if (!block && bsw_inflight(ctx) >= BSW_MAX_INFLIGHT) return 0;
        if (!j->d_regs) {
            j->d_regs.reset(new (std::nothrow) bsw_creg[j->n_seeds]);
            j->d_ext.reset(new (std::nothrow) uint8_t[j->n_seeds]);
            j->d_start.reset(new (std::nothrow) uint64_t[j->n_reads + 1]);
            if (!j->d_regs || !j->d_ext || !j->d_start) {
                errs e;
                j->stage = 2;
                j->rc = ctx_fail(ctx, e, fail(e, BSW_E_NOMEM, "bsw_chain2aln: %zu bytes for the regions", j->n_seeds * (sizeof(bsw_creg) + 1)));
                return 1;
            }
        }
        const int rc = g_c2a_job_ops.load(std::memory_order_acquire)->submit(ctx, &j->p, &j->opt, j->chains, j->n_chains, j->seeds, j->n_seeds, j->lens, j->n_reads, j->results, j->format,
                                                                             j->d_regs.get(), &j->d_n, j->d_ext.get(), j->d_start.get(), &j->d_stats, &j->rticket);
        if (rc == BSW_E_BUSY) return block ? rc : 0;
        if (rc) { j->stage = 2; j->rc = rc; return 1; }
    }
    if (j->stage == 1) {
        if (!block) return bsw_test(ctx, j->rticket);     /* (complete: it stays the job's to collect, in finish) */
        j->rc = bsw_wait_ticket(ctx, j->rticket);
        j->rticket = 0;
        j->stage = 2;
    }
    return 1;
}

extern "C" int bsw_chain2aln_test(bsw_c2a_job *job)
{
    if (!job) return BSW_E_INVAL;
    if (job->dev) return job_advance(job, false);
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
    if (job->dev) {
        int rc;
        if (!regs && job->stage < 2 && !job->rticket) {      /* a job that is dropped before its replay was submitted: none is started for it */
            rc = job->stage == 0 ? bsw_wait_ticket(ctx, job->ticket) : BSW_OK;
            job->ticket = 0;
            job->stage = 2;
            job->rc = rc;
        } else {
            rc = job_advance(job, true);
            if (rc != 1 && job->stage != 2) {         /* BSW_E_BUSY: the job stays intact, the caller calls again */
                if (rc == BSW_E_BUSY) return rc;
                job->stage = 2;                       /* (a ticket that was collected behind the job's back: nothing is left to wait for) */
                job->rc = rc < 0 ? rc : BSW_E_INVAL;
            }
        }
        rc = job->rc;
        if (!rc && !regs) {
            errs e;
            rc = ctx_fail(ctx, e, fail(e, BSW_E_INVAL, "bsw_chain2aln_finish: NULL regs"));
        } else if (!rc) {
            if (job->d_n) memcpy(regs, job->d_regs.get(), job->d_n * sizeof(bsw_creg));
            if (extended) memcpy(extended, job->d_ext.get(), job->n_seeds);
            if (reg_start) memcpy(reg_start, job->d_start.get(), (job->n_reads + 1) * sizeof(uint64_t));
            if (n_regs) *n_regs = job->d_n;
            if (stats) job_stats(job, job->d_n, stats);
        }
        job_free(job, ctx->dead);
        return rc;
    }
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
