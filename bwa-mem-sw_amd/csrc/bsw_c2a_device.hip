/*
 * bsw_c2a_device.hip — the host side of the replay of mem_chain2aln's seed loop on the GPU (part of the host side of
 * libbwasw_mi355.so; no kernel here): the table through which the companion library libbwasw_c2a.so hands over its launcher
 * (bsw_c2a_device_register, after align_long_ops), its loading (bsw_c2a_device_load), the process-wide switch, the chunk function
 * on an f4_lane, and the two calls, bsw_chain2aln_replay_batch and bsw_chain2aln_replay_submit_t.
 *
 * A chunk is a range of chains cut between two reads.  Its function builds the compact read and chain records, DMAs them, the
 * chunk's seeds and the chunk's result records (registered memory from where it lies), launches through the table, reads the
 * per-read counts back, then the compact regions (and the flags when `extended` is asked for), and puts the regions at the read's
 * place in regs[]: behind the regions of every earlier seed there is room for them.  A read with a chain above
 * BSW_C2A_DEV_MAX_CHAIN seeds is replayed here by the host routine and merged in read order.  The chunk that finishes last turns
 * the counts into reg_start[] and closes the gaps, as bsw_c2a_replay_planned does for its thread parts.
 */
#include "bsw_f4_host.h"
#include "bsw_c2a_core.h"

#include <dlfcn.h>

extern "C" BSW_LOCAL int bsw_c2a_check_arrays(const char *who, const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds, size_t n_seeds,
                                              const int32_t *lens, size_t n_reads, char *err, size_t err_cap);
extern "C" BSW_LOCAL int bsw_c2a_replay_chains(const bsw_params *p, const bsw_c2a_opt *o, const bsw_chain *chains, size_t c0, size_t c1,
                                               const bsw_cseed *seeds, const int32_t *lens, const void *results, size_t stride, bsw_creg *regs,
                                               size_t *n_regs, uint8_t *extended);

/* ---- the table, the companion, the switch ---- */
static std::atomic<const c2a_dev_ops *> g_c2a_ops{nullptr};
BSW_LOCAL void c2a_dev_register(const c2a_dev_ops *ops) { g_c2a_ops.store(ops, std::memory_order_release); }
BSW_LOCAL const c2a_dev_ops *c2a_dev_registered() { return g_c2a_ops.load(std::memory_order_acquire); }

static std::mutex g_c2a_mu;                          /* the load and its text */
static char g_c2a_text[512];

extern "C" int bsw_c2a_device_register(const void *ops)
{
    if (!ops || !((const c2a_dev_ops *)ops)->launch) return BSW_E_INVAL;
    c2a_dev_register((const c2a_dev_ops *)ops);
    return BSW_OK;
}

extern "C" const char *bsw_c2a_device_error(void) { return g_c2a_text; }

extern "C" int bsw_c2a_device_load(const char *path)
{
    std::lock_guard<std::mutex> lk(g_c2a_mu);
    if (c2a_dev_registered()) return BSW_OK;
    std::string file;
    if (path) file = path;
    else {
        Dl_info info;
        if (!dladdr((const void *)&bsw_c2a_device_load, &info) || !info.dli_fname) {
            snprintf(g_c2a_text, sizeof(g_c2a_text), "bsw_c2a_device_load: cannot tell where this library lies");
            return BSW_E_INVAL;
        }
        file = info.dli_fname;
        const size_t slash = file.rfind('/');
        file = (slash == std::string::npos ? std::string("") : file.substr(0, slash + 1)) + "libbwasw_c2a.so";
    }
    if (!dlopen(file.c_str(), RTLD_NOW | RTLD_LOCAL)) {
        const char *why = dlerror();
        snprintf(g_c2a_text, sizeof(g_c2a_text), "bsw_c2a_device_load: %s", why ? why : file.c_str());
        return BSW_E_INVAL;
    }
    if (!c2a_dev_registered()) {
        snprintf(g_c2a_text, sizeof(g_c2a_text), "bsw_c2a_device_load: %s registered no launcher", file.c_str());
        return BSW_E_INVAL;
    }
    g_c2a_text[0] = 0;
    return BSW_OK;
}

/* 0 off, 1 on, 2: on by BSW_C2A_DEVICE=1 and the companion not looked for yet */
static std::atomic<int> &c2a_switch()
{
    static std::atomic<int> sw([] {
        const char *e = getenv("BSW_C2A_DEVICE");
        return e && e[0] == '1' && e[1] == 0 ? 2 : 0;
    }());
    return sw;
}

extern "C" int bsw_c2a_device(void)
{
    int v = c2a_switch().load(std::memory_order_relaxed);
    if (v == 2) {                                    /* first use under the environment's 1 */
        v = c2a_dev_registered() || bsw_c2a_device_load(nullptr) == BSW_OK ? 1 : 0;
        c2a_switch().store(v, std::memory_order_relaxed);
    }
    return v;
}

extern "C" int bsw_set_c2a_device(int on)
{
    if (on && !c2a_dev_registered()) {
        c2a_switch().store(0, std::memory_order_relaxed);
        std::lock_guard<std::mutex> lk(g_c2a_mu);
        snprintf(g_c2a_text, sizeof(g_c2a_text), "bsw_set_c2a_device: no launcher is registered (bsw_c2a_device_load)");
        return BSW_E_INVAL;
    }
    c2a_switch().store(on ? 1 : 0, std::memory_order_relaxed);
    return BSW_OK;
}

/* ---- one replay: what its chunks share.  The ticket's closure holds it; the caller's arrays are the caller's ---- */
#define C2A_DEV_CHUNK_SEEDS (1u << 17)               /* ~31 MB of device scratch under full records; a launch of that many rows fills the machine */
struct c2a_dev_job {
    bsw_params p{};
    bsw_c2a_opt opt{};
    c2a_dpar par{};
    const bsw_chain *chains = nullptr;
    const bsw_cseed *seeds = nullptr;
    const int32_t *lens = nullptr;
    const char *results = nullptr;
    size_t n_chains = 0, n_seeds = 0, n_reads = 0, stride = 0;
    bsw_creg *regs = nullptr;
    size_t *n_regs = nullptr;
    uint8_t *extended = nullptr;
    uint64_t *reg_start = nullptr;
    bsw_c2a_dev_stats *stats = nullptr;
    std::vector<chunk_span> spans;                   /* over chains */
    std::vector<uint64_t> chunk_regs;                /* per chunk: regions it placed at regs[first seed of the chunk] */
    std::atomic<size_t> left{0};                     /* chunks that have not succeeded yet */
    std::atomic<uint64_t> reads_gpu{0}, reads_host{0}, h2d{0}, d2h{0};
};

static size_t c2a_chunk_index(const c2a_dev_job &J, chunk_span c)
{
    size_t lo = 0, hi = J.spans.size();
    while (lo + 1 < hi) {
        const size_t mid = (lo + hi) / 2;
        if (J.spans[mid].base <= c.base) lo = mid; else hi = mid;
    }
    return lo;
}

/* after the last chunk: counts -> starts, the chunks' regions moved together, the counts of the whole */
static void c2a_dev_finalize(c2a_dev_job &J)
{
    size_t total = 0;
    for (size_t k = 0; k < J.spans.size(); ++k) {
        bsw_creg *at = J.regs + J.chains[J.spans[k].base].first_seed;
        if (at != J.regs + total && J.chunk_regs[k]) memmove(J.regs + total, at, J.chunk_regs[k] * sizeof(bsw_creg));
        total += J.chunk_regs[k];
    }
    if (J.reg_start)
        for (size_t r = 0; r < J.n_reads; ++r) J.reg_start[r + 1] += J.reg_start[r];
    if (J.stats) {
        J.stats->reads_gpu = J.reads_gpu; J.stats->reads_host = J.reads_host; J.stats->chunks = J.spans.size();
        J.stats->h2d_bytes = J.h2d; J.stats->d2h_bytes = J.d2h;
    }
    *J.n_regs = total;
}

static inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

static int c2a_dev_chunk(bsw_ctx *ctx, errs &e, f4_lane &L, c2a_dev_job &J, chunk_span c)
{
    const c2a_dev_ops *ops = c2a_dev_registered();
    if (!ops) return fail(e, BSW_E_INVAL, "chain2aln replay: no launcher is registered");
    const bsw_chain *ch = J.chains + c.base;
    const size_t nc = c.cnt, seed_lo = (size_t)ch[0].first_seed, ns = (size_t)(ch[nc - 1].first_seed + (uint64_t)ch[nc - 1].n_seeds) - seed_lo;
    /* the compact records (host memory a queued copy reads: in front of the drain) */
    std::vector<c2a_dchain> dch(nc);
    std::vector<c2a_dread> drd;
    size_t n_host = 0;
    for (size_t k = 0; k < nc; ++k) {
        c2a_dchain &d = dch[k];
        d.seed0 = (uint32_t)(ch[k].first_seed - seed_lo); d.n_seeds = ch[k].n_seeds; d.l_query = J.lens[ch[k].read];
        d.rid = ch[k].rid; d.frac_rep = ch[k].frac_rep; d.read = ch[k].read; d.chain = (uint32_t)(c.base + k); d._pad = 0;
        if (!k || ch[k].read != ch[k - 1].read) drd.push_back(c2a_dread{(uint32_t)k, 0, d.seed0, 0, 0, 0});
        c2a_dread &r = drd.back();
        ++r.n_chains; r.n_seeds += (uint32_t)ch[k].n_seeds;
        if (ch[k].n_seeds > BSW_C2A_DEV_MAX_CHAIN && !r.host) { r.host = 1; ++n_host; }
    }
    const size_t nr = drd.size();
    const size_t rdb = nr * sizeof(c2a_dread), chb = nc * sizeof(c2a_dchain), sdb = ns * sizeof(bsw_cseed), rsb = ns * J.stride, rgb = ns * sizeof(bsw_creg);
    /* the lane's arena: records | chains | seeds | results | staged regions | compact regions | counts | offsets | flags */
    const size_t o_rd = 0, o_ch = o_rd + up256(rdb), o_sd = o_ch + up256(chb), o_rs = o_sd + up256(sdb), o_st = o_rs + up256(rsb), o_out = o_st + up256(rgb),
                 o_cnt = o_out + up256(rgb), o_off = o_cnt + up256(nr * 4), o_fl = o_off + up256((nr + 1) * 4), arena = o_fl + up256(ns);
    int rc = reserve_all(e, "device staging", {{L.b->c2a, arena}});
    if (rc) return rc;
    if (L.h_back && (rc = reserve_all(e, "pinned staging", {{*L.h_back, nr * 4 + 4 + 16}, {*L.h_in, up256(rdb) + chb + 16}})) != BSW_OK) return rc;
    uint8_t *D = L.b->c2a.p;
    std::vector<uint32_t> cnt(nr);
    uint32_t total = 0;
    std::vector<bsw_creg> tmp;                       /* with host reads: the device's regions before the merge */
    drain_on_failure drain(ctx, L.s, L.ev);
    HIPCHK(e, hipMemcpyAsync(D + o_rd, L.dma_src(drd.data(), rdb, 0), rdb, hipMemcpyHostToDevice, L.s));
    HIPCHK(e, hipMemcpyAsync(D + o_ch, L.dma_src(dch.data(), chb, up256(rdb)), chb, hipMemcpyHostToDevice, L.s));
    HIPCHK(e, hipMemcpyAsync(D + o_sd, J.seeds + seed_lo, sdb, hipMemcpyHostToDevice, L.s));
    HIPCHK(e, hipMemcpyAsync(D + o_rs, J.results + seed_lo * J.stride, rsb, hipMemcpyHostToDevice, L.s));
    L.h2d += rdb + chb + sdb + rsb;
    c2a_dev_args a;
    memset(&a, 0, sizeof(a));
    a.reads = (const c2a_dread *)(D + o_rd); a.n_reads = (uint32_t)nr; a.chains = (const c2a_dchain *)(D + o_ch);
    a.seeds = (const bsw_cseed *)(D + o_sd); a.seed_base = (uint32_t)seed_lo; a.results = D + o_rs; a.stride = (uint32_t)J.stride; a.par = J.par;
    a.stage = (bsw_creg *)(D + o_st); a.out = (bsw_creg *)(D + o_out); a.counts = (uint32_t *)(D + o_cnt); a.offs = (uint32_t *)(D + o_off);
    a.flags = D + o_fl;
    const hipError_t le = (hipError_t)ops->launch(&a, (void *)L.s);
    if (le != hipSuccess) return fail(e, BSW_E_HIP, "chain2aln replay launch failed: %s", hipGetErrorString(le));
    if ((rc = lane_read_back(ctx, e, L, {{cnt.data(), a.counts, nr * 4}, {&total, a.offs + nr, 4}})) != BSW_OK) return rc;
    if (total > ns) return fail(e, BSW_E_HIP, "chain2aln replay: the device reports %u regions of %zu seeds", total, ns);
    bsw_creg *place = J.regs + seed_lo;
    if (n_host) tmp.resize(total);
    const size_t flb = J.extended ? ns : 0;
    if (L.h_back && (rc = reserve_all(e, "pinned staging", {{*L.h_back, (size_t)total * sizeof(bsw_creg) + flb + 16}})) != BSW_OK) return rc;
    if ((rc = lane_read_back(ctx, e, L, {{n_host ? tmp.data() : place, a.out, (size_t)total * sizeof(bsw_creg)}, {J.extended ? J.extended + seed_lo : nullptr, a.flags, flb}})) != BSW_OK)
        return rc;
    drain.done();
    size_t placed = total;
    if (n_host) {                                    /* the reads in order: the device's regions, or the host routine over the read's own chains */
        size_t from = 0;
        placed = 0;
        for (size_t r = 0; r < nr; ++r) {
            if (!drd[r].host) {
                memcpy(place + placed, tmp.data() + from, (size_t)cnt[r] * sizeof(bsw_creg));
                from += cnt[r];
            } else {
                size_t got = 0;
                const size_t c0 = c.base + drd[r].chain0;
                rc = bsw_c2a_replay_chains(&J.p, &J.opt, J.chains, c0, c0 + drd[r].n_chains, J.seeds, J.lens, J.results, J.stride, place + placed, &got, J.extended);
                if (rc) return fail(e, rc, "chain2aln replay: the host route of read %u", dch[drd[r].chain0].read);
                cnt[r] = (uint32_t)got;
            }
            placed += cnt[r];
        }
    }
    if (J.reg_start)
        for (size_t r = 0; r < nr; ++r) J.reg_start[(size_t)dch[drd[r].chain0].read + 1] = cnt[r];
    J.chunk_regs[c2a_chunk_index(J, c)] = placed;
    J.reads_gpu += nr - n_host; J.reads_host += n_host; J.h2d += L.h2d; J.d2h += L.d2h;
    if (J.left.fetch_sub(1) == 1) c2a_dev_finalize(J);
    return BSW_OK;
}

/* what both calls check, in bsw_chain2aln_replay's order, then the job: the arrays, the options, the chunks.  Nothing of the caller's
 * is written here: a call that is refused (the checks, BSW_E_BUSY) leaves the outputs as they were but for *n_regs = 0; c2a_dev_clear
 * follows once the call is going to run.  checked: the arrays have passed bsw_chain2aln_plan already (the job) */
static int c2a_dev_prepare(bsw_ctx *ctx, errs &e, const char *who, bool checked, const bsw_params *p, const bsw_c2a_opt *opt, const bsw_chain *chains, size_t n_chains,
                           const bsw_cseed *seeds, size_t n_seeds, const int32_t *lens, size_t n_reads, const void *results, int result_format,
                           bsw_creg *regs, size_t *n_regs, uint8_t *extended, uint64_t *reg_start, bsw_c2a_dev_stats *stats, std::shared_ptr<c2a_dev_job> &out)
{
    char text[400];
    const int rc = checked ? BSW_OK : bsw_c2a_check_arrays(who, chains, n_chains, seeds, n_seeds, lens, n_reads, text, sizeof(text));
    if (rc) return fail(e, rc, "%s", text);
    if (!p || !n_regs || (n_seeds && (!results || !regs)) || p->e_del < 1 || p->e_ins < 1) return fail(e, BSW_E_INVAL, "%s: NULL or bad argument", who);
    if (result_format != BSW_RESULT_FULL && result_format != BSW_RESULT_PAIR) return fail(e, BSW_E_INVAL, "%s: unknown result format %d", who, result_format);
    if (!c2a_dev_registered()) return fail(e, BSW_E_INVAL, "%s: no launcher is registered (bsw_c2a_device_load)", who);
    std::shared_ptr<c2a_dev_job> J(new c2a_dev_job());
    J->p = *p;
    if (opt) J->opt = *opt; else bsw_c2a_default_opt(&J->opt);
    J->par = c2a_dpar{p->mat[0], p->o_del, p->e_del, p->o_ins, p->e_ins, p->w, J->opt.seedlen0_frac, J->opt.ovl_len_frac};
    J->chains = chains; J->seeds = seeds; J->lens = lens; J->results = (const char *)results; J->n_chains = n_chains; J->n_reads = n_reads;
    J->stride = result_format == BSW_RESULT_PAIR ? sizeof(bsw_pair) : sizeof(bsw_result);
    J->regs = regs; J->n_regs = n_regs; J->extended = extended; J->reg_start = reg_start; J->stats = stats;
    J->n_seeds = n_seeds;
    /* spans of chains, cut only between two reads, closed once they hold their share of the seeds: a read larger than that stays whole */
    const uint64_t env_chunk = chunk_work_env("BSW_C2A_DEV_CHUNK", 0);      /* (read per call: tests and measurements change it between calls) */
    const uint64_t target = env_chunk ? env_chunk : std::max<uint64_t>(f4_chunk_work(ctx, n_seeds, C2A_DEV_CHUNK_SEEDS), 1);
    for (size_t a = 0; a < n_chains;) {
        size_t b = a;
        uint64_t held = 0;
        while (b < n_chains && (held < target || chains[b].read == chains[b - 1].read)) held += (uint64_t)chains[b++].n_seeds;
        J->spans.push_back(chunk_span{a, b - a});
        a = b;
    }
    J->chunk_regs.assign(J->spans.size(), 0);
    J->left = J->spans.size();
    out = J;
    return BSW_OK;
}

static void c2a_dev_clear(c2a_dev_job &J)
{
    *J.n_regs = 0;
    if (J.extended && J.n_seeds) memset(J.extended, 0, J.n_seeds);
    if (J.reg_start) memset(J.reg_start, 0, (J.n_reads + 1) * sizeof(uint64_t));
    if (J.stats) memset(J.stats, 0, sizeof(*J.stats));
}

extern "C" int bsw_chain2aln_replay_batch(bsw_ctx *ctx, const bsw_params *p, const bsw_c2a_opt *opt, const bsw_chain *chains, size_t n_chains,
                                          const bsw_cseed *seeds, size_t n_seeds, const int32_t *lens, size_t n_reads, const void *results,
                                          int result_format, bsw_creg *regs, size_t *n_regs, uint8_t *extended, uint64_t *reg_start,
                                          bsw_c2a_dev_stats *stats)
{
    if (!ctx) return BSW_E_INVAL;
    errs &e = ctx->err;
    if (n_regs) *n_regs = 0;
    std::shared_ptr<c2a_dev_job> J;
    int rc = c2a_dev_prepare(ctx, e, "bsw_chain2aln_replay_batch", false, p, opt, chains, n_chains, seeds, n_seeds, lens, n_reads, results, result_format, regs, n_regs,
                             extended, reg_start, stats, J);
    if (rc) return rc;
    if ((rc = busy_check(ctx, "bsw_chain2aln_replay_batch")) != BSW_OK) return rc;
    c2a_dev_clear(*J);
    if (J->spans.empty()) { c2a_dev_finalize(*J); return BSW_OK; }
    HIPCHK(e, hipSetDevice(ctx->device0()));
    f4_lane L = ctx_lane(ctx);
    for (const chunk_span &c : J->spans) {
        L.h2d = L.d2h = 0;
        if ((rc = c2a_dev_chunk(ctx, e, L, *J, c)) != BSW_OK) { *n_regs = 0; return rc; }
    }
    return BSW_OK;
}

static int c2a_dev_submit(bool checked, bsw_ctx *ctx, const bsw_params *p, const bsw_c2a_opt *opt, const bsw_chain *chains, size_t n_chains,
                          const bsw_cseed *seeds, size_t n_seeds, const int32_t *lens, size_t n_reads, const void *results, int result_format,
                          bsw_creg *regs, size_t *n_regs, uint8_t *extended, uint64_t *reg_start, bsw_c2a_dev_stats *stats, bsw_ticket *ticket)
{
    static const char who[] = "bsw_chain2aln_replay_submit";
    if (!ctx) return BSW_E_INVAL;
    if (ticket) *ticket = 0;
    if (n_regs) *n_regs = 0;
    errs e;                                          /* (several threads may submit at once: the context's text is set under its lock) */
    if (ctx->dead) return ctx_fail(ctx, e, fail(e, BSW_E_HIP, "%s: context is dead (an earlier wait for the GPU timed out)", who));
    std::shared_ptr<c2a_dev_job> J;
    int rc = c2a_dev_prepare(ctx, e, who, checked, p, opt, chains, n_chains, seeds, n_seeds, lens, n_reads, results, result_format, regs, n_regs, extended, reg_start, stats, J);
    if (rc) return ctx_fail(ctx, e, rc);
    /* a submit that would be refused changes nothing: the outputs are cleared only once a place is likely (another thread may still
     * take it in between: the arrays are then cleared and the answer is BSW_E_BUSY all the same) */
    if (bsw_inflight(ctx) >= BSW_MAX_INFLIGHT) return ctx_fail(ctx, e, fail(e, BSW_E_BUSY, "%s: %d submits in flight already (BSW_MAX_INFLIGHT)", who, BSW_MAX_INFLIGHT));
    c2a_dev_clear(*J);
    if (J->spans.empty()) c2a_dev_finalize(*J);      /* (no chain: a ticket without a chunk, complete at once) */
    f4_submit f;
    f.name = "c2a";
    f.spans = J->spans;
    f.run = [J](bsw_ctx *cx, errs &ce, f4_lane &L, chunk_span c) { return c2a_dev_chunk(cx, ce, L, *J, c); };
    return pipeline_submit_f4(ctx, std::move(f), ticket, who);
}

extern "C" int bsw_chain2aln_replay_submit_t(bsw_ctx *ctx, const bsw_params *p, const bsw_c2a_opt *opt, const bsw_chain *chains, size_t n_chains,
                                             const bsw_cseed *seeds, size_t n_seeds, const int32_t *lens, size_t n_reads, const void *results,
                                             int result_format, bsw_creg *regs, size_t *n_regs, uint8_t *extended, uint64_t *reg_start,
                                             bsw_c2a_dev_stats *stats, bsw_ticket *ticket)
{
    return c2a_dev_submit(false, ctx, p, opt, chains, n_chains, seeds, n_seeds, lens, n_reads, results, result_format, regs, n_regs, extended, reg_start, stats, ticket);
}

/* the chain2aln job's way here (bsw_internal.h: c2a_job_ops).  The job's arrays passed the plan at start and are the caller's to leave
 * unchanged: its submit skips the pass over them, so the job's poll stays O(chains) */
static int c2a_job_submit(bsw_ctx *ctx, const bsw_params *p, const bsw_c2a_opt *opt, const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds, size_t n_seeds,
                          const int32_t *lens, size_t n_reads, const void *results, int result_format, bsw_creg *regs, size_t *n_regs, uint8_t *extended,
                          uint64_t *reg_start, bsw_c2a_dev_stats *stats, bsw_ticket *ticket)
{
    return c2a_dev_submit(true, ctx, p, opt, chains, n_chains, seeds, n_seeds, lens, n_reads, results, result_format, regs, n_regs, extended, reg_start, stats, ticket);
}
static const c2a_job_ops g_job_ops = {bsw_c2a_device, c2a_job_submit};
static const struct c2a_job_registrar {
    c2a_job_registrar() { c2a_job_register(&g_job_ops); }
} g_c2a_job_registrar;
