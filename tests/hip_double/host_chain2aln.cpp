/* host_chain2aln.cpp — the mem_chain2aln job (bsw_chain2aln_ref_start / _reads_start / _test / _finish / _stats:
 * bsw_chain2aln_job.hip over bsw_chain2aln.c and bsw_batch.hip's pipeline) on the host-memory HIP stand-in, plain and under ASan /
 * UBSan or TSan (TEST INFRASTRUCTURE; tests/test_chain2aln_double_cpu.py builds it with its row in tests/_host_double_build.py and runs it).
 * A stand-alone program: nothing is preloaded, no GPU is opened.
 *
 * What the job must hand back is bsw_chain2aln_replay over the CPU oracle's records of the plan's tasks (the sequences cut on the
 * host with bsw_pac_get_seq and bsw_seed_to_task); the replay itself is checked against its sequential restatement in
 * tests/test_chain2aln_cpu.py.
 *
 *   host_chain2aln forms    start / test / finish by pointer and by read index on 1, 2 and 3 devices, variants H, M and RTL,
 *                           full and pair records, chunks smaller than a read's seeds; an empty job
 *   host_chain2aln mixed    two jobs in flight beside a CIGAR and an extension ticket; the fifth submit is refused and leaves no
 *                           job; finish after a failed start; a plan failure and a submit failure from start
 *   host_chain2aln faults   every HIP / launcher call of a start .. finish of each form fails in turn; the job is freed
 */
#include <climits>
#include "host_ref_patch.h"

/* reads of 100 - 250 bases off both strands with substitutions; per read the true chain (its exact-match runs as seeds, long runs
 * cut in two), sometimes a thinned copy of it, sometimes a decoy chain; some chains carry a contig interval close around them */
struct cwork {
    std::vector<std::vector<uint8_t>> reads;
    std::vector<const uint8_t *> ptr;
    std::vector<int32_t> len;
    std::vector<bsw_chain> chains;
    std::vector<bsw_cseed> seeds;
    std::vector<bsw_creg> want;
    std::vector<uint8_t> want_ext;
    std::vector<uint64_t> want_start;
};

static void push_chain(cwork &w, uint32_t read, const std::vector<bsw_cseed> &ss, int64_t rlo, int64_t rhi, int rid, float frac)
{
    bsw_chain c;
    memset(&c, 0, sizeof(c));
    c.read = read; c.n_seeds = (int32_t)ss.size(); c.first_seed = w.seeds.size(); c.rlo = rlo; c.rhi = rhi; c.rid = rid; c.frac_rep = frac;
    w.chains.push_back(c);
    w.seeds.insert(w.seeds.end(), ss.begin(), ss.end());
}

static void make_chains(cwork &w, const genome_t &g, rng_t &r, size_t n_reads)
{
    const int64_t L = g.l_pac;
    for (size_t i = 0; i < n_reads; ++i) {
        const int len = r.in(100, 250);
        const bool rev = r.below(2) == 1;
        int64_t x = (rev ? L : 0) + 300 + r.below((int)(L - len - 600));
        if (i % 9 == 4) x = rev ? L + r.below(20) : L - len - r.below(20);        /* the window would bridge l_pac */
        std::vector<uint8_t> q(g.both.begin() + x, g.both.begin() + x + len);
        std::vector<int> brk;
        for (int k = 0; k < len; ++k)
            if (r.unit() < 0.03) { q[(size_t)k] = (uint8_t)((q[(size_t)k] + 1 + r.below(3)) & 3); brk.push_back(k); }
        brk.push_back(len);
        std::vector<bsw_cseed> ss;
        int a = 0;
        for (int b : brk) {
            int n = b - a;
            if (n >= 12) {
                if (n >= 30 && r.below(2)) {
                    const int m = r.in(12, n - 12);
                    ss.push_back(bsw_cseed{x + a, a, m + r.below(6), m, 0});
                    ss.push_back(bsw_cseed{x + a + m, a + m, n - m, n - m, 0});
                } else
                    ss.push_back(bsw_cseed{x + a, a, n, i % 4 == 0 ? r.in(10, 40) : n, 0});
            }
            a = b + 1;
        }
        if (ss.empty()) ss.push_back(bsw_cseed{x, 0, 12, 12, 0});
        if (i % 5 == 2 && i % 3 != 0 && i % 9 != 4) ss.push_back(bsw_cseed{ss[0].rbeg + 2, ss[0].qbeg, ss[0].len, ss[0].score, 0});      /* another diagonal over the first seed */
        const bool contig = i % 3 == 0;
        const int64_t lo = std::max<int64_t>(x - r.below(40), rev ? L : 0), hi = std::min<int64_t>(x + len + r.below(40), rev ? 2 * L : L);
        if (i % 7 == 3) push_chain(w, (uint32_t)i, {ss[(size_t)r.below((int)ss.size())]}, 0, 0, 1, 0.5f);       /* a one-seed chain in front */
        push_chain(w, (uint32_t)i, ss, contig ? lo : 0, contig ? hi : 0, 2, 0.125f);
        if (i % 4 == 1) {
            std::vector<bsw_cseed> half;
            for (size_t k = 0; k < ss.size(); k += 2) half.push_back(ss[k]);
            push_chain(w, (uint32_t)i, half, 0, 0, 2, 0.25f);
        }
        if (i % 3 == 1) {
            const int64_t y = (r.below(2) ? L : 0) + 300 + r.below((int)(L - len - 600));
            push_chain(w, (uint32_t)i, {bsw_cseed{y + 5, 5, 19, 19, 0}, bsw_cseed{y + 60, 60, 25, 25, 0}}, 0, 0, -1, 0.f);
        }
        w.reads.push_back(q);
    }
    for (auto &q : w.reads) { w.ptr.push_back(q.data()); w.len.push_back((int32_t)q.size()); }
}

/* the plan's tasks cut on the host, through the oracle, through the replay */
static void expect(cwork &w, const genome_t &g, const bsw_params &p, bool pair)
{
    const size_t n = w.seeds.size();
    std::vector<bsw_ref_task> rt(n);
    char text[400];
    const int rc = bsw_chain2aln_plan(&p, g.l_pac, w.chains.data(), w.chains.size(), w.seeds.data(), n, w.len.data(), w.len.size(), w.ptr.data(), nullptr, rt.data(), text, sizeof(text));
    CHECK(rc == BSW_OK, "bsw_chain2aln_plan -> %d (%s)", rc, text);
    std::vector<bsw_task> t(n);
    std::vector<std::vector<uint8_t>> keep(2 * n);
    for (size_t i = 0; i < n; ++i) {
        const bsw_ref_task &x = rt[i];
        CHECK(x.tag == i && x.init_score == -1, "task %zu: tag %u, init_score %d", i, x.tag, x.init_score);
        std::vector<uint8_t> &rseq = keep[2 * i], &scratch = keep[2 * i + 1];
        rseq.resize((size_t)(x.rmax1 - x.rmax0) + 1);
        CHECK(bsw_pac_get_seq(g.l_pac, g.pac.data(), x.rmax0, x.rmax1, rseq.data()) == x.rmax1 - x.rmax0, "task %zu: the window [%lld, %lld) bridges l_pac", i, (long long)x.rmax0, (long long)x.rmax1);
        scratch.resize(bsw_seed_scratch_bytes(&x.seed, x.rmax0) + 1);
        CHECK(bsw_seed_to_task(&p, &x.seed, x.l_query, x.query, x.rmax0, x.rmax1, rseq.data(), scratch.data(), scratch.size(), x.tag, &t[i]) == BSW_OK, "bsw_seed_to_task %zu", i);
    }
    const std::vector<bsw_result> res = expected(p, t.data(), n);
    std::vector<bsw_pair> pr(n);
    for (size_t i = 0; i < n; ++i) memcpy(&pr[i], &res[i], sizeof(bsw_pair));
    w.want.assign(n + 1, bsw_creg());
    w.want_ext.assign(n + 1, 0);
    w.want_start.assign(w.len.size() + 1, 0);
    size_t nr = 0;
    CHECK(bsw_chain2aln_replay(&p, nullptr, w.chains.data(), w.chains.size(), w.seeds.data(), n, w.len.data(), w.len.size(), pair ? (const void *)pr.data() : (const void *)res.data(),
                               pair ? BSW_RESULT_PAIR : BSW_RESULT_FULL, w.want.data(), &nr, w.want_ext.data(), w.want_start.data()) == BSW_OK, "bsw_chain2aln_replay");
    w.want.resize(nr);
    CHECK(nr > n / 5 && nr < n - n / 5, "the workload: %zu regions of %zu seeds", nr, n);
}

static bsw_ctx *ctx_of(int n_dev, size_t chunk_tasks, int format, int timeout_ms = 20000, int streams = 2)
{
    bsw_config c;
    bsw_default_config(&c);
    c.kernel = BSW_KERNEL_AUTO; c.streams = streams; c.pack_threads = 4; c.chunk_tasks = chunk_tasks; c.timeout_ms = timeout_ms;
    c.n_devices = n_dev; c.result_format = format;
    for (int k = 0; k < n_dev; ++k) c.devices[k] = k;
    bsw_ctx *ctx = nullptr;
    const int rc = bsw_create(&c, &ctx);
    CHECK(rc == BSW_OK && ctx, "bsw_create -> %d", rc);
    return ctx;
}

struct outs {
    std::vector<bsw_creg> regs;
    std::vector<uint8_t> ext;
    std::vector<uint64_t> start;
    size_t n = 77;
    bsw_c2a_stats st;
    explicit outs(const cwork &w) : regs(w.seeds.size() + 1), ext(w.seeds.size() + 1, 0x5a), start(w.len.size() + 2, 0x5a5a)
    {
        memset(regs.data(), 0x5a, regs.size() * sizeof(bsw_creg));
        memset(&st, 0, sizeof(st));
    }
};

static int finish(bsw_c2a_job *j, outs &o) { return bsw_chain2aln_finish(j, o.regs.data(), &o.n, o.ext.data(), o.start.data(), &o.st); }

static void same_c(const outs &o, const cwork &w, const char *what)
{
    const size_t n = w.seeds.size();
    CHECK(o.n == w.want.size(), "%s: %zu regions, want %zu", what, o.n, w.want.size());
    for (size_t i = 0; i < o.n; ++i)
        if (memcmp(&o.regs[i], &w.want[i], sizeof(bsw_creg)) != 0)
            CHECK(false, "%s: region %zu of %zu: seed %u [%lld, %lld) score %d, want seed %u [%lld, %lld) score %d", what, i, o.n, o.regs[i].seed, (long long)o.regs[i].rb,
                  (long long)o.regs[i].re, o.regs[i].score, w.want[i].seed, (long long)w.want[i].rb, (long long)w.want[i].re, w.want[i].score);
    CHECK(memcmp(o.ext.data(), w.want_ext.data(), n) == 0, "%s: extended[] differs", what);
    CHECK(memcmp(o.start.data(), w.want_start.data(), (w.len.size() + 1) * sizeof(uint64_t)) == 0, "%s: reg_start[] differs", what);
    CHECK(o.ext[n] == 0x5a && o.start[w.len.size() + 1] == 0x5a5a && o.regs[n].seed == 0x5a5a5a5au, "%s: a write behind the caller's arrays", what);
    CHECK(o.st.seeds_gpu == n && o.st.seeds_bwa == o.n && o.st.regs == o.n && o.st.chains == w.chains.size() && o.st.reads == w.len.size(), "%s: the stats", what);
}

static bsw_params params_of(int variant)
{
    bsw_params p;
    bsw_default_params(&p);
    p.variant = variant;
    return p;
}
static int start_ref(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, const cwork &w, bsw_c2a_job **j)
{
    return bsw_chain2aln_ref_start(ctx, &p, nullptr, ref, w.ptr.data(), w.len.data(), w.len.size(), w.chains.data(), w.chains.size(), w.seeds.data(), w.seeds.size(), j);
}
static int start_reads(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, bsw_reads *rd, const cwork &w, bsw_c2a_job **j)
{
    return bsw_chain2aln_reads_start(ctx, &p, nullptr, ref, rd, w.chains.data(), w.chains.size(), w.seeds.data(), w.seeds.size(), j);
}

/* both forms once on a context */
static void both_forms(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, const cwork &w, const char *what)
{
    bsw_c2a_job *j1 = nullptr, *j2 = nullptr;
    int rc = start_ref(ctx, p, ref, w, &j1);
    CHECK(rc == BSW_OK && j1, "%s: bsw_chain2aln_ref_start -> %d (%s)", what, rc, bsw_last_error(ctx));
    bsw_reads *rd = upload_reads(ctx, w);
    rc = start_reads(ctx, p, ref, rd, w, &j2);
    CHECK(rc == BSW_OK && j2, "%s: bsw_chain2aln_reads_start -> %d (%s)", what, rc, bsw_last_error(ctx));
    CHECK(bsw_inflight(ctx) == 2, "%s: %d submits in flight", what, bsw_inflight(ctx));
    bsw_c2a_stats st;
    CHECK(bsw_chain2aln_stats(j1, &st) == BSW_OK && st.seeds_gpu == w.seeds.size() && st.regs == 0, "%s: the stats of a job in flight", what);
    CHECK(bsw_reads_free(ctx, rd) == BSW_E_BUSY, "%s: bsw_reads_free while the job holds the block", what);
    int t1 = 0, t2 = 0;
    while ((t1 = bsw_chain2aln_test(j1)) == 0 || (t2 = bsw_chain2aln_test(j2)) == 0) std::this_thread::yield();
    CHECK(t1 == 1 && t2 == 1, "%s: bsw_chain2aln_test -> %d %d", what, t1, t2);
    CHECK(bsw_inflight(ctx) == 2, "%s: a poll collected a ticket", what);
    outs o1(w), o2(w);
    CHECK(finish(j1, o1) == BSW_OK, "%s: finish of the pointer job: %s", what, bsw_last_error(ctx));
    CHECK(finish(j2, o2) == BSW_OK, "%s: finish of the reads job: %s", what, bsw_last_error(ctx));
    CHECK(bsw_inflight(ctx) == 0, "%s: tickets left", what);
    CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "%s: bsw_reads_free after finish: %s", what, bsw_last_error(ctx));
    same_c(o1, w, what);
    same_c(o2, w, what);
}

static int forms_mode()
{
    genome_t g;
    g.make(70001, 5);
    size_t runs = 0;
    for (int D : {1, 2, 3})
        for (int variant : {BSW_VARIANT_H, BSW_VARIANT_M, BSW_VARIANT_RTL})
            for (int format : {BSW_RESULT_FULL, BSW_RESULT_PAIR}) {
                if (D > 1 && variant != (D == 2 ? BSW_VARIANT_H : BSW_VARIANT_RTL)) continue;
                fresh(D);
                {
                    rng_t r(50 + (uint64_t)D);
                    cwork w;
                    make_chains(w, g, r, 260);
                    const bsw_params p = params_of(variant);
                    expect(w, g, p, format == BSW_RESULT_PAIR);
                    bsw_ctx *ctx = ctx_of(D, 256, format);                 /* a read's seeds fall into different chunks and on different devices */
                    bsw_ref *ref = upload(ctx, g);
                    both_forms(ctx, p, ref, w, format == BSW_RESULT_PAIR ? "pair records" : "full records");
                    /* an empty job: complete at once, no ticket */
                    bsw_c2a_job *j = nullptr;
                    size_t n = 9;
                    uint64_t start[1] = {7};
                    CHECK(bsw_chain2aln_ref_start(ctx, &p, nullptr, ref, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, &j) == BSW_OK && j, "an empty job: %s", bsw_last_error(ctx));
                    CHECK(bsw_inflight(ctx) == 0 && bsw_chain2aln_test(j) == 1, "an empty job is complete");
                    CHECK(bsw_chain2aln_finish(j, nullptr, &n, nullptr, start, nullptr) == BSW_OK && n == 0 && start[0] == 0, "finish of an empty job");
                    bsw_ref_free(ctx, ref);
                    bsw_destroy(ctx);
                    ++runs;
                }
                CHECK(hipdbl::live_objects() == 0, "%zu HIP objects left alive", hipdbl::live_objects());
            }
    printf("forms: %zu contexts\nforms ok\n", runs);
    return 0;
}

static int mixed_mode()
{
    genome_t g;
    g.make(70001, 5);
    fresh(2);
    {
        const bsw_params p = params_of(BSW_VARIANT_H);
        rng_t r(8);
        cwork w;
        make_chains(w, g, r, 200);
        expect(w, g, p, false);
        workload we;
        make_workload(we, 1200, 150, 9, true);
        const std::vector<bsw_result> want_e = expected(p, we.tasks.data(), 1200);
        std::vector<bsw_ctask> ct;
        for (size_t i = 0; i < 64; ++i) {            /* exact pieces of the genome: the score is the length */
            bsw_ctask c;
            memset(&c, 0, sizeof(c));
            c.query = g.both.data() + 1000 + 200 * i; c.l_query = 100 + (int)i; c.w = 10; c.rb = 1000 + 200 * (int64_t)i; c.re = c.rb + c.l_query;
            c.min_score = INT_MIN; c.max_tries = 1;
            ct.push_back(c);
        }
        bsw_ctx *ctx = ctx_of(2, 256, BSW_RESULT_FULL);
        bsw_ref *ref = upload(ctx, g);
        bsw_reads *rd = upload_reads(ctx, w);
        std::vector<bsw_result> eo(1200);
        std::vector<bsw_cresult> co(ct.size());
        bsw_ticket te = 0, tc = 0;
        bsw_c2a_job *j1 = nullptr, *j2 = nullptr, *j5 = (bsw_c2a_job *)&g;
        CHECK(bsw_cigar_ref_submit_t(ctx, &p, ref, ct.data(), ct.size(), 64, nullptr, 0, nullptr, co.data(), &tc) == BSW_OK, "CIGAR: %s", bsw_last_error(ctx));
        CHECK(start_ref(ctx, p, ref, w, &j1) == BSW_OK && j1, "the pointer job: %s", bsw_last_error(ctx));
        CHECK(bsw_submit_t(ctx, &p, we.tasks.data(), 1200, eo.data(), &te) == BSW_OK, "extension: %s", bsw_last_error(ctx));
        CHECK(start_reads(ctx, p, ref, rd, w, &j2) == BSW_OK && j2, "the reads job: %s", bsw_last_error(ctx));
        CHECK(bsw_inflight(ctx) == 4, "four submits");
        /* the fifth: refused, no job, nothing changed */
        CHECK(start_ref(ctx, p, ref, w, &j5) == BSW_E_BUSY && j5 == nullptr, "the fifth submit as a pointer job");
        j5 = (bsw_c2a_job *)&g;
        CHECK(start_reads(ctx, p, ref, rd, w, &j5) == BSW_E_BUSY && j5 == nullptr, "the fifth submit as a reads job");
        CHECK(bsw_inflight(ctx) == 4, "a refused start changed the tickets");       /* (what it allocated: the leak check, and live_objects() at the end) */
        /* finish after a failed start */
        outs o5(w);
        CHECK(finish(j5, o5) == BSW_E_INVAL && bsw_chain2aln_test(j5) == BSW_E_INVAL && bsw_chain2aln_stats(j5, &o5.st) == BSW_E_INVAL, "the calls on no job");
        CHECK(o5.regs[0].seed == 0x5a5a5a5au, "finish of no job wrote regions");
        outs o1(w), o2(w);
        CHECK(finish(j2, o2) == BSW_OK, "the reads job: %s", bsw_last_error(ctx));
        CHECK(bsw_wait_ticket(ctx, tc) == BSW_OK, "the CIGAR ticket: %s", bsw_last_error(ctx));
        CHECK(finish(j1, o1) == BSW_OK, "the pointer job: %s", bsw_last_error(ctx));
        CHECK(bsw_wait_ticket(ctx, te) == BSW_OK, "the extension ticket: %s", bsw_last_error(ctx));
        CHECK(bsw_inflight(ctx) == 0, "tickets left");
        same_c(o1, w, "the pointer job beside other tickets");
        same_c(o2, w, "the reads job beside other tickets");
        CHECK(memcmp(eo.data(), want_e.data(), 1200 * sizeof(bsw_result)) == 0, "the extension ticket beside the jobs");
        for (size_t k = 0; k < ct.size(); ++k) CHECK(co[k].status == 0 && co[k].score == ct[k].l_query, "CIGAR task %zu: score %d", k, co[k].score);
        /* a start that fails in the plan, and one that fails in the submit: the code, a text, no job, nothing queued */
        cwork bad;
        bad.reads = w.reads; bad.ptr = w.ptr; bad.len = w.len; bad.chains = w.chains; bad.seeds = w.seeds;
        bad.seeds[0].qbeg = bad.len[bad.chains[0].read];          /* outside its read */
        j5 = (bsw_c2a_job *)&g;
        CHECK(start_reads(ctx, p, ref, rd, bad, &j5) == BSW_E_INVAL && j5 == nullptr && strstr(bsw_last_error(ctx), "outside its read"), "a seed outside its read: %s", bsw_last_error(ctx));
        j5 = (bsw_c2a_job *)&g;
        CHECK(start_ref(ctx, p, ref, bad, &j5) == BSW_E_INVAL && j5 == nullptr, "a seed outside its read, by pointer");
        CHECK(bsw_inflight(ctx) == 0, "a failed start queued something");
        /* a flank beyond BSW_MAX_QLEN passes the plan and is the submit's BSW_E_LIMIT */
        {
            cwork lg;
            lg.reads.push_back(std::vector<uint8_t>(g.both.begin() + 2000, g.both.begin() + 2000 + 8300));
            lg.ptr.push_back(lg.reads[0].data());
            lg.len.push_back(8300);
            push_chain(lg, 0, {bsw_cseed{2000 + 8250, 8250, 30, 30, 0}}, 0, 0, 0, 0.f);
            bsw_reads *lrd = upload_reads(ctx, lg);
            j5 = (bsw_c2a_job *)&g;
            CHECK(start_reads(ctx, p, ref, lrd, lg, &j5) == BSW_E_LIMIT && j5 == nullptr && *bsw_last_error(ctx), "a flank of 8 250 bases: %s", bsw_last_error(ctx));
            j5 = (bsw_c2a_job *)&g;
            const int rc = start_ref(ctx, p, ref, lg, &j5);
            outs ol(lg);
            /* (the pointer form checks lengths on the slot threads: its BSW_E_LIMIT may come from the wait) */
            CHECK(rc == BSW_E_LIMIT ? j5 == nullptr : (rc == BSW_OK && j5 && finish(j5, ol) == BSW_E_LIMIT), "a flank of 8 250 bases by pointer -> %d", rc);
            CHECK(bsw_inflight(ctx) == 0 && bsw_reads_free(ctx, lrd) == BSW_OK, "the refused long seed left something behind");
        }
        CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "bsw_reads_free: %s", bsw_last_error(ctx));
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
    }
    CHECK(hipdbl::live_objects() == 0, "%zu HIP objects left alive", hipdbl::live_objects());
    printf("mixed ok\n");
    return 0;
}

/* ---- faults: call k of start .. finish of each form fails, for every k.
 * The counted window is the same calls in every run, whatever the threads' timing: ONE slot per device (streams = 1), so chunk c of a
 * ticket runs on the slot of device c mod 2 and nowhere else, and a warm-up of both forms in front of the window, so that the
 * pipeline is started, both slot threads have set their device and hold their lazily allocated staging when the counting begins.
 * (A slot thread's start-up hipSetDevice that fails is kept for the slot's NEXT chunk, whichever ticket that belongs to: inside the
 * window it would fail a later, unrelated job.  tests/hip_double/host_faults.cpp sweeps the pipeline's start.) ---- */
static int faults_mode()
{
    genome_t g;
    g.make(70001, 5);
    const bsw_params p = params_of(BSW_VARIANT_H);
    rng_t r0(31);
    cwork w;
    make_chains(w, g, r0, 60);
    expect(w, g, p, false);
    CHECK(w.seeds.size() >= 3 * 128, "the workload: %zu seeds make fewer than three chunks", w.seeds.size());
    sweep_t s;
    s.releases = {"hipFree", "hipHostFree", "hipGetLastError", "hipEventDestroy", "hipStreamDestroy", "hipHostUnregister"};      /* ignored by design */
    s.exact = true;
    s.min_failed = 30;
    fault_sweep(s, 2, [&](sweep_t &s) {
        const unsigned long long k = s.k;
        bsw_ctx *ctx = ctx_of(2, 128, BSW_RESULT_FULL, 4000, 1);
        bsw_ref *ref = upload(ctx, g);
        both_forms(ctx, p, ref, w, "the warm-up");
        bsw_reads *rd = upload_reads(ctx, w);
        s.arm();
        bsw_c2a_job *j[2] = {nullptr, nullptr};
        outs o0(w), o1(w);
        int rc[2];
        std::string text[2];
        /* one job after the other: with both in flight the order of the two slots' calls would be the threads' */
        for (int f = 0; f < 2; ++f) {
            rc[f] = f ? start_reads(ctx, p, ref, rd, w, &j[f]) : start_ref(ctx, p, ref, w, &j[f]);
            CHECK((rc[f] != 0) == (j[f] == nullptr), "k=%llu: start %d -> %d and job %p", k, f, rc[f], (void *)j[f]);
            if (!rc[f]) rc[f] = finish(j[f], f ? o1 : o0);
            if (rc[f]) text[f] = bsw_last_error(ctx);
        }
        s.judge({{rc[0], text[0]}, {rc[1], text[1]}});
        if (rc[0] == BSW_OK) same_c(o0, w, "a pointer job that reported success");
        if (rc[1] == BSW_OK) same_c(o1, w, "a reads job that reported success");
        if (k == 0) printf("faults: C = %llu\n", (unsigned long long)s.C);
        /* both jobs are gone: no ticket, the block is free, and what they pinned is released */
        CHECK(bsw_inflight(ctx) == 0, "k=%llu: tickets left", k);
        CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "k=%llu: bsw_reads_free after the jobs: %s", k, bsw_last_error(ctx));
        /* the context is alive: both forms once more, exact */
        both_forms(ctx, p, ref, w, "after the failure");
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
    });
    printf("faults: injection points visited = %llu, a job failed %llu times, ignored %llu\n", (unsigned long long)s.visited, (unsigned long long)s.failed, (unsigned long long)s.ignored);
    s.done();
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "forms") return forms_mode();
    if (mode == "mixed") return mixed_mode();
    if (mode == "faults") return faults_mode();
    fprintf(stderr, "usage: host_chain2aln forms | mixed | faults\n");
    return 2;
}
