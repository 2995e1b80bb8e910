/* host_sdp.cpp — the mem_sort_dedup_patch job (bsw_sdp_ref_start / _reads_start / _test / _finish / _job_stats: bsw_sdp_job.hip over
 * the engine of bsw_sdp.c and the patch tickets of bsw_cigar.hip) on the host-memory HIP stand-in, plain and under ASan / UBSan or
 * TSan (TEST INFRASTRUCTURE; tests/test_sdp_double_cpu.py builds it with its row in tests/_host_double_build.py and runs it).  A stand-alone
 * program: nothing is preloaded, no GPU is opened.
 *
 * What the job must hand back is the engine driven in-process, its pairs answered by a C restatement of mem_patch_reg over the
 * C oracle's ksw_global2 (as tests/hip_double/host_patch.cpp has it); the engine itself is checked against its sequential
 * restatement in tests/test_sdp_cpu.py.
 *
 *   host_sdp forms    both forms on 1, 2 and 3 devices, one driven by polls and one by finish; patch = 0; an empty job
 *   host_sdp mixed    two multi-round jobs beside an extension and a CIGAR ticket; the fifth start is refused and leaves no job
 *   host_sdp busy     a second thread takes the place a job's round has just left: test answers 0, finish BSW_E_BUSY with the job
 *                     intact; once a ticket is collected finish completes with the right bytes
 *   host_sdp faults   every HIP / launcher call of a start .. finish of each form fails in turn; the job is freed
 */
#include <atomic>
#include <climits>
#include "host_ref_patch.h"

/* ---- the workload: reads of 1 - 4 colinear pieces of the genome with a small indel between them, a region per piece (in a
 * scrambled order), sometimes a shadow of a region one base on (the redundancy test), sometimes a region of another rid ---- */
struct swork {
    std::vector<std::vector<uint8_t>> reads;
    std::vector<const uint8_t *> ptr;
    std::vector<int32_t> len;
    std::vector<bsw_sreg> regs;
    std::vector<uint64_t> start;
    std::vector<bsw_sreg> want;
    std::vector<uint64_t> want_start;
    bsw_sdp_stats want_st;
    std::vector<bsw_rd_ptask> round1;                 /* the engine's first needs: tickets for the tests to put beside a job */
};

static bsw_sreg sreg_of(int64_t rb, int64_t re, int qb, int qe, int score, uint32_t read, int rid, int w, rng_t &r)
{
    bsw_sreg s;
    memset(&s, 0, sizeof(s));
    s.rb = rb; s.re = re; s.qb = qb; s.qe = qe; s.score = s.truesc = score; s.w = w; s.seedcov = r.in(10, qe - qb); s.sub = r.below(40); s.csub = r.below(40);
    s.rid = rid; s.n_comp = 0; s.read = read; s.src = 0x5a5a5a5au;
    return s;
}

static void make_regions(swork &w, const genome_t &g, rng_t &r, size_t n_reads)
{
    const int64_t L = g.l_pac;
    w.start.assign(1, 0);
    for (size_t i = 0; i < n_reads; ++i) {
        const int n_seg = 1 + (int)(i % 4);
        const bool rev = r.below(2) == 1;
        int64_t x = (rev ? L : 0) + 300 + r.below((int)(L - 1000));
        std::vector<uint8_t> q;
        std::vector<bsw_sreg> mine;
        for (int k = 0; k < n_seg; ++k) {
            const int ln = r.in(45, 75);
            if (k) {
                const int d = r.below(6);
                if (r.below(2)) for (int t = 0; t < d; ++t) q.push_back((uint8_t)r.below(4));
                else x += d;
            }
            const int q0 = (int)q.size();
            q.insert(q.end(), g.both.begin() + x, g.both.begin() + x + ln);
            const int cl = k ? r.below(4) : 0, cr = k < n_seg - 1 ? r.below(4) : 0;
            mine.push_back(sreg_of(x + cl, x + ln - cr, q0 + cl, q0 + ln - cr, ln - cl - cr - r.in(8, 13), (uint32_t)i, 2, r.below(20), r));
            x += ln;
        }
        if (i % 7 == 3) {                            /* a shadow one base on, with the lower or the higher score */
            bsw_sreg s = mine[(size_t)r.below((int)mine.size())];
            s.rb -= 1; s.re += 1; s.score += i % 2 ? 5 : -5;
            mine.push_back(s);
        }
        if (i % 5 == 1) mine.push_back(sreg_of(mine[0].re - 20, mine[0].re + 10, 3, 33, 20, (uint32_t)i, 9, 2, r));
        for (size_t k = mine.size(); k > 1; --k) std::swap(mine[k - 1], mine[(size_t)r.below((int)k)]);
        w.regs.insert(w.regs.end(), mine.begin(), mine.end());
        w.start.push_back(w.regs.size());
        w.reads.push_back(q);
    }
    for (auto &q : w.reads) { w.ptr.push_back(q.data()); w.len.push_back((int32_t)q.size()); }
}

/* the engine in-process, its pairs answered by ref_patch */
static void expect(swork &w, const genome_t &g, const bsw_params &p, const bsw_sdp_opt *opt = nullptr)
{
    bsw_sdp_eng *e = nullptr;
    char text[400];
    const int rc = bsw_sdp_open(&p, opt, g.l_pac, w.regs.data(), w.regs.size(), w.start.data(), w.len.data(), w.len.size(), &e, text, sizeof(text));
    CHECK(rc == BSW_OK && e, "bsw_sdp_open -> %d (%s)", rc, text);
    for (int round = 0;; ++round) {
        const bsw_rd_ptask *t = nullptr;
        size_t n = 0;
        CHECK(bsw_sdp_needs(e, &t, &n) == BSW_OK, "bsw_sdp_needs");
        if (!n) break;
        if (!round) w.round1.assign(t, t + n);
        std::vector<bsw_presult> res(n);
        for (size_t k = 0; k < n; ++k) res[k] = ref_patch(p, g, w.ptr[t[k].read], t[k].a, t[k].b);
        CHECK(bsw_sdp_feed(e, res.data(), n) == BSW_OK, "bsw_sdp_feed");
    }
    w.want.assign(w.regs.size() + 1, bsw_sreg());
    w.want_start.assign(w.len.size() + 1, 0);
    size_t n = 0;
    CHECK(bsw_sdp_collect(e, w.want.data(), &n, w.want_start.data(), &w.want_st) == BSW_OK, "bsw_sdp_collect");
    w.want.resize(n);
    bsw_sdp_close(e);
}

struct outs {
    std::vector<bsw_sreg> regs;
    std::vector<uint64_t> start;
    size_t n = 77;
    bsw_sdp_stats st;
    explicit outs(const swork &w) : regs(w.regs.size() + 1), start(w.len.size() + 2, 0x5a5a)
    {
        memset(regs.data(), 0x5a, regs.size() * sizeof(bsw_sreg));
        memset(&st, 0, sizeof(st));
    }
};

static int finish(bsw_sdp_job *j, outs &o) { return bsw_sdp_finish(j, o.regs.data(), &o.n, o.start.data(), &o.st); }

static void same_s(const outs &o, const swork &w, const char *what)
{
    CHECK(o.n == w.want.size(), "%s: %zu regions, want %zu", what, o.n, w.want.size());
    for (size_t i = 0; i < o.n; ++i)
        if (memcmp(&o.regs[i], &w.want[i], sizeof(bsw_sreg)) != 0)
            CHECK(false, "%s: region %zu of %zu: src %u [%lld, %lld) score %d, want src %u [%lld, %lld) score %d", what, i, o.n, o.regs[i].src, (long long)o.regs[i].rb,
                  (long long)o.regs[i].re, o.regs[i].score, w.want[i].src, (long long)w.want[i].rb, (long long)w.want[i].re, w.want[i].score);
    CHECK(memcmp(o.start.data(), w.want_start.data(), (w.len.size() + 1) * sizeof(uint64_t)) == 0, "%s: out_start[] differs", what);
    CHECK(o.start[w.len.size() + 1] == 0x5a5a && o.regs[w.regs.size()].src == 0x5a5a5a5au, "%s: a write behind the caller's arrays", what);
    CHECK(memcmp(&o.st, &w.want_st, sizeof(bsw_sdp_stats)) == 0, "%s: the stats (rounds %llu / %llu, tasks %llu / %llu, merges %llu / %llu)", what,
          (unsigned long long)o.st.rounds, (unsigned long long)w.want_st.rounds, (unsigned long long)o.st.tasks, (unsigned long long)w.want_st.tasks,
          (unsigned long long)o.st.merges, (unsigned long long)w.want_st.merges);
}

static int start_ref(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, const swork &w, bsw_sdp_job **j, const bsw_sdp_opt *opt = nullptr)
{
    return bsw_sdp_ref_start(ctx, &p, opt, ref, w.ptr.data(), w.len.data(), w.len.size(), w.regs.data(), w.regs.size(), w.start.data(), j);
}
static int start_reads(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, bsw_reads *rd, const swork &w, bsw_sdp_job **j, const bsw_sdp_opt *opt = nullptr)
{
    return bsw_sdp_reads_start(ctx, &p, opt, ref, rd, w.regs.data(), w.regs.size(), w.start.data(), j);
}

/* both forms once on a context: the pointer job driven by polls alone, the reads job by finish */
static void both_forms(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, const swork &w, const char *what)
{
    bsw_sdp_job *j1 = nullptr, *j2 = nullptr;
    int rc = start_ref(ctx, p, ref, w, &j1);
    CHECK(rc == BSW_OK && j1, "%s: bsw_sdp_ref_start -> %d (%s)", what, rc, bsw_last_error(ctx));
    bsw_reads *rd = upload_reads(ctx, w);
    rc = start_reads(ctx, p, ref, rd, w, &j2);
    CHECK(rc == BSW_OK && j2, "%s: bsw_sdp_reads_start -> %d (%s)", what, rc, bsw_last_error(ctx));
    CHECK(bsw_inflight(ctx) == 2, "%s: %d submits in flight", what, bsw_inflight(ctx));
    bsw_sdp_stats st;
    CHECK(bsw_sdp_job_stats(j2, &st) == BSW_OK && st.rounds == 1 && st.tasks == w.want_st.tasks_first && st.regs_out == 0, "%s: the stats of a job in flight", what);
    CHECK(bsw_reads_free(ctx, rd) == BSW_E_BUSY, "%s: bsw_reads_free while the job holds the block", what);
    int t1 = 0;
    while ((t1 = bsw_sdp_test(j1)) == 0) std::this_thread::yield();
    CHECK(t1 == 1 && bsw_sdp_test(j1) == 1, "%s: bsw_sdp_test -> %d (%s)", what, t1, bsw_last_error(ctx));
    outs o1(w), o2(w);
    CHECK(finish(j2, o2) == BSW_OK, "%s: finish of the reads job: %s", what, bsw_last_error(ctx));
    CHECK(bsw_inflight(ctx) == 0, "%s: tickets left", what);
    CHECK(finish(j1, o1) == BSW_OK, "%s: finish of the pointer job: %s", what, bsw_last_error(ctx));
    CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "%s: bsw_reads_free after finish: %s", what, bsw_last_error(ctx));
    same_s(o1, w, what);
    same_s(o2, w, what);
}

static int forms_mode()
{
    genome_t g;
    g.make(70001, 5);
    const bsw_params p = default_params();
    size_t runs = 0;
    for (int D : {1, 2, 3}) {
        fresh(D);
        {
            rng_t r(50 + (uint64_t)D);
            swork w;
            make_regions(w, g, r, 240);
            expect(w, g, p);
            CHECK(w.want_st.rounds >= 3 && w.want_st.merges >= 100 && w.want_st.kills_p >= 3 && w.want_st.kills_q >= 3 && w.want_st.tasks > w.want_st.tasks_first,
                  "the workload: %llu rounds, %llu merges, %llu + %llu kills", (unsigned long long)w.want_st.rounds, (unsigned long long)w.want_st.merges,
                  (unsigned long long)w.want_st.kills_p, (unsigned long long)w.want_st.kills_q);
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, D, 256);
            bsw_ref *ref = upload(ctx, g);
            both_forms(ctx, p, ref, w, "both forms");
            /* patch = 0: complete at once, no ticket */
            bsw_sdp_opt o0;
            bsw_sdp_default_opt(&o0);
            o0.patch = 0;
            swork w0;
            w0.reads = w.reads; w0.regs = w.regs; w0.start = w.start; w0.len = w.len;
            for (auto &q : w0.reads) w0.ptr.push_back(q.data());
            expect(w0, g, p, &o0);
            CHECK(w0.want_st.rounds == 0 && w0.want_st.merges == 0 && w0.want.size() > w.want.size(), "patch = 0 in-process");
            bsw_sdp_job *j = nullptr;
            CHECK(start_ref(ctx, p, ref, w0, &j, &o0) == BSW_OK && j, "patch = 0: %s", bsw_last_error(ctx));
            CHECK(bsw_inflight(ctx) == 0 && bsw_sdp_test(j) == 1, "a patch = 0 job is complete");
            outs oz(w0);
            CHECK(finish(j, oz) == BSW_OK, "finish of a patch = 0 job");
            same_s(oz, w0, "patch = 0");
            /* an empty job */
            size_t n = 9;
            uint64_t start[1] = {0}, ostart[1] = {7};
            j = nullptr;
            CHECK(bsw_sdp_ref_start(ctx, &p, nullptr, ref, nullptr, nullptr, 0, nullptr, 0, start, &j) == BSW_OK && j, "an empty job: %s", bsw_last_error(ctx));
            CHECK(bsw_inflight(ctx) == 0 && bsw_sdp_test(j) == 1, "an empty job is complete");
            CHECK(bsw_sdp_finish(j, nullptr, &n, ostart, nullptr) == BSW_OK && n == 0 && ostart[0] == 0, "finish of an empty job");
            bsw_ref_free(ctx, ref);
            bsw_destroy(ctx);
            ++runs;
        }
        CHECK(hipdbl::live_objects() == 0, "%zu HIP objects left alive", hipdbl::live_objects());
    }
    printf("forms: %zu contexts\nforms ok\n", runs);
    return 0;
}

static std::vector<bsw_ctask> cigar_tasks(const genome_t &g)
{
    std::vector<bsw_ctask> ct;
    for (size_t i = 0; i < 64; ++i) {                /* exact pieces of the genome: the score is the length */
        bsw_ctask c;
        memset(&c, 0, sizeof(c));
        c.query = g.both.data() + 1000 + 200 * i; c.l_query = 100 + (int)i; c.w = 10; c.rb = 1000 + 200 * (int64_t)i; c.re = c.rb + c.l_query;
        c.min_score = INT_MIN; c.max_tries = 1;
        ct.push_back(c);
    }
    return ct;
}

static int mixed_mode()
{
    genome_t g;
    g.make(70001, 5);
    fresh(2);
    {
        const bsw_params p = default_params();
        rng_t r(8);
        swork w;
        make_regions(w, g, r, 200);
        expect(w, g, p);
        CHECK(w.want_st.rounds >= 3, "the workload: %llu rounds", (unsigned long long)w.want_st.rounds);
        workload we;
        make_workload(we, 1200, 150, 9, true);
        const std::vector<bsw_result> want_e = expected(p, we.tasks.data(), 1200);
        const std::vector<bsw_ctask> ct = cigar_tasks(g);
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256);
        bsw_ref *ref = upload(ctx, g);
        bsw_reads *rd = upload_reads(ctx, w);
        std::vector<bsw_result> eo(1200);
        std::vector<bsw_cresult> co(ct.size());
        bsw_ticket te = 0, tc = 0;
        bsw_sdp_job *j1 = nullptr, *j2 = nullptr, *j5 = (bsw_sdp_job *)&g;
        CHECK(bsw_cigar_ref_submit_t(ctx, &p, ref, ct.data(), ct.size(), 64, nullptr, 0, nullptr, co.data(), &tc) == BSW_OK, "CIGAR: %s", bsw_last_error(ctx));
        CHECK(start_ref(ctx, p, ref, w, &j1) == BSW_OK && j1, "the pointer job: %s", bsw_last_error(ctx));
        CHECK(bsw_submit_t(ctx, &p, we.tasks.data(), 1200, eo.data(), &te) == BSW_OK, "extension: %s", bsw_last_error(ctx));
        CHECK(start_reads(ctx, p, ref, rd, w, &j2) == BSW_OK && j2, "the reads job: %s", bsw_last_error(ctx));
        CHECK(bsw_inflight(ctx) == 4, "four submits");
        CHECK(start_ref(ctx, p, ref, w, &j5) == BSW_E_BUSY && j5 == nullptr && strstr(bsw_last_error(ctx), "BSW_MAX_INFLIGHT"), "the fifth submit as a pointer job");
        j5 = (bsw_sdp_job *)&g;
        CHECK(start_reads(ctx, p, ref, rd, w, &j5) == BSW_E_BUSY && j5 == nullptr, "the fifth submit as a reads job");
        CHECK(bsw_inflight(ctx) == 4, "a refused start changed the tickets");       /* (what it allocated: the leak check, and live_objects() at the end) */
        outs o5(w);
        CHECK(finish(j5, o5) == BSW_E_INVAL && bsw_sdp_test(j5) == BSW_E_INVAL && bsw_sdp_job_stats(j5, &o5.st) == BSW_E_INVAL, "the calls on no job");
        CHECK(o5.regs[0].src == 0x5a5a5a5au, "finish of no job wrote regions");
        outs o1(w), o2(w);
        CHECK(finish(j2, o2) == BSW_OK, "the reads job: %s", bsw_last_error(ctx));
        CHECK(bsw_wait_ticket(ctx, tc) == BSW_OK, "the CIGAR ticket: %s", bsw_last_error(ctx));
        CHECK(finish(j1, o1) == BSW_OK, "the pointer job: %s", bsw_last_error(ctx));
        CHECK(bsw_wait_ticket(ctx, te) == BSW_OK, "the extension ticket: %s", bsw_last_error(ctx));
        CHECK(bsw_inflight(ctx) == 0, "tickets left");
        same_s(o1, w, "the pointer job beside other tickets");
        same_s(o2, w, "the reads job beside other tickets");
        CHECK(memcmp(eo.data(), want_e.data(), 1200 * sizeof(bsw_result)) == 0, "the extension ticket beside the jobs");
        for (size_t k = 0; k < ct.size(); ++k) CHECK(co[k].status == 0 && co[k].score == ct[k].l_query, "CIGAR task %zu: score %d", k, co[k].score);
        /* a start that fails in open: the code, a text that names the region, no job, nothing queued */
        swork bad;
        bad.reads = w.reads; bad.ptr = w.ptr; bad.len = w.len; bad.regs = w.regs; bad.start = w.start;
        bad.regs[5].qe = bad.regs[5].qb;
        j5 = (bsw_sdp_job *)&g;
        CHECK(start_reads(ctx, p, ref, rd, bad, &j5) == BSW_E_INVAL && j5 == nullptr && strstr(bsw_last_error(ctx), "region 5"), "an excluded region on input: %s", bsw_last_error(ctx));
        j5 = (bsw_sdp_job *)&g;
        CHECK(start_ref(ctx, p, ref, bad, &j5) == BSW_E_INVAL && j5 == nullptr, "an excluded region on input, by pointer");
        CHECK(bsw_inflight(ctx) == 0, "a failed start queued something");
        CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "bsw_reads_free: %s", bsw_last_error(ctx));
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
    }
    CHECK(hipdbl::live_objects() == 0, "%zu HIP objects left alive", hipdbl::live_objects());
    printf("mixed ok\n");
    return 0;
}

/* ---- busy: on ONE thread a follow-up round always finds the place its own ticket has just left, so the place is taken by a
 * second thread that submits as soon as it can.  Whether it wins the race is timing: the scenario is repeated until it has. ---- */
static int busy_mode()
{
    genome_t g;
    g.make(70001, 5);
    const bsw_params p = default_params();
    rng_t r(77);
    swork w;
    make_regions(w, g, r, 400);
    expect(w, g, p);
    CHECK(w.want_st.rounds >= 3 && w.round1.size() >= 64, "the workload: %llu rounds", (unsigned long long)w.want_st.rounds);
    std::vector<bsw_ptask> fill(32);
    for (size_t k = 0; k < fill.size(); ++k) {
        const bsw_rd_ptask &t = w.round1[k];
        fill[k].query = w.ptr[t.read]; fill[k].l_query = w.len[t.read]; fill[k]._pad = 0; fill[k].a = t.a; fill[k].b = t.b;
    }
    int seen = 0, attempts = 0;
    for (; attempts < 200 && !seen; ++attempts) {
        fresh(1);
        {
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256);
            bsw_ref *ref = upload(ctx, g);
            bsw_sdp_job *j = nullptr;
            CHECK(start_ref(ctx, p, ref, w, &j) == BSW_OK && j, "the job: %s", bsw_last_error(ctx));
            std::vector<bsw_presult> fo[4];
            bsw_ticket tf[4] = {0, 0, 0, 0};
            for (int k = 0; k < 3; ++k) {
                fo[k].resize(fill.size());
                CHECK(bsw_patch_ref_submit_t(ctx, &p, ref, fill.data(), fill.size(), fo[k].data(), &tf[k]) == BSW_OK, "ticket %d: %s", k, bsw_last_error(ctx));
            }
            CHECK(bsw_inflight(ctx) == 4, "four submits");
            fo[3].resize(fill.size());
            std::atomic<bool> stop{false}, took{false};
            std::thread other([&]() {
                while (!stop.load()) {
                    const int rc = bsw_patch_ref_submit_t(ctx, &p, ref, fill.data(), fill.size(), fo[3].data(), &tf[3]);
                    if (rc == BSW_OK) { took.store(true); return; }
                    CHECK(rc == BSW_E_BUSY, "the other thread's submit -> %d", rc);
                }
            });
            outs o(w);
            int rc = finish(j, o);
            stop.store(true);
            other.join();
            if (rc == BSW_E_BUSY) {
                seen = 1;
                CHECK(took.load() && bsw_inflight(ctx) == 4, "BSW_E_BUSY with %d submits in flight", bsw_inflight(ctx));
                CHECK(o.n == 0 && o.regs[0].src == 0x5a5a5a5au, "a finish that answered BSW_E_BUSY wrote regions");
                CHECK(bsw_sdp_test(j) == 0, "test with the four places taken");
                CHECK(finish(j, o) == BSW_E_BUSY, "finish with the four places taken, again");
                bsw_sdp_stats st;
                CHECK(bsw_sdp_job_stats(j, &st) == BSW_OK && st.rounds >= 2, "the job is intact");
                CHECK(bsw_wait_ticket(ctx, tf[0]) == BSW_OK, "a ticket: %s", bsw_last_error(ctx));
                tf[0] = 0;
                rc = finish(j, o);
            }
            CHECK(rc == BSW_OK, "finish: %d (%s)", rc, bsw_last_error(ctx));
            same_s(o, w, "a job whose follow-up round found no place");
            for (int k = 0; k < 4; ++k)
                if (tf[k]) CHECK(bsw_wait_ticket(ctx, tf[k]) == BSW_OK, "ticket %d: %s", k, bsw_last_error(ctx));
            CHECK(bsw_inflight(ctx) == 0, "tickets left");
            bsw_ref_free(ctx, ref);
            bsw_destroy(ctx);
        }
        CHECK(hipdbl::live_objects() == 0, "%zu HIP objects left alive", hipdbl::live_objects());
    }
    CHECK(seen, "in %d attempts the other thread never took the place", attempts);
    printf("busy: seen after %d attempts\nbusy ok\n", attempts);
    return 0;
}

/* ---- faults: call k of start .. finish of each form fails, for every k.  One slot per device (streams = 1) and a warm-up of both
 * forms in front of the window, as tests/hip_double/host_chain2aln.cpp explains. ---- */
static int faults_mode()
{
    genome_t g;
    g.make(70001, 5);
    const bsw_params p = default_params();
    rng_t r0(31);
    swork w;
    make_regions(w, g, r0, 60);
    expect(w, g, p);
    CHECK(w.want_st.rounds >= 3, "the workload: %llu rounds", (unsigned long long)w.want_st.rounds);
    sweep_t s;
    /* releases whose code is ignored by design; a slot's hipSetDevice when it gets no chunk */
    s.releases = {"hipSetDevice", "hipFree", "hipHostFree", "hipGetLastError", "hipEventDestroy", "hipStreamDestroy", "hipHostUnregister", "hipEventQuery"};
    s.min_visited = 60; s.min_failed = 50;
    fault_sweep(s, 2, [&](sweep_t &s) {
        const unsigned long long k = s.k;
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 128, 1, 4000);
        bsw_ref *ref = upload(ctx, g);
        both_forms(ctx, p, ref, w, "the warm-up");
        bsw_reads *rd = upload_reads(ctx, w);
        s.arm();
        bsw_sdp_job *j[2] = {nullptr, nullptr};
        outs o0(w), o1(w);
        int rc[2];
        std::string text[2];
        for (int f = 0; f < 2; ++f) {            /* one job after the other: with both in flight the order of the slots' calls would be the threads' */
            rc[f] = f ? start_reads(ctx, p, ref, rd, w, &j[f]) : start_ref(ctx, p, ref, w, &j[f]);
            CHECK((rc[f] != 0) == (j[f] == nullptr), "k=%llu: start %d -> %d and job %p", k, f, rc[f], (void *)j[f]);
            if (!rc[f]) rc[f] = finish(j[f], f ? o1 : o0);
            CHECK(rc[f] != BSW_E_BUSY, "k=%llu: BSW_E_BUSY on one thread", k);
            if (rc[f]) text[f] = bsw_last_error(ctx);
        }
        s.judge({{rc[0], text[0]}, {rc[1], text[1]}});
        if (rc[0] == BSW_OK) same_s(o0, w, "a pointer job that reported success");
        if (rc[1] == BSW_OK) same_s(o1, w, "a reads job that reported success");
        if (k == 0) printf("faults: C = %llu\n", (unsigned long long)s.C);
        /* both jobs are gone: no ticket, the block is free, and what they pinned is released */
        CHECK(bsw_inflight(ctx) == 0, "k=%llu: tickets left", k);
        CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "k=%llu: bsw_reads_free after the jobs: %s", k, bsw_last_error(ctx));
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
    if (mode == "busy") return busy_mode();
    if (mode == "faults") return faults_mode();
    fprintf(stderr, "usage: host_sdp forms | mixed | busy | faults\n");
    return 2;
}
