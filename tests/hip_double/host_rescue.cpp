/* host_rescue.cpp — the mate-rescue job (bsw_rescue_ref_start / _reads_start / _test / _finish / _job_stats: bsw_rescue_job.hip over
 * the engine of bsw_rescue.c, the pass of bsw_sdp.c and the rescue tickets of bsw_matesw.hip) on the host-memory HIP stand-in, plain
 * and under ASan / UBSan or TSan (TEST INFRASTRUCTURE; tests/test_rescue_double_cpu.py registers its row in
 * tests/_host_double_build.py's table and runs it).  A stand-alone program: nothing is preloaded, no GPU is opened.
 *
 * What the job must hand back is the engine driven in-process, its windows answered by the synchronous bsw_matesw_ref_batch on a
 * one-device context of its own; the engine itself is checked against its sequential restatement in tests/test_rescue_cpu.py.
 *
 *   host_rescue forms    both forms on 1, 2 and 3 devices, one driven by polls and one by finish; all orientations failed; an empty job
 *   host_rescue mixed    two multi-round jobs beside an extension and a CIGAR ticket; the fifth start is refused and leaves no job
 *   host_rescue busy     a second thread takes the place a job's round has just left: test answers 0, finish BSW_E_BUSY with the job
 *                        intact; once a ticket is collected finish completes with the right bytes
 *   host_rescue faults   every HIP / launcher call of a start .. finish of each form fails in turn; the job is freed
 */
#include <atomic>
#include <climits>
#include "host_ref_patch.h"

static const int LOW = 100, HIGH = 500, N = 100;

/* ---- the workload: FR pairs of 100 bases in three contigs: proper pairs, mates without a region, two anchors three bases apart,
 * junk mates, and the late case of tests/_rescue_ref.py (a copy of the mate planted 300 bases left of the first anchor), which
 * costs a second round ---- */
struct rwork {
    genome_t g;
    std::vector<bsw_contig> contigs;
    std::vector<std::vector<uint8_t>> reads;
    std::vector<const uint8_t *> ptr;
    std::vector<int32_t> len;
    std::vector<bsw_sreg> regs;
    std::vector<uint64_t> start;
    bsw_rescue_opt opt;
    std::vector<bsw_sreg> want;
    std::vector<uint64_t> want_start;
    std::vector<int32_t> want_n_sw;
    bsw_rescue_stats want_st;
    size_t cap = 0;
    std::vector<bsw_mtask> round1;                    /* the engine's first needs: tickets for the tests to put beside a job */
};

static bsw_sreg reg_at(int64_t c, int n, int qb, int score, uint32_t read, int rid)
{
    bsw_sreg s;
    memset(&s, 0, sizeof(s));
    s.rb = c; s.re = c + n; s.qb = qb; s.qe = qb + n; s.score = s.truesc = score; s.seedcov = n / 2; s.rid = rid; s.read = read; s.src = 0x5a5a5a5au;
    return s;
}

static void make_pairs(rwork &w, uint64_t seed, size_t n_pairs)
{
    const int64_t L = 70001;
    const int64_t off[3] = {0, 25000, 45001}, ln[3] = {25000, 20001, 25000};
    rng_t r(seed);
    w.g.make(L, 5);
    const size_t n_late = (n_pairs + 4) / 5;
    std::vector<uint8_t> &b = w.g.both;
    for (size_t k = 0; k < n_late; ++k) {             /* the planted copies, then the reverse strand and the pac again */
        const int64_t x1 = 1500 + 1200 * (int64_t)(k % 18) + (k >= 18 ? 45001 : 0);
        for (int i = 0; i < N; ++i) b[(size_t)(x1 - 300 + i)] = b[(size_t)(x1 + 6 + i)];
    }
    for (int64_t x = L; x < 2 * L; ++x) b[(size_t)x] = (uint8_t)(3 - b[(size_t)(2 * L - 1 - x)]);
    w.g.pac.assign((size_t)((L + 3) >> 2), 0);
    for (int64_t x = 0; x < L; ++x) w.g.pac[(size_t)(x >> 2)] |= (uint8_t)(b[(size_t)x] << ((~x & 3) << 1));
    for (int k = 0; k < 3; ++k) w.contigs.push_back(bsw_contig{off[k], ln[k]});
    bsw_rescue_default_opt(&w.opt);
    w.opt.low[1] = LOW; w.opt.high[1] = HIGH; w.opt.failed[1] = 0;
    auto rid_of = [&](int64_t c) { const int64_t f = c < L ? c : 2 * L - 1 - c; return f < off[1] ? 0 : f < off[2] ? 1 : 2; };
    auto at = [&](int64_t c) { return std::vector<uint8_t>(b.begin() + c, b.begin() + c + N); };
    auto mate_of = [&](int64_t x, int dist) { return 2 * L - 1 - (x + dist); };
    w.start.assign(1, 0);
    size_t late = 0;
    for (size_t i = 0; i < n_pairs; ++i) {
        const uint32_t ra = (uint32_t)(2 * i), rm = ra + 1;
        const int kind = (int)(i % 5);
        std::vector<bsw_sreg> a, m;
        std::vector<uint8_t> qa, qm;
        if (kind == 3) {
            const int64_t x1 = 1500 + 1200 * (int64_t)(late % 18) + (late >= 18 ? 45001 : 0), mc = mate_of(x1, 105);
            ++late;
            qa = at(x1); qm = at(mc);
            a.push_back(reg_at(x1, N, 0, N, ra, rid_of(x1)));
            a.push_back(reg_at(x1 - 400, N, 0, 90, ra, rid_of(x1)));
            m.push_back(reg_at(mc + 10, 40, 10, 40, rm, rid_of(mc)));
        } else {
            const int c = r.below(3);
            const int64_t f = off[c] + 700 + r.below((int)ln[c] - 1500);
            const int64_t x = r.below(2) ? f : 2 * L - f - N, mc = mate_of(x, r.in(LOW + 5, HIGH - 5));
            qa = at(x); qm = at(mc);
            for (int s = r.below(4); s > 0; --s) qm[(size_t)r.below(N)] = (uint8_t)r.below(4);
            a.push_back(reg_at(x, N, 0, N, ra, c));
            if (kind == 0) m.push_back(reg_at(mc, N, 0, 90, rm, c));
            if (kind == 2) a.push_back(reg_at(x + 3, N - 3, 3, 90, ra, c));
            if (kind == 4) for (auto &q : qm) q = (uint8_t)r.below(4);
        }
        w.regs.insert(w.regs.end(), a.begin(), a.end());
        w.start.push_back(w.regs.size());
        w.regs.insert(w.regs.end(), m.begin(), m.end());
        w.start.push_back(w.regs.size());
        w.reads.push_back(qa);
        w.reads.push_back(qm);
    }
    for (auto &q : w.reads) { w.ptr.push_back(q.data()); w.len.push_back((int32_t)q.size()); }
}

/* the engine in-process, its windows answered by the synchronous call on a context of its own */
static void expect(rwork &w, const bsw_params &p, const bsw_rescue_opt *opt = nullptr)
{
    bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256);
    bsw_ref *ref = upload(ctx, w.g);
    bsw_rescue_eng *e = nullptr;
    char text[400];
    const int rc = bsw_rescue_open(&p, opt ? opt : &w.opt, w.g.l_pac, w.contigs.data(), w.contigs.size(), w.regs.data(), w.regs.size(), w.start.data(), w.len.data(),
                                   w.len.size(), &e, text, sizeof(text));
    CHECK(rc == BSW_OK && e, "bsw_rescue_open -> %d (%s)", rc, text);
    for (int round = 0;; ++round) {
        const bsw_rd_mtask *t = nullptr;
        size_t n = 0;
        CHECK(bsw_rescue_needs(e, &t, &n) == BSW_OK, "bsw_rescue_needs");
        if (!n) break;
        std::vector<bsw_mtask> mt(n);
        for (size_t k = 0; k < n; ++k) {
            mt[k].mate = w.ptr[t[k].read]; mt[k].l_ms = w.len[t[k].read]; mt[k].is_rev = t[k].is_rev; mt[k].rb = t[k].rb; mt[k].re = t[k].re;
            mt[k].xtra = t[k].xtra; mt[k].min_score = t[k].min_score;
        }
        if (!round) w.round1 = mt;
        std::vector<bsw_mresult> res(n);
        CHECK(bsw_matesw_ref_batch(ctx, &p, ref, mt.data(), n, res.data()) == BSW_OK, "bsw_matesw_ref_batch: %s", bsw_last_error(ctx));
        CHECK(bsw_rescue_feed(e, res.data(), n) == BSW_OK, "bsw_rescue_feed");
    }
    w.cap = bsw_rescue_out_capacity(e);
    w.want.assign(w.cap + 1, bsw_sreg());
    w.want_start.assign(w.len.size() + 1, 0);
    w.want_n_sw.assign(w.len.size() / 2 + 1, 0);
    size_t n = 0;
    CHECK(bsw_rescue_collect(e, w.want.data(), &n, w.want_start.data(), w.want_n_sw.data(), &w.want_st) == BSW_OK, "bsw_rescue_collect");
    w.want.resize(n);
    w.want_n_sw.resize(w.len.size() / 2);
    bsw_rescue_close(e);
    bsw_ref_free(ctx, ref);
    bsw_destroy(ctx);
}

struct outs {
    std::vector<bsw_sreg> regs;
    std::vector<uint64_t> start;
    std::vector<int32_t> n_sw;
    size_t n = 77;
    bsw_rescue_stats st;
    explicit outs(const rwork &w) : regs(w.cap + 1), start(w.len.size() + 2, 0x5a5a), n_sw(w.len.size() / 2 + 1, 0x5a5a)
    {
        memset(regs.data(), 0x5a, regs.size() * sizeof(bsw_sreg));
        memset(&st, 0, sizeof(st));
    }
};

static int finish(bsw_rescue_job *j, outs &o) { return bsw_rescue_finish(j, o.regs.data(), o.regs.size() - 1, &o.n, o.start.data(), o.n_sw.data(), &o.st); }

static void same_r(const outs &o, const rwork &w, const char *what)
{
    CHECK(o.n == w.want.size(), "%s: %zu regions, want %zu", what, o.n, w.want.size());
    for (size_t i = 0; i < o.n; ++i)
        if (memcmp(&o.regs[i], &w.want[i], sizeof(bsw_sreg)) != 0)
            CHECK(false, "%s: region %zu of %zu: src %u [%lld, %lld) score %d, want src %u [%lld, %lld) score %d", what, i, o.n, o.regs[i].src, (long long)o.regs[i].rb,
                  (long long)o.regs[i].re, o.regs[i].score, w.want[i].src, (long long)w.want[i].rb, (long long)w.want[i].re, w.want[i].score);
    CHECK(memcmp(o.start.data(), w.want_start.data(), (w.len.size() + 1) * sizeof(uint64_t)) == 0, "%s: out_start[] differs", what);
    CHECK(w.want_n_sw.empty() || memcmp(o.n_sw.data(), w.want_n_sw.data(), w.want_n_sw.size() * sizeof(int32_t)) == 0, "%s: n_sw[] differs", what);
    CHECK(o.start[w.len.size() + 1] == 0x5a5a && o.n_sw[w.len.size() / 2] == 0x5a5a && o.regs[w.cap].src == 0x5a5a5a5au, "%s: a write behind the caller's arrays", what);
    CHECK(memcmp(&o.st, &w.want_st, sizeof(bsw_rescue_stats)) == 0, "%s: the stats (rounds %llu / %llu, tasks %llu / %llu, pushed %llu / %llu)", what,
          (unsigned long long)o.st.rounds, (unsigned long long)w.want_st.rounds, (unsigned long long)o.st.tasks, (unsigned long long)w.want_st.tasks,
          (unsigned long long)o.st.pushed, (unsigned long long)w.want_st.pushed);
}

static int start_ref(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, const rwork &w, bsw_rescue_job **j, const bsw_rescue_opt *opt = nullptr)
{
    return bsw_rescue_ref_start(ctx, &p, opt ? opt : &w.opt, ref, w.ptr.data(), w.len.data(), w.len.size(), w.contigs.data(), w.contigs.size(), w.regs.data(),
                                w.regs.size(), w.start.data(), j);
}
static int start_reads(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, bsw_reads *rd, const rwork &w, bsw_rescue_job **j, const bsw_rescue_opt *opt = nullptr)
{
    return bsw_rescue_reads_start(ctx, &p, opt ? opt : &w.opt, ref, rd, w.contigs.data(), w.contigs.size(), w.regs.data(), w.regs.size(), w.start.data(), j);
}

/* both forms once on a context: the pointer job driven by polls alone, the reads job by finish */
static void both_forms(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, const rwork &w, const char *what)
{
    bsw_rescue_job *j1 = nullptr, *j2 = nullptr;
    int rc = start_ref(ctx, p, ref, w, &j1);
    CHECK(rc == BSW_OK && j1, "%s: bsw_rescue_ref_start -> %d (%s)", what, rc, bsw_last_error(ctx));
    bsw_reads *rd = upload_reads(ctx, w);
    rc = start_reads(ctx, p, ref, rd, w, &j2);
    CHECK(rc == BSW_OK && j2, "%s: bsw_rescue_reads_start -> %d (%s)", what, rc, bsw_last_error(ctx));
    CHECK(bsw_inflight(ctx) == 2, "%s: %d submits in flight", what, bsw_inflight(ctx));
    bsw_rescue_stats st;
    CHECK(bsw_rescue_job_stats(j2, &st) == BSW_OK && st.rounds == 1 && st.tasks == w.want_st.tasks_first && st.regs_out == 0, "%s: the stats of a job in flight", what);
    CHECK(bsw_rescue_job_out_capacity(j2) == w.cap, "%s: the job's capacity", what);
    CHECK(bsw_reads_free(ctx, rd) == BSW_E_BUSY, "%s: bsw_reads_free while the job holds the block", what);
    int t1 = 0;
    while ((t1 = bsw_rescue_test(j1)) == 0) std::this_thread::yield();
    CHECK(t1 == 1 && bsw_rescue_test(j1) == 1, "%s: bsw_rescue_test -> %d (%s)", what, t1, bsw_last_error(ctx));
    outs o1(w), o2(w);
    CHECK(finish(j2, o2) == BSW_OK, "%s: finish of the reads job: %s", what, bsw_last_error(ctx));
    CHECK(bsw_inflight(ctx) == 0, "%s: tickets left", what);
    CHECK(finish(j1, o1) == BSW_OK, "%s: finish of the pointer job: %s", what, bsw_last_error(ctx));
    CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "%s: bsw_reads_free after finish: %s", what, bsw_last_error(ctx));
    same_r(o1, w, what);
    same_r(o2, w, what);
}

static void check_workload(const rwork &w)
{
    CHECK(w.want_st.rounds == 2 && w.want_st.late >= 3 && w.want_st.pushed >= 20 && w.want_st.tasks_first > w.want_st.alns_bwa - w.want_st.late,
          "the workload: %llu rounds, %llu late, %llu pushed, %llu tasks in round 1, %llu alignments", (unsigned long long)w.want_st.rounds,
          (unsigned long long)w.want_st.late, (unsigned long long)w.want_st.pushed, (unsigned long long)w.want_st.tasks_first, (unsigned long long)w.want_st.alns_bwa);
}

static int forms_mode()
{
    const bsw_params p = default_params();
    size_t runs = 0;
    for (int D : {1, 2, 3}) {
        fresh(D);
        {
            rwork w;
            make_pairs(w, 50 + (uint64_t)D, 120);
            expect(w, p);
            check_workload(w);
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, D, 256);
            bsw_ref *ref = upload(ctx, w.g);
            both_forms(ctx, p, ref, w, "both forms");
            /* every orientation failed (the defaults): complete at once, no ticket, the input back */
            bsw_rescue_opt o0;
            bsw_rescue_default_opt(&o0);
            bsw_rescue_job *j = nullptr;
            CHECK(start_ref(ctx, p, ref, w, &j, &o0) == BSW_OK && j, "all failed: %s", bsw_last_error(ctx));
            CHECK(bsw_inflight(ctx) == 0 && bsw_rescue_test(j) == 1, "a job with nothing to ask is complete");
            outs oz(w);
            CHECK(finish(j, oz) == BSW_OK && oz.n == w.regs.size() && oz.st.tasks == 0 && oz.st.regs_out == w.regs.size(), "finish of a job with nothing to ask");
            for (size_t k = 0; k < oz.n; ++k)
                CHECK(oz.regs[k].rb == w.regs[k].rb && oz.regs[k].score == w.regs[k].score && oz.regs[k].src == k && oz.regs[k].n_comp == w.regs[k].n_comp, "region %zu came back changed", k);
            /* finish with too little room: BSW_E_INVAL, the job is freed all the same */
            j = nullptr;
            CHECK(start_ref(ctx, p, ref, w, &j) == BSW_OK && j, "the job: %s", bsw_last_error(ctx));
            outs os(w);
            CHECK(bsw_rescue_finish(j, os.regs.data(), 3, &os.n, os.start.data(), os.n_sw.data(), &os.st) == BSW_E_INVAL && os.n == 0 && strstr(bsw_last_error(ctx), "room for 3"),
                  "finish with room for 3 regions: %s", bsw_last_error(ctx));
            CHECK(os.regs[0].src == 0x5a5a5a5au && bsw_inflight(ctx) == 0, "a refused finish wrote regions or left a ticket");
            /* an empty job */
            size_t n = 9;
            uint64_t start[1] = {0}, ostart[1] = {7};
            j = nullptr;
            CHECK(bsw_rescue_ref_start(ctx, &p, &w.opt, ref, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, start, &j) == BSW_OK && j, "an empty job: %s", bsw_last_error(ctx));
            CHECK(bsw_inflight(ctx) == 0 && bsw_rescue_test(j) == 1, "an empty job is complete");
            CHECK(bsw_rescue_finish(j, nullptr, 0, &n, ostart, nullptr, nullptr) == BSW_OK && n == 0 && ostart[0] == 0, "finish of an empty job");
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
    fresh(2);
    {
        const bsw_params p = default_params();
        rwork w;
        make_pairs(w, 8, 100);
        expect(w, p);
        check_workload(w);
        workload we;
        make_workload(we, 1200, 150, 9, true);
        const std::vector<bsw_result> want_e = expected(p, we.tasks.data(), 1200);
        const std::vector<bsw_ctask> ct = cigar_tasks(w.g);
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256);
        bsw_ref *ref = upload(ctx, w.g);
        bsw_reads *rd = upload_reads(ctx, w);
        std::vector<bsw_result> eo(1200);
        std::vector<bsw_cresult> co(ct.size());
        bsw_ticket te = 0, tc = 0;
        bsw_rescue_job *j1 = nullptr, *j2 = nullptr, *j5 = (bsw_rescue_job *)&w;
        CHECK(bsw_cigar_ref_submit_t(ctx, &p, ref, ct.data(), ct.size(), 64, nullptr, 0, nullptr, co.data(), &tc) == BSW_OK, "CIGAR: %s", bsw_last_error(ctx));
        CHECK(start_ref(ctx, p, ref, w, &j1) == BSW_OK && j1, "the pointer job: %s", bsw_last_error(ctx));
        CHECK(bsw_submit_t(ctx, &p, we.tasks.data(), 1200, eo.data(), &te) == BSW_OK, "extension: %s", bsw_last_error(ctx));
        CHECK(start_reads(ctx, p, ref, rd, w, &j2) == BSW_OK && j2, "the reads job: %s", bsw_last_error(ctx));
        CHECK(bsw_inflight(ctx) == 4, "four submits");
        CHECK(start_ref(ctx, p, ref, w, &j5) == BSW_E_BUSY && j5 == nullptr && strstr(bsw_last_error(ctx), "BSW_MAX_INFLIGHT"), "the fifth submit as a pointer job");
        j5 = (bsw_rescue_job *)&w;
        CHECK(start_reads(ctx, p, ref, rd, w, &j5) == BSW_E_BUSY && j5 == nullptr, "the fifth submit as a reads job");
        CHECK(bsw_inflight(ctx) == 4, "a refused start changed the tickets");
        outs o5(w);
        CHECK(finish(j5, o5) == BSW_E_INVAL && bsw_rescue_test(j5) == BSW_E_INVAL && bsw_rescue_job_stats(j5, &o5.st) == BSW_E_INVAL, "the calls on no job");
        CHECK(o5.regs[0].src == 0x5a5a5a5au, "finish of no job wrote regions");
        outs o1(w), o2(w);
        CHECK(finish(j2, o2) == BSW_OK, "the reads job: %s", bsw_last_error(ctx));
        CHECK(bsw_wait_ticket(ctx, tc) == BSW_OK, "the CIGAR ticket: %s", bsw_last_error(ctx));
        CHECK(finish(j1, o1) == BSW_OK, "the pointer job: %s", bsw_last_error(ctx));
        CHECK(bsw_wait_ticket(ctx, te) == BSW_OK, "the extension ticket: %s", bsw_last_error(ctx));
        CHECK(bsw_inflight(ctx) == 0, "tickets left");
        same_r(o1, w, "the pointer job beside other tickets");
        same_r(o2, w, "the reads job beside other tickets");
        CHECK(memcmp(eo.data(), want_e.data(), 1200 * sizeof(bsw_result)) == 0, "the extension ticket beside the jobs");
        for (size_t k = 0; k < ct.size(); ++k) CHECK(co[k].status == 0 && co[k].score == ct[k].l_query, "CIGAR task %zu: score %d", k, co[k].score);
        /* a start that fails in open: the code, a text that names the region, no job, nothing queued */
        std::vector<bsw_sreg> good = w.regs;
        w.regs[5].rid = 7;
        j5 = (bsw_rescue_job *)&w;
        CHECK(start_reads(ctx, p, ref, rd, w, &j5) == BSW_E_INVAL && j5 == nullptr && strstr(bsw_last_error(ctx), "region 5"), "a rid of no contig: %s", bsw_last_error(ctx));
        j5 = (bsw_rescue_job *)&w;
        CHECK(start_ref(ctx, p, ref, w, &j5) == BSW_E_INVAL && j5 == nullptr, "a rid of no contig, by pointer");
        w.regs = good;
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
    const bsw_params p = default_params();
    rwork w;
    fresh(1);
    make_pairs(w, 77, 160);
    expect(w, p);
    check_workload(w);
    CHECK(w.round1.size() >= 64, "round 1 has %zu tasks", w.round1.size());
    const std::vector<bsw_mtask> fill(w.round1.begin(), w.round1.begin() + 32);
    int seen = 0, attempts = 0;
    for (; attempts < 200 && !seen; ++attempts) {
        fresh(1);
        {
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256);
            bsw_ref *ref = upload(ctx, w.g);
            bsw_rescue_job *j = nullptr;
            CHECK(start_ref(ctx, p, ref, w, &j) == BSW_OK && j, "the job: %s", bsw_last_error(ctx));
            std::vector<bsw_mresult> fo[4];
            bsw_ticket tf[4] = {0, 0, 0, 0};
            for (int k = 0; k < 3; ++k) {
                fo[k].resize(fill.size());
                CHECK(bsw_matesw_ref_submit_t(ctx, &p, ref, fill.data(), fill.size(), fo[k].data(), &tf[k]) == BSW_OK, "ticket %d: %s", k, bsw_last_error(ctx));
            }
            CHECK(bsw_inflight(ctx) == 4, "four submits");
            fo[3].resize(fill.size());
            std::atomic<bool> stop{false}, took{false};
            std::thread other([&]() {
                while (!stop.load()) {
                    const int rc = bsw_matesw_ref_submit_t(ctx, &p, ref, fill.data(), fill.size(), fo[3].data(), &tf[3]);
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
                CHECK(bsw_rescue_test(j) == 0, "test with the four places taken");
                CHECK(finish(j, o) == BSW_E_BUSY, "finish with the four places taken, again");
                bsw_rescue_stats st;
                CHECK(bsw_rescue_job_stats(j, &st) == BSW_OK && st.rounds == 2, "the job is intact");
                CHECK(bsw_wait_ticket(ctx, tf[0]) == BSW_OK, "a ticket: %s", bsw_last_error(ctx));
                tf[0] = 0;
                rc = finish(j, o);
            }
            CHECK(rc == BSW_OK, "finish: %d (%s)", rc, bsw_last_error(ctx));
            same_r(o, w, "a job whose follow-up round found no place");
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
    const bsw_params p = default_params();
    rwork w;
    fresh(1);
    make_pairs(w, 31, 40);
    expect(w, p);
    check_workload(w);
    sweep_t s;
    /* releases whose code is ignored by design; a slot's hipSetDevice when it gets no chunk */
    s.releases = {"hipSetDevice", "hipFree", "hipHostFree", "hipGetLastError", "hipEventDestroy", "hipStreamDestroy", "hipHostUnregister", "hipEventQuery"};
    s.min_visited = 40; s.min_failed = 30;
    fault_sweep(s, 2, [&](sweep_t &s) {
        const unsigned long long k = s.k;
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 128, 1, 4000);
        bsw_ref *ref = upload(ctx, w.g);
        both_forms(ctx, p, ref, w, "the warm-up");
        bsw_reads *rd = upload_reads(ctx, w);
        s.arm();
        bsw_rescue_job *j[2] = {nullptr, nullptr};
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
        if (rc[0] == BSW_OK) same_r(o0, w, "a pointer job that reported success");
        if (rc[1] == BSW_OK) same_r(o1, w, "a reads job that reported success");
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
    fprintf(stderr, "usage: host_rescue forms | mixed | busy | faults\n");
    return 2;
}
