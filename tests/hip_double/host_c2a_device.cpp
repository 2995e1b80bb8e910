/* host_c2a_device.cpp — the main library's unit of the chain2aln device replay (bsw_c2a_device.hip: the launcher table, the switch,
 * the chunk function, bsw_chain2aln_replay_batch and bsw_chain2aln_replay_submit_t) and the two-stage job of bsw_chain2aln_job.hip on
 * the host-memory HIP stand-in, plain and under ASan / UBSan or TSan (TEST INFRASTRUCTURE; tests/test_c2a_device_cpu.py adds its row
 * to tests/_host_double_build.py and runs it).  launchers_c2a.cpp registers a CPU launcher built from bsw_c2a_core.h, the header the
 * kernel is compiled from.  The oracle is bsw_chain2aln_replay on the same arrays.
 *
 *   host_c2a_device calls    both calls on synthetic chains: 1 - 3 devices, both record formats, BSW_C2A_DEV_CHUNK 1 / 256 / 4 096,
 *                            a read above the cap (the host route), reads without a chain, extended = NULL, no seed at all, refusals
 *   host_c2a_device job      the chain2aln job with the switch on, both forms (the workload and the checks of host_chain2aln.cpp),
 *                            polled and blocking; a dropped job gives its place and its block back
 *   host_c2a_device faults   every HIP / launcher call of a replay ticket fails in turn
 *   host_c2a_device busy     the job when its replay submit meets BSW_E_BUSY — through a c2a_job_ops table of this program whose submit
 *                            answers BSW_E_BUSY a given number of times before it forwards, and with the four places really taken:
 *                            test answers 0 and later 1, finish answers BSW_E_BUSY with the job intact and then succeeds; dropped there
 */
#include "../../bwa-mem-sw_amd/csrc/bsw_internal.h"  /* c2a_job_ops, c2a_job_register: the table the job reaches the replay through */
#define main host_chain2aln_main                     /* the job's workload, expectations and checks: stated once, there */
#include "host_chain2aln.cpp"
#undef main

namespace standin_c2a { uint64_t launches(); }
static uint64_t standin_c2a_launches() { return standin_c2a::launches(); }

struct cset {
    std::vector<bsw_chain> chains;
    std::vector<bsw_cseed> seeds;
    std::vector<int32_t> lens;
    std::vector<bsw_pair> pairs;
    std::vector<bsw_result> full;                    /* the same records with junk in the tail */
    std::vector<bsw_creg> want;
    std::vector<uint8_t> want_ext;
    std::vector<uint64_t> want_start;
    size_t n_host = 0, n_with_chain = 0;
};

/* the recipe of tests/_c2a_device_gen.py; big: read `big` gets one chain of that many seeds in front */
static void make_set(cset &s, rng_t &r, size_t n_reads, const std::vector<int> &sizes, size_t big_read, int big)
{
    static const int ws[6] = {1, 5, 10, 50, 100, 200};
    for (size_t i = 0; i < n_reads; ++i) {
        const int l = r.in(100, 250);
        s.lens.push_back(l);
        if (i % 11 == 5) continue;                   /* a read without any chain */
        ++s.n_with_chain;
        std::vector<int> counts;
        if (i == big_read && big) counts.push_back(big);
        for (int k = r.in(1, 4); k > 0; --k) counts.push_back(sizes[(size_t)r.below((int)sizes.size())]);
        bool host = false;
        int64_t d0 = 0;
        for (size_t k = 0; k < counts.size(); ++k) {
            if (!k || r.below(2)) d0 = ((int64_t)(i % 3 == 0) << 33) + r.in(1000, 1000000);
            bsw_chain c;
            memset(&c, 0, sizeof(c));
            c.read = (uint32_t)i; c.n_seeds = counts[k]; c.first_seed = s.seeds.size(); c.rid = r.below(25); c.frac_rep = (float)r.below(100) / 128.f;
            s.chains.push_back(c);
            host = host || counts[k] > 512;
            for (int j = 0; j < counts[k]; ++j) {
                const int len = r.in(12, 40), qb = r.below(l - len + 1), off = r.unit() < .7 ? 0 : r.in(-6, 6);
                const int sc = r.unit() < .7 ? len : r.below(len + 1), gl = r.below(qb + 1), gr = r.below(l - qb - len + 1);
                s.seeds.push_back(bsw_cseed{d0 + qb + off, qb, len, sc, 0});
                s.pairs.push_back(bsw_pair{(uint32_t)s.pairs.size(), qb - gl, gr, -std::max(gl + r.in(-2, 2), 0), std::max(gr + r.in(-2, 2), 0), r.below(300), r.below(300), ws[r.below(6)]});
            }
        }
        s.n_host += host;
    }
    s.full.resize(s.pairs.size());
    for (size_t i = 0; i < s.pairs.size(); ++i) {
        memset(&s.full[i], 0xa5 ^ (int)(i & 0xff), sizeof(bsw_result));
        memcpy(&s.full[i], &s.pairs[i], sizeof(bsw_pair));
    }
}

static void expect_set(cset &s, const bsw_params &p, const bsw_c2a_opt *o)
{
    const size_t n = s.seeds.size();
    s.want.assign(n + 1, bsw_creg());
    s.want_ext.assign(n + 1, 0);
    s.want_start.assign(s.lens.size() + 1, 0);
    size_t nr = 0;
    CHECK(bsw_chain2aln_replay(&p, o, s.chains.data(), s.chains.size(), s.seeds.data(), n, s.lens.data(), s.lens.size(), s.pairs.data(), BSW_RESULT_PAIR, s.want.data(), &nr,
                               s.want_ext.data(), s.want_start.data()) == BSW_OK, "bsw_chain2aln_replay");
    s.want.resize(nr);
}

struct douts {
    std::vector<bsw_creg> regs;
    std::vector<uint8_t> ext;
    std::vector<uint64_t> start;
    size_t n = 77;
    bsw_c2a_dev_stats st;
    explicit douts(const cset &s) : regs(s.seeds.size() + 1), ext(s.seeds.size() + 1, 0x5a), start(s.lens.size() + 2, 0x5a5a)
    {
        memset(regs.data(), 0x5a, regs.size() * sizeof(bsw_creg));
        memset(&st, 0x5a, sizeof(st));
    }
};

static int replay_batch(bsw_ctx *ctx, const bsw_params &p, const bsw_c2a_opt *o, const cset &s, bool full, douts &d, bool ext = true)
{
    return bsw_chain2aln_replay_batch(ctx, &p, o, s.chains.data(), s.chains.size(), s.seeds.data(), s.seeds.size(), s.lens.data(), s.lens.size(),
                                      full ? (const void *)s.full.data() : (const void *)s.pairs.data(), full ? BSW_RESULT_FULL : BSW_RESULT_PAIR, d.regs.data(), &d.n,
                                      ext ? d.ext.data() : nullptr, d.start.data(), &d.st);
}
static int replay_submit(bsw_ctx *ctx, const bsw_params &p, const bsw_c2a_opt *o, const cset &s, bool full, douts &d, bsw_ticket *t, bool ext = true)
{
    return bsw_chain2aln_replay_submit_t(ctx, &p, o, s.chains.data(), s.chains.size(), s.seeds.data(), s.seeds.size(), s.lens.data(), s.lens.size(),
                                         full ? (const void *)s.full.data() : (const void *)s.pairs.data(), full ? BSW_RESULT_FULL : BSW_RESULT_PAIR, d.regs.data(), &d.n,
                                         ext ? d.ext.data() : nullptr, d.start.data(), &d.st, t);
}

static void same_d(const douts &d, const cset &s, const char *what, bool ext = true)
{
    const size_t n = s.seeds.size();
    CHECK(d.n == s.want.size(), "%s: %zu regions, want %zu", what, d.n, s.want.size());
    for (size_t i = 0; i < d.n; ++i)
        CHECK(memcmp(&d.regs[i], &s.want[i], sizeof(bsw_creg)) == 0, "%s: region %zu of %zu: read %u seed %u, want read %u seed %u", what, i, d.n, d.regs[i].read, d.regs[i].seed,
              s.want[i].read, s.want[i].seed);
    if (ext) CHECK(memcmp(d.ext.data(), s.want_ext.data(), n) == 0, "%s: extended[] differs", what);
    else for (size_t i = 0; i < n; ++i) CHECK(d.ext[i] == 0x5a, "%s: extended[] was not asked for and is written", what);
    CHECK(memcmp(d.start.data(), s.want_start.data(), (s.lens.size() + 1) * sizeof(uint64_t)) == 0, "%s: reg_start[] differs", what);
    CHECK(d.ext[n] == 0x5a && d.start[s.lens.size() + 1] == 0x5a5a && d.regs[n].seed == 0x5a5a5a5au, "%s: a write behind the caller's arrays", what);
    CHECK(d.st.reads_host == s.n_host && d.st.reads_gpu == s.n_with_chain - s.n_host, "%s: reads_gpu %llu, reads_host %llu", what, (unsigned long long)d.st.reads_gpu,
          (unsigned long long)d.st.reads_host);
    CHECK(d.st.d2h_bytes <= 64 * d.n + 8 * s.n_with_chain + (ext ? n : 0) + 256 * d.st.chunks, "%s: %llu bytes came back", what, (unsigned long long)d.st.d2h_bytes);
}

static int calls_mode()
{
    const bsw_params p = params_of(BSW_VARIANT_H);
    size_t runs = 0;
    for (int D : {1, 2, 3})
        for (const char *chunk : {"1", "256", "4096"}) {
            fresh(D);
            setenv("BSW_C2A_DEV_CHUNK", chunk, 1);
            {
                rng_t r(90 + (uint64_t)D);
                cset s;
                make_set(s, r, 70, {1, 15, 16, 17, 31, 32, 33, 63, 64, 65}, 20, D == 2 ? 513 : 600);
                bsw_c2a_opt o;
                bsw_c2a_default_opt(&o);
                if (D == 3) { o.seedlen0_frac = 1. / 3; o.ovl_len_frac = 2. / 3; }
                expect_set(s, p, &o);
                CHECK(s.n_host == 1 && s.want.size() > s.seeds.size() / 5, "the set: %zu host reads, %zu regions of %zu seeds", s.n_host, s.want.size(), s.seeds.size());
                bsw_ctx *ctx = ctx_of(D, 0, BSW_RESULT_FULL);
                for (int full = 0; full < 2; ++full)
                    for (int ext = 1; ext >= 0; --ext) {
                        douts a(s), b(s);
                        CHECK(replay_batch(ctx, p, &o, s, full != 0, a, ext != 0) == BSW_OK, "bsw_chain2aln_replay_batch: %s", bsw_last_error(ctx));
                        same_d(a, s, "the synchronous call", ext != 0);
                        bsw_ticket t = 0;
                        CHECK(replay_submit(ctx, p, &o, s, full != 0, b, &t, ext != 0) == BSW_OK && t, "bsw_chain2aln_replay_submit_t: %s", bsw_last_error(ctx));
                        /* the synchronous call while the ticket is uncollected */
                        douts busy(s);
                        CHECK(replay_batch(ctx, p, &o, s, false, busy) == BSW_E_BUSY && busy.n == 0, "the synchronous call beside a ticket");
                        CHECK(bsw_inflight(ctx) == 1 && bsw_wait_ticket(ctx, t) == BSW_OK && bsw_inflight(ctx) == 0, "the ticket: %s", bsw_last_error(ctx));
                        same_d(b, s, "the ticket", ext != 0);
                        CHECK(a.st.chunks == b.st.chunks && (strcmp(chunk, "1") ? a.st.chunks > 1 : a.st.chunks == s.n_with_chain), "%llu chunks", (unsigned long long)a.st.chunks);
                        ++runs;
                    }
                /* four tickets, the fifth is refused and changes nothing */
                std::vector<std::unique_ptr<douts>> d;
                bsw_ticket t[5] = {0, 0, 0, 0, 9};
                for (int k = 0; k < 4; ++k) {
                    d.emplace_back(new douts(s));
                    CHECK(replay_submit(ctx, p, &o, s, false, *d.back(), &t[k]) == BSW_OK, "ticket %d: %s", k, bsw_last_error(ctx));
                }
                douts five(s);
                CHECK(replay_submit(ctx, p, &o, s, false, five, &t[4]) == BSW_E_BUSY && t[4] == 0 && five.regs[0].seed == 0x5a5a5a5au, "the fifth ticket");
                for (int k = 3; k >= 0; --k) { CHECK(bsw_wait_ticket(ctx, t[k]) == BSW_OK, "ticket %d: %s", k, bsw_last_error(ctx)); same_d(*d[(size_t)k], s, "one of four tickets"); }
                /* no seed at all; bad arrays: the host replay's codes */
                cset none;
                none.lens = {100, 120};
                expect_set(none, p, nullptr);
                douts dn(none);
                CHECK(replay_batch(ctx, p, nullptr, none, false, dn) == BSW_OK && dn.n == 0 && dn.start[0] == 0 && dn.start[2] == 0 && dn.st.chunks == 0, "no seed at all");
                bsw_ticket tn = 0;
                CHECK(replay_submit(ctx, p, nullptr, none, false, dn, &tn) == BSW_OK && bsw_test(ctx, tn) == 1 && bsw_wait_ticket(ctx, tn) == BSW_OK && dn.n == 0, "no seed at all as a ticket");
                cset bad = s;
                bad.chains[1].first_seed += 1;
                douts db(bad);
                const int want_rc = bsw_chain2aln_replay(&p, &o, bad.chains.data(), bad.chains.size(), bad.seeds.data(), bad.seeds.size(), bad.lens.data(), bad.lens.size(), bad.pairs.data(),
                                                         BSW_RESULT_PAIR, db.regs.data(), &db.n, nullptr, nullptr);
                CHECK(want_rc == BSW_E_INVAL && replay_batch(ctx, p, &o, bad, false, db) == want_rc && strstr(bsw_last_error(ctx), "do not follow"), "bad arrays: %s", bsw_last_error(ctx));
                CHECK(replay_submit(ctx, p, &o, bad, false, db, &tn) == want_rc && tn == 0 && bsw_inflight(ctx) == 0, "bad arrays as a ticket");
                bsw_destroy(ctx);
            }
            CHECK(hipdbl::live_objects() == 0, "%zu HIP objects left alive", hipdbl::live_objects());
        }
    unsetenv("BSW_C2A_DEV_CHUNK");
    printf("calls: %zu pairs of calls\ncalls ok\n", runs);
    return 0;
}

static int job_mode()
{
    genome_t g;
    g.make(70001, 5);
    CHECK(bsw_set_c2a_device(1) == BSW_OK && bsw_c2a_device() == 1, "the switch with a registered launcher");
    size_t runs = 0;
    for (int D : {1, 2})
        for (int format : {BSW_RESULT_FULL, BSW_RESULT_PAIR}) {
            fresh(D);
            {
                rng_t r(50 + (uint64_t)D);
                cwork w;
                make_chains(w, g, r, 260);
                const bsw_params p = params_of(D == 1 ? BSW_VARIANT_H : BSW_VARIANT_RTL);
                expect(w, g, p, format == BSW_RESULT_PAIR);
                bsw_ctx *ctx = ctx_of(D, 256, format);
                bsw_ref *ref = upload(ctx, g);
                setenv("BSW_C2A_DEV_CHUNK", "512", 1);
                both_forms(ctx, p, ref, w, "the two-stage job, polled");          /* (two jobs in flight: two submits, polled to 1, uncollected) */
                unsetenv("BSW_C2A_DEV_CHUNK");
                /* blocking alone; the switch turned off behind the job's back changes nothing for it */
                bsw_c2a_job *j = nullptr;
                CHECK(start_ref(ctx, p, ref, w, &j) == BSW_OK && j, "start: %s", bsw_last_error(ctx));
                CHECK(bsw_set_c2a_device(0) == BSW_OK, "the switch off");
                outs o(w);
                CHECK(finish(j, o) == BSW_OK && bsw_inflight(ctx) == 0, "finish: %s", bsw_last_error(ctx));
                same_c(o, w, "the two-stage job, blocking");
                const uint64_t launches = standin_c2a_launches();
                CHECK(launches > 0, "the job did not replay on the device");
                /* with the switch off the job replays on the host: no launch */
                CHECK(start_ref(ctx, p, ref, w, &j) == BSW_OK && j, "start: %s", bsw_last_error(ctx));
                outs oh(w);
                CHECK(finish(j, oh) == BSW_OK && standin_c2a_launches() == launches, "the job with the switch off launched the replay");
                same_c(oh, w, "the job with the switch off");
                CHECK(bsw_set_c2a_device(1) == BSW_OK, "the switch on");
                /* dropped: in the first stage, and once the replay ticket is there */
                bsw_reads *rd = upload_reads(ctx, w);
                size_t n = 5;
                CHECK(start_reads(ctx, p, ref, rd, w, &j) == BSW_OK && bsw_inflight(ctx) == 1, "start: %s", bsw_last_error(ctx));
                CHECK(bsw_chain2aln_finish(j, nullptr, &n, nullptr, nullptr, nullptr) == BSW_E_INVAL && n == 0 && bsw_inflight(ctx) == 0, "a dropped job in its first stage");
                CHECK(start_reads(ctx, p, ref, rd, w, &j) == BSW_OK, "start: %s", bsw_last_error(ctx));
                int t = 0;
                while ((t = bsw_chain2aln_test(j)) == 0) std::this_thread::yield();
                CHECK(t == 1 && bsw_inflight(ctx) == 1 && bsw_chain2aln_test(j) == 1, "the poll of the two-stage job -> %d", t);
                CHECK(bsw_chain2aln_finish(j, nullptr, &n, nullptr, nullptr, nullptr) == BSW_E_INVAL && bsw_inflight(ctx) == 0, "a dropped job in its second stage");
                CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "the dropped jobs hold the block: %s", bsw_last_error(ctx));
                bsw_ref_free(ctx, ref);
                bsw_destroy(ctx);
                ++runs;
            }
            CHECK(hipdbl::live_objects() == 0, "%zu HIP objects left alive", hipdbl::live_objects());
        }
    bsw_set_c2a_device(0);
    printf("job: %zu contexts\njob ok\n", runs);
    return 0;
}

/* every HIP / launcher call of a replay ticket fails in turn (ONE slot per device and a warm-up in front of the window, as in
 * host_chain2aln.cpp); another replay ticket, complete and uncollected, sits beside it */
static int c2a_faults_mode()
{
    const bsw_params p = params_of(BSW_VARIANT_H);
    rng_t r0(77);
    cset s, other;
    make_set(s, r0, 40, {1, 16, 17, 33}, 7, 520);
    make_set(other, r0, 30, {2, 15, 32}, 0, 0);
    expect_set(s, p, nullptr);
    expect_set(other, p, nullptr);
    setenv("BSW_C2A_DEV_CHUNK", "128", 1);
    sweep_t sw;
    sw.releases = {"hipFree", "hipHostFree", "hipGetLastError", "hipEventDestroy", "hipStreamDestroy", "hipHostUnregister"};
    sw.exact = true;
    sw.min_failed = 20;
    fault_sweep(sw, 2, [&](sweep_t &sw) {
        const unsigned long long k = sw.k;
        bsw_ctx *ctx = ctx_of(2, 0, BSW_RESULT_FULL, 4000, 1);
        for (int full = 0; full < 2; ++full) {       /* the warm-up: the pipeline runs, both slots hold their staging */
            douts wu(s);
            bsw_ticket t = 0;
            CHECK(replay_submit(ctx, p, nullptr, s, full != 0, wu, &t) == BSW_OK && bsw_wait_ticket(ctx, t) == BSW_OK, "the warm-up: %s", bsw_last_error(ctx));
            same_d(wu, s, "the warm-up");
        }
        douts od(other);
        bsw_ticket to = 0;
        CHECK(replay_submit(ctx, p, nullptr, other, false, od, &to) == BSW_OK, "the other ticket: %s", bsw_last_error(ctx));
        while (bsw_test(ctx, to) == 0) std::this_thread::yield();
        sw.arm();
        douts d(s);
        bsw_ticket t = 0;
        int rc = replay_submit(ctx, p, nullptr, s, true, d, &t);
        CHECK((rc != 0) == (t == 0), "k=%llu: submit -> %d and ticket %llu", k, rc, (unsigned long long)t);
        if (!rc) rc = bsw_wait_ticket(ctx, t);
        const std::string text = rc ? bsw_last_error(ctx) : "";
        sw.judge({{rc, text}});
        if (rc == BSW_OK) same_d(d, s, "a ticket that reported success");
        else CHECK(d.n == 0, "k=%llu: a failed ticket leaves %zu regions", k, d.n);
        if (k == 0) printf("faults: C = %llu\n", (unsigned long long)sw.C);
        CHECK(bsw_wait_ticket(ctx, to) == BSW_OK && bsw_inflight(ctx) == 0, "k=%llu: the other ticket: %s", k, bsw_last_error(ctx));
        same_d(od, other, "the other ticket");
        douts again(s), sync(s);                     /* the context is alive: the next replays are exact */
        CHECK(replay_submit(ctx, p, nullptr, s, false, again, &t) == BSW_OK && bsw_wait_ticket(ctx, t) == BSW_OK, "k=%llu: the next ticket: %s", k, bsw_last_error(ctx));
        same_d(again, s, "the next ticket");
        CHECK(replay_batch(ctx, p, nullptr, s, true, sync) == BSW_OK, "k=%llu: the next synchronous call: %s", k, bsw_last_error(ctx));
        same_d(sync, s, "the next synchronous call");
        bsw_destroy(ctx);
    });
    unsetenv("BSW_C2A_DEV_CHUNK");
    printf("faults: injection points visited = %llu, the ticket failed %llu times, ignored %llu\n", (unsigned long long)sw.visited, (unsigned long long)sw.failed, (unsigned long long)sw.ignored);
    sw.done();
    printf("faults ok\n");
    return 0;
}

/* ---- busy ---- */
static std::atomic<int> g_busy_left{0}, g_busy_seen{0};
static int busy_submit(bsw_ctx *ctx, const bsw_params *p, const bsw_c2a_opt *opt, const bsw_chain *chains, size_t n_chains, const bsw_cseed *seeds, size_t n_seeds,
                       const int32_t *lens, size_t n_reads, const void *results, int result_format, bsw_creg *regs, size_t *n_regs, uint8_t *extended,
                       uint64_t *reg_start, bsw_c2a_dev_stats *stats, bsw_ticket *ticket)
{
    if (g_busy_left.load() > 0) { --g_busy_left; ++g_busy_seen; if (ticket) *ticket = 0; return BSW_E_BUSY; }
    return bsw_chain2aln_replay_submit_t(ctx, p, opt, chains, n_chains, seeds, n_seeds, lens, n_reads, results, result_format, regs, n_regs, extended, reg_start, stats, ticket);
}
static const c2a_job_ops g_busy_ops = {bsw_c2a_device, busy_submit};

static int busy_mode()
{
    genome_t g;
    g.make(70001, 5);
    c2a_job_register(&g_busy_ops);                   /* (in place of the unit's own table, for the rest of the program) */
    CHECK(bsw_set_c2a_device(1) == BSW_OK, "the switch");
    const bsw_params p = params_of(BSW_VARIANT_H);
    size_t runs = 0;
    for (int form = 0; form < 2; ++form) {
        fresh(2);
        {
            rng_t r(61 + (uint64_t)form);
            cwork w;
            make_chains(w, g, r, 120);
            expect(w, g, p, false);
            cset s;
            make_set(s, r, 20, {2, 3, 17}, 0, 0);
            expect_set(s, p, nullptr);
            bsw_ctx *ctx = ctx_of(2, 256, BSW_RESULT_FULL);
            bsw_ref *ref = upload(ctx, g);
            bsw_reads *rd = upload_reads(ctx, w);
            auto start = [&](bsw_c2a_job **j) {
                const int rc = form ? start_reads(ctx, p, ref, rd, w, j) : start_ref(ctx, p, ref, w, j);
                CHECK(rc == BSW_OK && *j && bsw_inflight(ctx) == 1, "start: %s", bsw_last_error(ctx));
            };
            bsw_c2a_job *j = nullptr;
            int t = 0;
            /* polled: three refusals, then the replay runs.  test never answers an error; between the refusals the job holds no place */
            g_busy_left = 3; g_busy_seen = 0;
            start(&j);
            size_t zeros_after = 0;
            while ((t = bsw_chain2aln_test(j)) == 0) { if (g_busy_seen.load()) ++zeros_after; if (g_busy_seen.load() && g_busy_left.load()) CHECK(bsw_inflight(ctx) == 0, "a refused job holds a place"); std::this_thread::yield(); }
            CHECK(t == 1 && g_busy_seen.load() == 3 && g_busy_left.load() == 0 && zeros_after >= 3, "the poll over three refusals -> %d after %d refusals", t, g_busy_seen.load());
            CHECK(bsw_inflight(ctx) == 1 && bsw_chain2aln_test(j) == 1, "complete, and the job's to collect");
            {
                outs o(w);
                CHECK(finish(j, o) == BSW_OK && bsw_inflight(ctx) == 0, "finish after the poll: %s", bsw_last_error(ctx));
                same_c(o, w, "polled over three refusals");
            }
            /* blocking: finish answers BSW_E_BUSY twice, the job and the caller's arrays intact, then succeeds (its own arrays are reused) */
            g_busy_left = 2; g_busy_seen = 0;
            start(&j);
            {
                outs o(w);
                CHECK(finish(j, o) == BSW_E_BUSY && o.n == 0 && o.regs[0].seed == 0x5a5a5a5au && o.ext[0] == 0x5a, "the first finish");
                CHECK(bsw_inflight(ctx) == 0, "a refused job holds a place");
                bsw_c2a_stats st;
                CHECK(bsw_chain2aln_stats(j, &st) == BSW_OK && st.seeds_gpu == w.seeds.size(), "the job is intact after BSW_E_BUSY");
                CHECK(finish(j, o) == BSW_E_BUSY && g_busy_seen.load() == 2, "the second finish");
                CHECK(finish(j, o) == BSW_OK && bsw_inflight(ctx) == 0, "the third finish: %s", bsw_last_error(ctx));
                same_c(o, w, "finish after two refusals");
            }
            /* the four places REALLY taken while the job has none: the poll answers 0 and leaves no text, finish answers the submit's own
             * BSW_E_BUSY, and once a place is free it succeeds */
            g_busy_left = 1; g_busy_seen = 0;
            start(&j);
            while (!g_busy_seen.load()) { CHECK(bsw_chain2aln_test(j) == 0, "the poll before the refusal"); std::this_thread::yield(); }
            CHECK(bsw_inflight(ctx) == 0, "the job holds no place after the refusal");
            std::vector<std::unique_ptr<douts>> d;
            bsw_ticket tk[4];
            for (int k = 0; k < 4; ++k) {
                d.emplace_back(new douts(s));
                CHECK(replay_submit(ctx, p, nullptr, s, false, *d.back(), &tk[k]) == BSW_OK, "ticket %d: %s", k, bsw_last_error(ctx));
            }
            const std::string before = bsw_last_error(ctx);
            for (int k = 0; k < 5; ++k) CHECK(bsw_chain2aln_test(j) == 0 && bsw_inflight(ctx) == 4, "the poll beside four tickets");
            CHECK(before == bsw_last_error(ctx), "a poll that met BSW_E_BUSY wrote the context's text: %s", bsw_last_error(ctx));
            {
                outs o(w);
                CHECK(finish(j, o) == BSW_E_BUSY && strstr(bsw_last_error(ctx), "BSW_MAX_INFLIGHT") && bsw_inflight(ctx) == 4, "finish beside four tickets: %s", bsw_last_error(ctx));
                CHECK(bsw_wait_ticket(ctx, tk[3]) == BSW_OK, "ticket 3: %s", bsw_last_error(ctx));
                CHECK(bsw_chain2aln_test(j) >= 0 && bsw_inflight(ctx) == 4, "the poll takes the free place");
                while ((t = bsw_chain2aln_test(j)) == 0) std::this_thread::yield();
                CHECK(t == 1 && finish(j, o) == BSW_OK && bsw_inflight(ctx) == 3, "finish once a place was free: %s", bsw_last_error(ctx));
                same_c(o, w, "finish once a place was free");
            }
            for (int k = 0; k < 3; ++k) { CHECK(bsw_wait_ticket(ctx, tk[k]) == BSW_OK, "ticket %d: %s", k, bsw_last_error(ctx)); same_d(*d[(size_t)k], s, "a ticket beside the refused job"); }
            same_d(*d[3], s, "a ticket beside the refused job");
            /* dropped after a refusal: no replay is started for it; the place and the block are given back */
            g_busy_left = 1; g_busy_seen = 0;
            start(&j);
            while (!g_busy_seen.load()) { CHECK(bsw_chain2aln_test(j) == 0, "the poll before the refusal"); std::this_thread::yield(); }
            size_t n = 5;
            g_busy_left = 7;                         /* (a replay submit from here on would be refused: none is made) */
            CHECK(bsw_chain2aln_finish(j, nullptr, &n, nullptr, nullptr, nullptr) == BSW_E_INVAL && n == 0 && g_busy_left.load() == 7 && bsw_inflight(ctx) == 0, "a job dropped after a refusal");
            g_busy_left = 0;
            CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "the block after the jobs: %s", bsw_last_error(ctx));
            bsw_ref_free(ctx, ref);
            bsw_destroy(ctx);
            ++runs;
        }
        CHECK(hipdbl::live_objects() == 0, "%zu HIP objects left alive", hipdbl::live_objects());
    }
    bsw_set_c2a_device(0);
    printf("busy: %zu contexts\nbusy ok\n", runs);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "busy") return busy_mode();
    if (mode == "calls") return calls_mode();
    if (mode == "job") return job_mode();
    if (mode == "faults") return c2a_faults_mode();
    fprintf(stderr, "usage: host_c2a_device calls | job | faults | busy\n");
    return 2;
}
