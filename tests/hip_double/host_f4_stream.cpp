/* host_f4_stream.cpp — bsw_cigar_ref_submit_t / bsw_matesw_ref_submit_t (the CIGAR and mate-rescue jobs of the slot pipeline,
 * bsw_batch.hip / bsw_cigar.hip / bsw_matesw.hip) on the host-memory HIP stand-in, under ASan / UBSan or TSan
 * (TEST INFRASTRUCTURE; tests/test_f4_stream_cpu.py builds, links and runs it).
 *
 *   host_f4_stream parity     submits on 1, 2, 3 and 8 devices, registered and pageable reads, more chunks than slots: equal to
 *                             the synchronous calls on a one-device context, byte for byte
 *   host_f4_stream reach      every stream of device 1 of two stalled: a multi-chunk submit does not complete until they are released
 *   host_f4_stream mixed      four submits of three kinds in flight, the fifth and the synchronous call answer BSW_E_BUSY
 *   host_f4_stream storm      nine threads submit and collect mixed tickets on one context
 *   host_f4_stream faults     every single HIP or launcher call of a three-ticket scenario fails in turn
 *   host_f4_stream watchdog   a stalled stream under a short timeout: BSW_E_HIP, the context is dead
 *
 * The workloads are those the synchronous calls are tested with: this file takes make_cigar / make_matesw, the genome and the
 * arena from host_f4_work.h, as host_f4.cpp does, so a kind, strand or retry count added there is run here too.
 * The expected values are the synchronous calls' results, which tests/test_host_double_cpu.py compares with the restatements of
 * bwa (tests/_gencigar_ref.py, tests/_matesw_ref.py) on the same workloads.
 */
#include "host_f4_tickets.h"

/* ---- parity ---- */
static int parity_mode()
{
    const bsw_params p = default_params();
    genome1_t g;
    g.make(150001, 77);
    const size_t n = 1300;
    size_t cases = 0;
    uint64_t chunks_seen = 0;
    for (int reg = 0; reg < 2; ++reg) {
        fresh(8);
        {
            rng_t r(2000 + (uint64_t)reg);
            arena_t arc(n * 300 + 8192, reg != 0), arm(n * 400 + 8192, reg != 0);
            cwork cw;
            mwork mw;
            make_cigar(cw, arc, g, r, n);
            make_matesw(mw, arm, g, r, n);
            want_t want;
            expected_f4(p, g, cw, mw, want);
            {   /* the workload holds what the issue names */
                int st[3] = {0, 0, 0}, tries[4] = {0, 0, 0, 0}, rev = 0, fwd = 0, nogap = 0, mst[3] = {0, 0, 0}, isrev[2] = {0, 0};
                for (size_t i = 0; i < n; ++i) {
                    const bsw_cresult &c = want.c.res[i];
                    ++st[c.status ? 1 : 0];
                    if (!c.status) { ++tries[std::min(c.tries, 3)]; (cw.t[i].rb >= g.l_pac ? rev : fwd)++; nogap += cw.t[i].w == 0; }
                    ++mst[want.m[i].status];
                    ++isrev[mw.t[i].is_rev];
                }
                CHECK(st[0] && st[1] && tries[1] && tries[2] && tries[3] && rev && fwd && nogap, "the CIGAR workload lacks a status, a strand, a retry count or the no-gap shortcut");
                CHECK(mst[0] && mst[1] && mst[2] && isrev[0] && isrev[1], "the rescue workload lacks a status or an orientation");
            }
            const int GS[] = {1, 2, 3, 8};
            const size_t live0 = hipdbl::live_objects();           /* (the registered arenas) */
            for (int G : GS) {
                bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, G, 256, 2);
                bsw_ref *ref = upload(ctx, g);
                c_out co;
                std::vector<bsw_mresult> mo;
                bsw_ticket tc = 0, tm = 0;
                int rc = submit_m(ctx, p, ref, mw, mo, &tm);
                CHECK(rc == BSW_OK && tm, "bsw_matesw_ref_submit_t on %d devices -> %d (%s)", G, rc, bsw_last_error(ctx));
                rc = submit_c(ctx, p, ref, cw, co, &tc);
                CHECK(rc == BSW_OK && tc && tc != tm, "bsw_cigar_ref_submit_t on %d devices -> %d (%s)", G, rc, bsw_last_error(ctx));
                CHECK(bsw_inflight(ctx) == 2, "bsw_inflight says %d with two tickets uncollected", bsw_inflight(ctx));
                rc = bsw_wait_ticket(ctx, tc);
                CHECK(rc == BSW_OK, "the CIGAR ticket on %d devices -> %d (%s)", G, rc, bsw_last_error(ctx));
                rc = bsw_wait(ctx);
                CHECK(rc == BSW_OK, "bsw_wait on %d devices -> %d (%s)", G, rc, bsw_last_error(ctx));
                std::string why;
                CHECK(same_c(co, want.c, n, &why), "%s reads, %d devices: the CIGAR submit differs from bsw_cigar_ref_batch: %s", reg ? "registered" : "pageable", G, why.c_str());
                CHECK(same_m(mo, want.m, n), "%s reads, %d devices: the rescue submit differs from bsw_matesw_ref_batch", reg ? "registered" : "pageable", G);
                const bsw_stats s = stats_of(ctx);
                CHECK(s.submits == 2 && s.seeds == 0 && s.h2d_bytes > 0 && s.d2h_bytes >= n * (sizeof(bsw_cresult) + sizeof(bsw_kswr)), "bsw_host_stats: %llu submits, %llu seeds, %llu / %llu bytes",
                      (unsigned long long)s.submits, (unsigned long long)s.seeds, (unsigned long long)s.h2d_bytes, (unsigned long long)s.d2h_bytes);
                CHECK(s.chunks > 2ull * 2 * (uint64_t)G, "%llu chunks for two submits on %d devices of 2 slots: not more chunks than slots", (unsigned long long)s.chunks, G);
                chunks_seen += s.chunks;
                /* n == 0 completes at once; ticket may be NULL */
                bsw_ticket t0 = 0;
                CHECK(bsw_matesw_ref_submit_t(ctx, &p, ref, nullptr, 0, nullptr, &t0) == BSW_OK && t0 && bsw_test(ctx, t0) == 1, "an empty rescue submit");
                CHECK(bsw_cigar_ref_submit_t(ctx, &p, ref, nullptr, 0, MAXC, nullptr, MAXMD, nullptr, nullptr, nullptr) == BSW_OK, "an empty CIGAR submit without a ticket");
                CHECK(bsw_wait(ctx) == BSW_OK && bsw_inflight(ctx) == 0, "the empty submits");
                /* the checks of the synchronous calls, in the caller's thread, and no ticket */
                {
                    std::vector<bsw_mtask> bad(mw.t.begin(), mw.t.begin() + 40);
                    bad[17].is_rev = 2;
                    std::vector<bsw_mresult> br(40);
                    bsw_ticket tb = 77;
                    rc = bsw_matesw_ref_submit_t(ctx, &p, ref, bad.data(), 40, br.data(), &tb);
                    const std::string a = bsw_last_error(ctx);
                    CHECK(rc == BSW_E_INVAL && tb == 0 && bsw_inflight(ctx) == 0, "a malformed rescue task -> %d, ticket %llu", rc, (unsigned long long)tb);
                    rc = bsw_matesw_ref_batch(ctx, &p, ref, bad.data(), 40, br.data());
                    CHECK(rc == BSW_E_INVAL && a == bsw_last_error(ctx), "the submit says '%s', the batch call '%s'", a.c_str(), bsw_last_error(ctx));
                    std::vector<bsw_ctask> cb(cw.t.begin(), cw.t.begin() + 40);
                    cb[23].max_tries = 4;
                    cb[31].l_query = BSW_GLOBAL_MAX_QLEN + 1;
                    std::vector<bsw_cresult> cr(40);
                    rc = bsw_cigar_ref_submit_t(ctx, &p, ref, cb.data(), 40, MAXC, nullptr, MAXMD, nullptr, cr.data(), &tb);
                    const std::string b = bsw_last_error(ctx);
                    CHECK(rc == BSW_E_INVAL && tb == 0 && bsw_inflight(ctx) == 0, "a malformed CIGAR task -> %d", rc);
                    rc = bsw_cigar_ref_batch(ctx, &p, ref, cb.data(), 40, MAXC, nullptr, MAXMD, nullptr, cr.data());
                    CHECK(rc == BSW_E_INVAL && b == bsw_last_error(ctx), "the submit says '%s', the batch call '%s'", b.c_str(), bsw_last_error(ctx));
                    cb[23].max_tries = 1;
                    rc = bsw_cigar_ref_submit_t(ctx, &p, ref, cb.data(), 40, MAXC, nullptr, MAXMD, nullptr, cr.data(), &tb);
                    CHECK(rc == BSW_E_LIMIT && tb == 0, "a CIGAR task beyond the limit -> %d", rc);
                    CHECK(bsw_cigar_ref_submit_t(ctx, &p, ref, cb.data(), 40, 0, nullptr, MAXMD, nullptr, cr.data(), &tb) == BSW_E_INVAL, "max_cigar 0");
                }
                bsw_ref_free(ctx, ref);
                bsw_destroy(ctx);
                CHECK(hipdbl::live_objects() == live0, "%d devices: %zu HIP objects left alive after bsw_destroy", G, hipdbl::live_objects() - live0);
                ++cases;
            }
        }
    }
    printf("parity: %zu cases, %llu chunks\n", cases, (unsigned long long)chunks_seen);
    return 0;
}

/* ---- reach: the work of a submit reaches every device ---- */
static int reach_mode()
{
    const bsw_params p = default_params();
    genome1_t g;
    g.make(120001, 31);
    const size_t n = 900;
    for (int kind = 0; kind < 2; ++kind) {
        fresh(2);
        {
            rng_t r(77);
            arena_t arc(n * 300 + 8192, true), arm(n * 400 + 8192, false);
            cwork cw;
            mwork mw;
            make_cigar(cw, arc, g, r, n);
            make_matesw(mw, arm, g, r, n);
            want_t want;
            expected_f4(p, g, cw, mw, want);                      /* (its context makes streams 0 and 1 of the double) */
            uint64_t total = 0;
            {   /* how many chunks the submit is cut into: the same submit on a context nobody stalls (streams 2 .. 5) */
                bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256, 2);
                bsw_ref *ref = upload(ctx, g);
                c_out co;
                std::vector<bsw_mresult> mo;
                const int rc = kind ? submit_c(ctx, p, ref, cw, co, nullptr) : submit_m(ctx, p, ref, mw, mo, nullptr);
                CHECK(rc == BSW_OK && bsw_wait(ctx) == BSW_OK, "the unstalled submit: %s", bsw_last_error(ctx));
                total = stats_of(ctx).chunks;
                bsw_ref_free(ctx, ref);
                bsw_destroy(ctx);
            }
            CHECK(total >= 6, "%llu chunks: the submit is not cut into more chunks than the context has slots", (unsigned long long)total);
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256, 2);   /* streams 6, 7 on device 0 and 8, 9 on device 1 */
            bsw_ref *ref = upload(ctx, g);
            hipdbl::stall_stream(8);
            hipdbl::stall_stream(9);
            c_out co;
            std::vector<bsw_mresult> mo;
            bsw_ticket t = 0;
            const int rc = kind ? submit_c(ctx, p, ref, cw, co, &t) : submit_m(ctx, p, ref, mw, mo, &t);
            CHECK(rc == BSW_OK && t, "the submit -> %d (%s)", rc, bsw_last_error(ctx));
            const uint64_t dev0 = (total + 1) / 2;               /* chunk k -> device k mod 2 */
            const auto t0 = std::chrono::steady_clock::now();
            while (stats_of(ctx).chunks < dev0) {
                CHECK(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(120), "device 0 ran %llu of its %llu chunks", (unsigned long long)stats_of(ctx).chunks, (unsigned long long)dev0);
                std::this_thread::sleep_for(std::chrono::milliseconds(2));
            }
            std::this_thread::sleep_for(std::chrono::milliseconds(50));
            CHECK(bsw_test(ctx, t) == 0, "the submit completed although every stream of device 1 is stalled: its chunks all ran on device 0");
            CHECK(stats_of(ctx).chunks == dev0, "%llu chunks done with device 1 stalled, device 0 owns %llu", (unsigned long long)stats_of(ctx).chunks, (unsigned long long)dev0);
            hipdbl::release_streams();
            CHECK(bsw_wait_ticket(ctx, t) == BSW_OK, "the released submit: %s", bsw_last_error(ctx));
            std::string why;
            if (kind) CHECK(same_c(co, want.c, n, &why), "reach: the CIGAR submit differs: %s", why.c_str());
            else CHECK(same_m(mo, want.m, n), "reach: the rescue submit differs");
            CHECK(stats_of(ctx).chunks == total, "chunks");
            bsw_ref_free(ctx, ref);
            bsw_destroy(ctx);
        }
        CHECK(hipdbl::live_objects() == 0, "reach: %zu HIP objects left", hipdbl::live_objects());
    }
    printf("reach: ok\n");
    return 0;
}

/* ---- mixed: four submits of three kinds in flight ---- */
static int mixed_mode()
{
    const bsw_params p = default_params();
    genome1_t g;
    g.make(120001, 41);
    const size_t n = 700, ne = 900;
    fresh(2);
    {
        rng_t r(99);
        arena_t arc(n * 300 + 8192, false), arm(n * 400 + 8192, true);
        cwork cw;
        mwork mw;
        make_cigar(cw, arc, g, r, n);
        make_matesw(mw, arm, g, r, n);
        want_t want;
        expected_f4(p, g, cw, mw, want);                          /* (streams 0, 1) */
        workload we;
        make_workload(we, ne, 150, 5, true);
        const std::vector<bsw_result> want_e = expected(p, we.tasks.data(), ne);
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256, 2);       /* streams 2 .. 5 */
        bsw_ref *ref = upload(ctx, g);
        for (int k = 2; k < 6; ++k) hipdbl::stall_stream(k);
        std::vector<bsw_result> e1(ne), e2(ne);
        c_out co, co5;
        std::vector<bsw_mresult> mo, mo5;
        bsw_ticket t[4] = {0, 0, 0, 0}, t5 = 55;
        CHECK(bsw_submit_t(ctx, &p, we.tasks.data(), ne, e1.data(), &t[0]) == BSW_OK, "extension submit: %s", bsw_last_error(ctx));
        CHECK(submit_m(ctx, p, ref, mw, mo, &t[1]) == BSW_OK, "rescue submit beside an extension submit: %s", bsw_last_error(ctx));
        CHECK(submit_c(ctx, p, ref, cw, co, &t[2]) == BSW_OK, "CIGAR submit beside two others: %s", bsw_last_error(ctx));
        CHECK(bsw_submit_t(ctx, &p, we.tasks.data(), ne, e2.data(), &t[3]) == BSW_OK, "an extension submit behind the new kinds: %s", bsw_last_error(ctx));
        CHECK(bsw_inflight(ctx) == 4, "bsw_inflight = %d", bsw_inflight(ctx));
        CHECK(submit_m(ctx, p, ref, mw, mo5, &t5) == BSW_E_BUSY && t5 == 0, "a fifth submit (rescue)");
        CHECK(submit_c(ctx, p, ref, cw, co5, &t5) == BSW_E_BUSY && t5 == 0, "a fifth submit (CIGAR)");
        CHECK(bsw_submit_t(ctx, &p, we.tasks.data(), ne, e2.data(), &t5) == BSW_E_BUSY, "a fifth submit (extension)");
        CHECK(bsw_inflight(ctx) == 4, "a refused submit changed bsw_inflight to %d", bsw_inflight(ctx));
        CHECK(bsw_matesw_ref_batch(ctx, &p, ref, mw.t.data(), n, mo5.data()) == BSW_E_BUSY, "the synchronous rescue call with tickets in flight");
        CHECK(bsw_cigar_ref_batch(ctx, &p, ref, cw.t.data(), n, MAXC, nullptr, MAXMD, nullptr, co5.res.data()) == BSW_E_BUSY, "the synchronous CIGAR call with tickets in flight");
        for (int k = 0; k < 4; ++k) CHECK(bsw_test(ctx, t[k]) == 0, "ticket %d is complete behind stalled streams", k);
        hipdbl::release_streams();
        for (int k = 3; k >= 0; --k) {                            /* poll, then collect, newest first */
            const auto t0 = std::chrono::steady_clock::now();
            int s;
            while ((s = bsw_test(ctx, t[k])) == 0) {
                CHECK(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(200), "ticket %d does not complete", k);
                std::this_thread::sleep_for(std::chrono::milliseconds(1));
            }
            CHECK(s == 1, "bsw_test -> %d", s);
            CHECK(bsw_wait_ticket(ctx, t[k]) == BSW_OK, "ticket %d: %s", k, bsw_last_error(ctx));
            CHECK(bsw_inflight(ctx) == k, "bsw_inflight = %d after collecting ticket %d", bsw_inflight(ctx), k);
        }
        same_results(e1.data(), want_e.data(), ne, "mixed: the first extension submit");
        same_results(e2.data(), want_e.data(), ne, "mixed: the second extension submit");
        std::string why;
        CHECK(same_c(co, want.c, n, &why), "mixed: the CIGAR submit differs: %s", why.c_str());
        CHECK(same_m(mo, want.m, n), "mixed: the rescue submit differs");
        sync_m(ctx, p, ref, mw, mo5);                              /* ... and the synchronous calls work again */
        sync_c(ctx, p, ref, cw, co5);
        CHECK(same_m(mo5, want.m, n) && same_c(co5, want.c, n), "mixed: the synchronous calls after the tickets");
        const bsw_stats s = stats_of(ctx);
        CHECK(s.submits == 4 && s.seeds == 2 * ne, "bsw_host_stats: %llu submits, %llu seeds", (unsigned long long)s.submits, (unsigned long long)s.seeds);
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
    }
    CHECK(hipdbl::live_objects() == 0, "mixed: %zu HIP objects left", hipdbl::live_objects());
    printf("mixed: ok\n");
    return 0;
}

/* ---- storm: the scenario of host_tickets.cpp with three kinds of tickets ---- */
static int storm_mode()
{
    const bsw_params p = default_params();
    genome1_t g;
    g.make(90001, 51);
    fresh(2);
    {
        const int T = 8, ROUNDS = 5;
        const size_t n = 260, ne = 500;
        std::vector<std::unique_ptr<arena_t>> ar;
        std::vector<cwork> cw((size_t)T);
        std::vector<mwork> mw((size_t)T);
        std::vector<want_t> want((size_t)T);
        std::vector<std::unique_ptr<workload>> we((size_t)T);
        std::vector<std::vector<bsw_result>> want_e((size_t)T);
        for (int k = 0; k < T; ++k) {
            rng_t r(600 + (uint64_t)k);
            ar.emplace_back(new arena_t(n * 700 + 16384, k % 2 == 0));
            make_cigar(cw[(size_t)k], *ar.back(), g, r, n);
            make_matesw(mw[(size_t)k], *ar.back(), g, r, n);
            expected_f4(p, g, cw[(size_t)k], mw[(size_t)k], want[(size_t)k]);
            we[(size_t)k].reset(new workload());
            make_workload(*we[(size_t)k], ne, 150, 300 + (uint64_t)k, k % 2 == 1);
            want_e[(size_t)k] = expected(p, we[(size_t)k]->tasks.data(), ne);
        }
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256, 2, 60000);
        bsw_ref *ref = upload(ctx, g);
        std::atomic<int> running{T}, busy{0}, stolen{0}, bad{0};
        std::vector<std::thread> th;
        for (int k = 0; k < T; ++k)
            th.emplace_back([&, k]() {
                std::vector<bsw_result> got(ne);
                c_out co;
                std::vector<bsw_mresult> mo;
                for (int r = 0; r < ROUNDS; ++r) {
                    const int kind = (k + r) % 3;
                    bsw_ticket t = 0;
                    int rc;
                    for (;;) {
                        if (kind == 0) { memset(got.data(), 0x5a, ne * sizeof(bsw_result)); rc = bsw_submit_t(ctx, &p, we[(size_t)k]->tasks.data(), ne, got.data(), &t); }
                        else if (kind == 1) rc = submit_m(ctx, p, ref, mw[(size_t)k], mo, &t);
                        else rc = submit_c(ctx, p, ref, cw[(size_t)k], co, &t);
                        if (rc != BSW_E_BUSY) break;
                        ++busy;
                        std::this_thread::sleep_for(std::chrono::microseconds(200));
                    }
                    if (rc != BSW_OK || !t) { ++bad; break; }
                    bool elsewhere = false;
                    if ((r + k) % 2 == 0)
                        for (;;) {
                            const int s = bsw_test(ctx, t);
                            if (s == 1) break;
                            if (s < 0) { elsewhere = true; break; }
                            std::this_thread::sleep_for(std::chrono::microseconds(100));
                        }
                    if (!elsewhere) {
                        rc = bsw_wait_ticket(ctx, t);
                        if (rc == BSW_E_INVAL) elsewhere = true;
                        else if (rc != BSW_OK) { ++bad; break; }
                    }
                    if (elsewhere) ++stolen;
                    const bool ok = kind == 0 ? memcmp(got.data(), want_e[(size_t)k].data(), ne * sizeof(bsw_result)) == 0
                                  : kind == 1 ? same_m(mo, want[(size_t)k].m, n) : same_c(co, want[(size_t)k].c, n);
                    if (!ok) { ++bad; break; }
                }
                --running;
            });
        std::thread sweeper([&]() {
            while (running.load() > 0) {
                const int inflight = bsw_inflight(ctx);
                if (inflight < 0 || inflight > BSW_MAX_INFLIGHT) ++bad;
                if (bsw_wait(ctx) != BSW_OK) ++bad;
                std::this_thread::sleep_for(std::chrono::milliseconds(2));
            }
        });
        for (auto &t : th) t.join();
        sweeper.join();
        CHECK(bad.load() == 0, "%d threads saw a wrong code or wrong results", bad.load());
        CHECK(bsw_wait(ctx) == BSW_OK && bsw_inflight(ctx) == 0, "submits left in flight");
        printf("storm: %d submits, %d answered BSW_E_BUSY first, %d collected by the bsw_wait thread\n", T * ROUNDS, busy.load(), stolen.load());
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
    }
    CHECK(hipdbl::live_objects() == 0, "storm: %zu HIP objects left", hipdbl::live_objects());
    return 0;
}

/* ---- faults: call k of the scenario fails, for every k ---- */
static int faults_mode()
{
    const bsw_params p = default_params();
    genome1_t g;
    g.make(90001, 13);
    const size_t n = 150, ne = 500;
    uint64_t visited = 0, failed = 0, ignored = 0, dead = 0, C = 0;
    for (int reg = 0; reg < 2; ++reg) {
        want_t want;
        std::vector<bsw_result> want_e;
        for (uint64_t k = 0;; ++k) {
            bool made = true;
            fresh(2);
            {
                rng_t r(31);
                arena_t arc(n * 300 + 8192, reg != 0), arm(n * 400 + 8192, reg != 0);
                cwork cw;
                mwork mw;
                make_cigar(cw, arc, g, r, n);
                make_matesw(mw, arm, g, r, n);
                workload we;
                make_workload(we, ne, 150, 9, reg != 0);
                if (k == 0) { expected_f4(p, g, cw, mw, want); want_e = expected(p, we.tasks.data(), ne); }
                const size_t live0 = hipdbl::live_objects();       /* (the registered arenas) */
                bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256, 2, 4000);
                bsw_ref *ref = upload(ctx, g);
                std::vector<bsw_result> eo(ne);
                c_out co;
                std::vector<bsw_mresult> mo;
                memset(eo.data(), 0x5a, ne * sizeof(bsw_result));
                hipdbl::reset_counters();
                if (k) hipdbl::fail_overall(k);
                bsw_ticket t[3] = {0, 0, 0};
                int rs[3];
                rs[0] = bsw_submit_t(ctx, &p, we.tasks.data(), ne, eo.data(), &t[0]);
                rs[1] = submit_m(ctx, p, ref, mw, mo, &t[1]);
                rs[2] = submit_c(ctx, p, ref, cw, co, &t[2]);
                CHECK(rs[0] == BSW_OK && rs[1] == BSW_OK && rs[2] == BSW_OK, "k=%llu: the submits answer %d %d %d (%s)", (unsigned long long)k, rs[0], rs[1], rs[2], bsw_last_error(ctx));
                int rc[3];
                std::string text[3];
                for (int j = 0; j < 3; ++j) {                      /* every ticket completes: a hang ends at the test's time limit */
                    rc[j] = bsw_wait_ticket(ctx, t[j]);
                    text[j] = rc[j] ? bsw_last_error(ctx) : "";
                }
                const char *f = hipdbl::fired();
                const std::string fname = f ? f : "";
                const uint64_t calls = hipdbl::overall_calls();
                hipdbl::clear_failures();
                std::string why;
                const bool ok_e = memcmp(eo.data(), want_e.data(), ne * sizeof(bsw_result)) == 0, ok_m = same_m(mo, want.m, n), ok_c = same_c(co, want.c, n, &why);
                if (rc[0] == BSW_OK) CHECK(ok_e, "k=%llu (%s failed): the extension ticket reports success and its results differ", (unsigned long long)k, fname.c_str());
                if (rc[1] == BSW_OK) CHECK(ok_m, "k=%llu (%s failed): the rescue ticket reports success and its results differ", (unsigned long long)k, fname.c_str());
                if (rc[2] == BSW_OK) CHECK(ok_c, "k=%llu (%s failed): the CIGAR ticket reports success and its results differ: %s", (unsigned long long)k, fname.c_str(), why.c_str());
                const int nfail = (rc[0] != 0) + (rc[1] != 0) + (rc[2] != 0);
                if (k == 0) {
                    C = calls;
                    CHECK(nfail == 0, "the clean scenario -> %d %d %d", rc[0], rc[1], rc[2]);
                    CHECK(stats_of(ctx).chunks >= 8, "the scenario's submits are cut into %llu chunks", (unsigned long long)stats_of(ctx).chunks);
                    printf("faults, %s memory: C = %llu\n", reg ? "registered" : "pageable", (unsigned long long)C);
                } else if (!f) {
                    /* (the number of calls varies a little with the threads' timing — a slot that finds its queue empty hands its
                     * chunk over at once, one that does not records an event first: the sweep ends at the first k this run did not reach) */
                    CHECK(k > calls && 10 * k > 9 * C, "call %llu of the scenario was never made (this run made %llu, the clean one %llu)", (unsigned long long)k, (unsigned long long)calls, (unsigned long long)C);
                    CHECK(nfail == 0, "k=%llu: no failure happened and a ticket failed", (unsigned long long)k);
                    made = false;
                } else {
                    ++visited;
                    if (nfail) {
                        ++failed;
                        const bool alloc = fname == "hipMalloc" || fname == "hipHostMalloc";
                        for (int j = 0; j < 3; ++j)
                            if (rc[j]) {
                                CHECK(rc[j] == BSW_E_HIP || (alloc && rc[j] == BSW_E_NOMEM), "k=%llu: %s failed and ticket %d answered %d (%s)", (unsigned long long)k, fname.c_str(), j, rc[j], text[j].c_str());
                                CHECK(!text[j].empty(), "k=%llu: %s failed, ticket %d answered %d without a text", (unsigned long long)k, fname.c_str(), j, rc[j]);
                                CHECK(text[j].compare(0, 7, "aborted") != 0, "k=%llu: ticket %d reports '%s', not the failure itself", (unsigned long long)k, j, text[j].c_str());
                            }
                    } else {
                        ++ignored;                                 /* (a release whose return code is ignored by design) */
                        CHECK(fname == "hipFree" || fname == "hipHostFree" || fname == "hipGetLastError", "k=%llu: %s failed and every ticket reported success", (unsigned long long)k, fname.c_str());
                    }
                }
                CHECK(bsw_inflight(ctx) == 0, "tickets left");
                /* a context that is not dead accepts and completes a further submit of every kind */
                c_out co2;
                std::vector<bsw_mresult> mo2;
                bsw_ticket t2[3] = {0, 0, 0};
                const int r2 = submit_m(ctx, p, ref, mw, mo2, &t2[1]);
                bool is_dead = false;
                if (r2 == BSW_E_HIP && strstr(bsw_last_error(ctx), "dead")) { is_dead = true; ++dead; }
                else {
                    CHECK(r2 == BSW_OK, "k=%llu (%s failed): a further rescue submit -> %d (%s)", (unsigned long long)k, fname.c_str(), r2, bsw_last_error(ctx));
                    CHECK(submit_c(ctx, p, ref, cw, co2, &t2[2]) == BSW_OK, "k=%llu: a further CIGAR submit: %s", (unsigned long long)k, bsw_last_error(ctx));
                    memset(eo.data(), 0x5a, ne * sizeof(bsw_result));
                    CHECK(bsw_submit_t(ctx, &p, we.tasks.data(), ne, eo.data(), &t2[0]) == BSW_OK, "k=%llu: a further extension submit: %s", (unsigned long long)k, bsw_last_error(ctx));
                    const int w2 = bsw_wait(ctx);
                    CHECK(w2 == BSW_OK, "k=%llu (%s failed): the further submits -> %d (%s)", (unsigned long long)k, fname.c_str(), w2, bsw_last_error(ctx));
                    CHECK(same_m(mo2, want.m, n) && same_c(co2, want.c, n, &why) && memcmp(eo.data(), want_e.data(), ne * sizeof(bsw_result)) == 0,
                          "k=%llu (%s failed): the further submits are not bit-exact (%s)", (unsigned long long)k, fname.c_str(), why.c_str());
                }
                CHECK(!is_dead || nfail, "k=%llu: the context is dead and no ticket failed", (unsigned long long)k);
                bsw_ref_free(ctx, ref);
                bsw_destroy(ctx);
                if (!is_dead) CHECK(hipdbl::live_objects() == live0, "k=%llu (%s failed): %zu HIP objects left alive after bsw_destroy", (unsigned long long)k, fname.c_str(), hipdbl::live_objects() - live0);
            }
            if (!made) break;
        }
    }
    printf("faults: injection points visited = %llu, a ticket failed %llu times, ignored releases %llu, dead contexts %llu\n", (unsigned long long)visited,
           (unsigned long long)failed, (unsigned long long)ignored, (unsigned long long)dead);
    CHECK(visited >= 150 && failed >= 100, "the sweep visited %llu calls", (unsigned long long)visited);
    return 0;
}

/* ---- watchdog ---- */
static int watchdog_mode()
{
    const bsw_params p = default_params();
    genome1_t g;
    g.make(90001, 61);
    const size_t n = 300;
    for (int kind = 0; kind < 2; ++kind) {
        fresh(1);
        {
            rng_t r(5);
            arena_t arc(n * 300 + 8192, false), arm(n * 400 + 8192, false);
            cwork cw;
            mwork mw;
            make_cigar(cw, arc, g, r, n);
            make_matesw(mw, arm, g, r, n);
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2, 300);
            bsw_ref *ref = upload(ctx, g);
            hipdbl::stall_stream(0);
            hipdbl::stall_stream(1);
            c_out co;
            std::vector<bsw_mresult> mo;
            bsw_ticket t = 0;
            int rc = kind ? submit_c(ctx, p, ref, cw, co, &t) : submit_m(ctx, p, ref, mw, mo, &t);
            CHECK(rc == BSW_OK && t, "the submit -> %d", rc);
            const auto t0 = std::chrono::steady_clock::now();
            rc = bsw_wait_ticket(ctx, t);
            CHECK(rc == BSW_E_HIP && strstr(bsw_last_error(ctx), "timeout"), "bsw_wait_ticket behind a stalled stream -> %d (%s)", rc, bsw_last_error(ctx));
            CHECK(std::chrono::steady_clock::now() - t0 < std::chrono::seconds(20), "the watchdog of 300 ms took too long");
            CHECK(bsw_inflight(ctx) == 0, "tickets in flight on the dead context");
            rc = kind ? submit_c(ctx, p, ref, cw, co, &t) : submit_m(ctx, p, ref, mw, mo, &t);
            CHECK(rc == BSW_E_HIP && t == 0 && strstr(bsw_last_error(ctx), "dead"), "a further submit on the dead context -> %d (%s)", rc, bsw_last_error(ctx));
            m_init(mo, n);
            rc = bsw_matesw_ref_batch(ctx, &p, ref, mw.t.data(), n, mo.data());
            CHECK(rc == BSW_E_HIP && strstr(bsw_last_error(ctx), "dead"), "the synchronous call on the dead context -> %d", rc);
            /* What was queued behind the stall still runs once released: it reads the pinned staging and the device buffers a dead
             * context leaves behind on purpose, and the reference copy — which therefore stays allocated until the double has
             * joined its stream workers (fresh); its handle is kept reachable instead of freed. */
            hipdbl::release_streams();
            bsw_destroy(ctx);
            fresh(1);
            static bsw_ref *kept[2];
            kept[kind] = ref;
        }
    }
    printf("watchdog: ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    /* small work targets: the submits of these workloads are cut into more chunks than the contexts have slots */
    setenv("BSW_F4_MATESW_WORK", "400000", 1);
    setenv("BSW_F4_CIGAR_WORK", "150000", 1);
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "parity") return parity_mode();
    if (mode == "reach") return reach_mode();
    if (mode == "mixed") return mixed_mode();
    if (mode == "storm") return storm_mode();
    if (mode == "faults") return faults_mode();
    if (mode == "watchdog") return watchdog_mode();
    fprintf(stderr, "usage: host_f4_stream parity|reach|mixed|storm|faults|watchdog\n");
    return 2;
}
