/* host_faults.cpp — every single HIP failure (TEST INFRASTRUCTURE; tests/test_host_double_cpu.py).  The failures are return codes
 * of the host-memory stand-in in a process that never opens a GPU.
 *
 *   host_faults sweep I M    the scenario below with call k failing, for every k = I (mod M) until no call k is made any more
 *   host_faults create       every call of bsw_create failing in turn: partial construction must unwind
 *   host_faults ref_upload   every call of bsw_ref_upload on three devices failing in turn
 *
 * The scenario: two devices, two slots each, three submits in flight (host sequences, packed, resident reference) of four chunks
 * each; they are waited for one by one, a further submit follows on the same context, then the reference and the context are
 * released.  A clean run makes C counted calls (hipdbl::overall_calls) after bsw_create and bsw_ref_upload have returned.
 */
#include <chrono>
#include "host_common.h"

static const size_t N = 1024;                        /* 4 chunks of 256 */
static const double LIMIT_S = 20.0;                  /* one wait; the context's watchdog is 3 s */

struct refw {
    std::vector<uint8_t> pac;
    int64_t l_pac = 40001;
    std::vector<bsw_ref_task> rt;
    uint8_t *arena = nullptr;
    std::vector<bsw_task> tasks;
    std::vector<uint8_t> seqs;
    ~refw() { bsw_host_free(arena); }
};

static void make_refw(refw &w, const bsw_params &p, size_t n)
{
    bsw_synth_spec sp;
    memset(&sp, 0, sizeof(sp));
    sp.seed = 99; sp.read_len = 150; sp.seed_len_min = 19; sp.seed_len_max = 40; sp.sub_rate = 0.03; sp.indel_rate = 0.008;
    sp.n_rate = 0.004; sp.junk_frac = 0.1; sp.a = 1; sp.w = 100; sp.o = 6; sp.e = 1;
    w.pac.assign((size_t)((w.l_pac + 3) >> 2), 0);
    w.rt.resize(n);
    const size_t alen = n * 150 + 64;
    w.arena = (uint8_t *)bsw_host_alloc(alen);
    memset(w.arena, 0, alen);
    CHECK(bsw_synth_ref_generate(&sp, &p, w.l_pac, w.pac.data(), n, w.rt.data(), w.arena, alen) >= 0, "bsw_synth_ref_generate");
    size_t need = 0;
    for (size_t i = 0; i < n; ++i) need += (size_t)(w.rt[i].rmax1 - w.rt[i].rmax0) + bsw_seed_scratch_bytes(&w.rt[i].seed, w.rt[i].rmax0) + 16;
    w.seqs.assign(need + 16, 0);
    w.tasks.resize(n);
    size_t at = 0;
    for (size_t i = 0; i < n; ++i) {
        bsw_ref_task &r = w.rt[i];
        r.tag = (uint32_t)i;
        uint8_t *rseq = w.seqs.data() + at;
        at += (size_t)bsw_pac_get_seq(w.l_pac, w.pac.data(), r.rmax0, r.rmax1, rseq);
        const size_t sl = bsw_seed_scratch_bytes(&r.seed, r.rmax0);
        CHECK(bsw_seed_to_task(&p, &r.seed, r.l_query, r.query, r.rmax0, r.rmax1, rseq, w.seqs.data() + at, sl, r.tag, &w.tasks[i]) == BSW_OK, "bsw_seed_to_task");
        w.tasks[i].init_score = r.init_score;
        at += sl;
    }
}

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static bool is_release(const char *name)
{
    for (const char *r : {"hipFree", "hipHostFree", "hipEventDestroy", "hipStreamDestroy", "hipHostUnregister", "hipGetLastError"})
        if (!strcmp(name, r)) return true;
    return false;
}
static bool is_alloc(const char *name) { return !strcmp(name, "hipMalloc") || !strcmp(name, "hipHostMalloc"); }

static bool names_a_step(const char *msg)
{
    for (const char *w : {"staging", "DMA", "hip", "launch", "timeout", "memset"})
        if (strstr(msg, w)) return true;
    return false;
}

struct wants_t { std::vector<bsw_result> a, b, r; };

struct outcome { uint64_t calls = 0; const char *fired = nullptr; int phase = 0; int failed = 0; };

/* k = 0: clean */
static outcome scenario(uint64_t k, wants_t &wants, bool first)
{
    outcome oc;
    fresh(2);
    {
        bsw_params p;
        bsw_default_params(&p);
        workload wa, wb;
        refw wr;
        make_workload(wa, N, 150, 1001, true);
        make_workload(wb, N, 150, 1002, true);
        make_refw(wr, p, N);
        if (first) {
            wants.a = expected(p, wa.tasks.data(), N);
            wants.b = expected(p, wb.tasks.data(), N);
            wants.r = expected(p, wr.tasks.data(), N);
        }
        const size_t cap = bsw_pack_tasks_bound(wb.tasks.data(), N);
        uint64_t *parena = (uint64_t *)bsw_host_alloc(cap);
        std::vector<bsw_task> pt(N);
        CHECK(bsw_pack_tasks(wb.tasks.data(), N, parena, cap, pt.data()) >= 0, "bsw_pack_tasks");
        bsw_result *oa = (bsw_result *)bsw_host_alloc(N * sizeof(bsw_result));
        std::vector<bsw_result> ob(N), orr(N), of(N);

        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256, 2, 3000);
        bsw_ref *ref = nullptr;
        CHECK(bsw_ref_upload(ctx, wr.pac.data(), wr.l_pac, &ref) == BSW_OK, "bsw_ref_upload: %s", bsw_last_error(ctx));
        hipdbl::reset_counters();
        if (k) hipdbl::fail_overall(k);

        /* phase 1: three submits in flight */
        bsw_ticket t[3] = {0, 0, 0};
        int rc = bsw_submit_t(ctx, &p, wa.tasks.data(), N, oa, &t[0]);
        CHECK(rc == BSW_OK, "k=%llu: bsw_submit_t -> %d (%s)", (unsigned long long)k, rc, bsw_last_error(ctx));
        rc = bsw_submit_packed_t(ctx, &p, pt.data(), N, ob.data(), &t[1]);
        CHECK(rc == BSW_OK, "k=%llu: bsw_submit_packed_t -> %d (%s)", (unsigned long long)k, rc, bsw_last_error(ctx));
        rc = bsw_submit_ref_t(ctx, &p, ref, wr.rt.data(), N, orr.data(), &t[2]);
        CHECK(rc == BSW_OK, "k=%llu: bsw_submit_ref_t -> %d (%s)", (unsigned long long)k, rc, bsw_last_error(ctx));
        const bsw_result *got[3] = {oa, ob.data(), orr.data()};
        const std::vector<bsw_result> *want[3] = {&wants.a, &wants.b, &wants.r};
        bool alloc_seen = false;
        for (int i = 0; i < 3; ++i) {
            const double t0 = now_s();
            rc = bsw_wait_ticket(ctx, t[i]);
            CHECK(now_s() - t0 < LIMIT_S, "k=%llu: bsw_wait_ticket(%d) took %.1f s", (unsigned long long)k, i, now_s() - t0);
            if (rc == BSW_OK) same_results(got[i], want[i]->data(), N, "a ticket that reported success");
            else {
                ++oc.failed;
                const char *msg = bsw_last_error(ctx);
                CHECK(rc == BSW_E_NOMEM || rc == BSW_E_HIP, "k=%llu: ticket %d -> %d (%s)", (unsigned long long)k, i, rc, msg);
                CHECK(msg && *msg && names_a_step(msg), "k=%llu: ticket %d failed with %d and the text '%s' names no step", (unsigned long long)k, i, rc, msg ? msg : "(null)");
                CHECK(!strstr(msg, "aborted"), "k=%llu: ticket %d reports the chunks that gave up ('%s'), not the failure itself", (unsigned long long)k, i, msg);
                alloc_seen = alloc_seen || rc == BSW_E_NOMEM;
            }
        }
        CHECK(bsw_inflight(ctx) == 0, "k=%llu: %d submits in flight after every ticket was collected", (unsigned long long)k, bsw_inflight(ctx));
        const char *f1 = hipdbl::fired();
        if (f1) {
            oc.phase = 1;
            CHECK(oc.failed <= 1, "k=%llu (%s): one failing call failed %d tickets", (unsigned long long)k, f1, oc.failed);
            if (!is_release(f1)) CHECK(oc.failed == 1, "k=%llu: %s failed and every ticket reported success", (unsigned long long)k, f1);
            else CHECK(oc.failed == 0, "k=%llu: a failing %s (return code ignored by design) failed a ticket", (unsigned long long)k, f1);
            if (oc.failed) CHECK(alloc_seen == is_alloc(f1), "k=%llu: %s failed, the ticket answered %s", (unsigned long long)k, f1, alloc_seen ? "BSW_E_NOMEM" : "BSW_E_HIP");
        } else
            CHECK(oc.failed == 0, "k=%llu: no planned failure has happened, yet %d tickets failed (%s)", (unsigned long long)k, oc.failed, bsw_last_error(ctx));

        /* phase 2: the context after the failure.  An injected return code never kills it (only the watchdog does): the
         * next submit must be bit-exact */
        bsw_ticket tf = 0;
        rc = bsw_submit_t(ctx, &p, wa.tasks.data(), N, of.data(), &tf);
        CHECK(rc == BSW_OK, "k=%llu: a further submit -> %d (%s)", (unsigned long long)k, rc, bsw_last_error(ctx));
        const double t0 = now_s();
        rc = bsw_wait_ticket(ctx, tf);
        CHECK(now_s() - t0 < LIMIT_S, "k=%llu: the further submit's wait took %.1f s", (unsigned long long)k, now_s() - t0);
        const char *f2 = hipdbl::fired();
        if (oc.phase == 1 || !f2 || is_release(f2)) {
            CHECK(rc == BSW_OK, "k=%llu (%s failed earlier): a further submit on the same context -> %d (%s)", (unsigned long long)k, f1 ? f1 : "nothing", rc, bsw_last_error(ctx));
            same_results(of.data(), wants.a.data(), N, "the further submit");
        } else {
            oc.phase = 2;
            CHECK(rc == (is_alloc(f2) ? BSW_E_NOMEM : BSW_E_HIP), "k=%llu: %s failed in the further submit, its ticket answered %d (%s)", (unsigned long long)k, f2, rc, bsw_last_error(ctx));
            ++oc.failed;
        }
        CHECK(bsw_inflight(ctx) == 0, "k=%llu: submits left in flight", (unsigned long long)k);
        /* phase 3: release */
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
        oc.calls = hipdbl::overall_calls();
        oc.fired = hipdbl::fired();
        if (oc.fired && !oc.phase) oc.phase = 3;
        hipdbl::clear_failures();
        bsw_host_free(parena);
        bsw_host_free(oa);
    }
    CHECK(hipdbl::live_objects() == 0, "k=%llu: %zu HIP objects left alive after bsw_destroy", (unsigned long long)k, hipdbl::live_objects());
    return oc;
}

static int sweep(uint64_t part, uint64_t parts)
{
    wants_t wants;
    const outcome clean = scenario(0, wants, true);
    CHECK(!clean.fired && !clean.failed, "the clean run failed");
    const uint64_t C = clean.calls;
    printf("sweep: C = %llu calls in the clean scenario\n", (unsigned long long)C);
    uint64_t visited = 0, fired = 0, by_phase[4] = {0, 0, 0, 0}, failed_tickets = 0, last_fired = 0;
    int misses = 0;
    for (uint64_t k = 1 + part; misses < 3; k += parts) {
        printf("k=%llu\n", (unsigned long long)k);
        fflush(stdout);
        const outcome oc = scenario(k, wants, false);
        ++visited;
        if (oc.fired) { ++fired; ++by_phase[oc.phase]; failed_tickets += (uint64_t)oc.failed; last_fired = k; misses = 0; }
        else {
            /* (how many calls a run makes depends a little on timing: whether a slot found its previous chunk still pending) */
            CHECK(k + 16 > C, "call %llu was never made although the clean run made %llu", (unsigned long long)k, (unsigned long long)C);
            ++misses;
        }
    }
    CHECK(last_fired + 16 > C, "the sweep ended at call %llu, the clean run made %llu", (unsigned long long)last_fired, (unsigned long long)C);
    printf("sweep part %llu/%llu: C = %llu, injection points visited = %llu, fired = %llu (submits %llu, further submit %llu, release %llu), failed tickets %llu, skipped 0\n",
           (unsigned long long)part, (unsigned long long)parts, (unsigned long long)C, (unsigned long long)visited, (unsigned long long)fired,
           (unsigned long long)by_phase[1], (unsigned long long)by_phase[2], (unsigned long long)by_phase[3], (unsigned long long)failed_tickets);
    return 0;
}

/* ---- bsw_create ---- */
static int create_sweep()
{
    bsw_params p;
    bsw_default_params(&p);
    uint64_t C = 0, refused = 0, degraded = 0;
    for (uint64_t k = 0;; ++k) {
        fresh(3);
        {
            workload w;
            make_workload(w, 600, 150, 7, false);
            const std::vector<bsw_result> want = expected(p, w.tasks.data(), 600);
            bsw_config c;
            bsw_default_config(&c);
            c.streams = 3; c.chunk_tasks = 256; c.timeout_ms = 3000; c.n_devices = 3; c.devices[0] = 0; c.devices[1] = 1; c.devices[2] = 2;
            if (k) hipdbl::fail_overall(k);
            bsw_ctx *ctx = nullptr;
            const int rc = bsw_create(&c, &ctx);
            const char *f = hipdbl::fired();
            if (k == 0) { C = hipdbl::overall_calls(); CHECK(rc == BSW_OK, "clean bsw_create -> %d", rc); printf("create: C = %llu\n", (unsigned long long)C); }
            hipdbl::clear_failures();
            if (k && !f) { CHECK(k > C, "call %llu of bsw_create was never made (C = %llu)", (unsigned long long)k, (unsigned long long)C); if (ctx) bsw_destroy(ctx); break; }
            if (rc != BSW_OK) {
                ++refused;
                CHECK(!ctx, "k=%llu: bsw_create failed with %d and handed out a context", (unsigned long long)k, rc);
                CHECK(rc == BSW_E_HIP || rc == BSW_E_NODEVICE, "k=%llu (%s): bsw_create -> %d", (unsigned long long)k, f, rc);
            } else {
                /* the optional machinery (fork events, chain flags, PCI placement) may fail: the context works without it */
                if (k) ++degraded;
                std::vector<bsw_result> got(600);
                int r2 = bsw_submit(ctx, &p, w.tasks.data(), 600, got.data());
                if (!r2) r2 = bsw_wait(ctx);
                CHECK(r2 == BSW_OK, "k=%llu (%s): a context created in spite of the failure cannot run: %d (%s)", (unsigned long long)k, f ? f : "-", r2, bsw_last_error(ctx));
                same_results(got.data(), want.data(), 600, "after a degraded bsw_create");
                bsw_dev_batch *b = nullptr;
                r2 = bsw_upload(ctx, &p, w.tasks.data(), 600, &b);
                if (!r2) r2 = bsw_run(ctx, b);
                if (!r2) r2 = bsw_download(ctx, b, got.data());
                CHECK(r2 == BSW_OK, "k=%llu: resident batch on a degraded context: %d (%s)", (unsigned long long)k, r2, bsw_last_error(ctx));
                same_results(got.data(), want.data(), 600, "resident batch after a degraded bsw_create");
                bsw_free_batch(ctx, b);
                bsw_destroy(ctx);
            }
        }
        CHECK(hipdbl::live_objects() == 0, "k=%llu: bsw_create left %zu HIP objects behind", (unsigned long long)k, hipdbl::live_objects());
    }
    printf("create sweep: C = %llu, injection points visited = %llu, refused %llu, created without the optional part %llu, skipped 0\n",
           (unsigned long long)C, (unsigned long long)C, (unsigned long long)refused, (unsigned long long)degraded);
    CHECK(refused + degraded == C, "visited %llu of %llu", (unsigned long long)(refused + degraded), (unsigned long long)C);
    return 0;
}

/* ---- bsw_ref_upload ---- */
static int ref_upload_sweep()
{
    uint64_t C = 0, visited = 0;
    std::vector<uint8_t> pac(5000, 0x1b);
    for (uint64_t k = 0;; ++k) {
        fresh(3);
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 3, 256, 2, 3000);
        const size_t before = hipdbl::live_objects();
        hipdbl::reset_counters();
        if (k) hipdbl::fail_overall(k);
        bsw_ref *ref = nullptr;
        const int rc = bsw_ref_upload(ctx, pac.data(), 19999, &ref);
        const char *f = hipdbl::fired();
        if (k == 0) { C = hipdbl::overall_calls(); CHECK(rc == BSW_OK && ref, "clean bsw_ref_upload -> %d", rc); printf("ref_upload: C = %llu\n", (unsigned long long)C); }
        hipdbl::clear_failures();
        if (k && !f) { CHECK(k > C, "call %llu was never made", (unsigned long long)k); bsw_ref_free(ctx, ref); bsw_destroy(ctx); break; }
        if (k) {
            ++visited;
            if (rc != BSW_OK) {
                CHECK(!ref && rc == BSW_E_HIP && *bsw_last_error(ctx), "k=%llu (%s): bsw_ref_upload -> %d, ref %p", (unsigned long long)k, f, rc, (void *)ref);
                CHECK(hipdbl::live_objects() == before, "k=%llu (%s): a failed bsw_ref_upload left %zu allocations behind", (unsigned long long)k, f, hipdbl::live_objects() - before);
            }
        }
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
        CHECK(hipdbl::live_objects() == 0, "k=%llu: %zu HIP objects left", (unsigned long long)k, hipdbl::live_objects());
    }
    printf("ref_upload sweep: C = %llu, injection points visited = %llu, skipped 0\n", (unsigned long long)C, (unsigned long long)visited);
    CHECK(visited == C, "visited %llu of %llu", (unsigned long long)visited, (unsigned long long)C);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "sweep" && argc > 3) return sweep(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
    if (mode == "create") return create_sweep();
    if (mode == "ref_upload") return ref_upload_sweep();
    fprintf(stderr, "usage: host_faults sweep I M | create | ref_upload\n");
    return 2;
}
