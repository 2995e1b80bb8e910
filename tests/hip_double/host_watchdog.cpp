/* host_watchdog.cpp — the watchdog that marks a context dead (TEST INFRASTRUCTURE; tests/test_host_double_cpu.py).  A stream of
 * the host-memory stand-in is made to sleep; no device is involved.
 *   host_watchdog stall    a stalled stream under a resident batch and under a submit; another context is unaffected
 *   host_watchdog chain    BSW_CHAIN_SELFTEST=1 (set by the caller): every wait of the launch chain expires, bsw_chain_timeouts
 *                          counts exactly those
 */
#include <chrono>
#include "host_common.h"

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static int stall_mode()
{
    fresh(1);
    bsw_params p;
    bsw_default_params(&p);
    {
        workload w;
        make_workload(w, 1500, 150, 5, false);
        const std::vector<bsw_result> want = expected(p, w.tasks.data(), 1500);
        std::vector<bsw_result> got(1500), got2(1500), gotb(1500);
        /* context A: resident path (streams 0 and 1 of the double); context B: streaming (2, 3); context C: healthy (4, 5) */
        bsw_ctx *A = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2, 300);
        bsw_ctx *Bc = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2, 300);
        bsw_ctx *C = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2, 20000);
        hipdbl::stall_stream(0);
        hipdbl::stall_stream(2);

        bsw_dev_batch *b = nullptr;
        double t0 = now_s();
        int rc = bsw_upload(A, &p, w.tasks.data(), 1500, &b);
        CHECK(rc == BSW_E_HIP && !b, "bsw_upload on a stalled stream -> %d", rc);
        CHECK(strstr(bsw_last_error(A), "timeout"), "the text '%s' does not say timeout", bsw_last_error(A));
        CHECK(now_s() - t0 < 10.0, "the watchdog of 300 ms took %.1f s", now_s() - t0);
        rc = bsw_upload(A, &p, w.tasks.data(), 1500, &b);
        CHECK(rc == BSW_E_HIP && strstr(bsw_last_error(A), "dead"), "a later call on the dead context -> %d (%s)", rc, bsw_last_error(A));
        rc = bsw_submit(A, &p, w.tasks.data(), 1500, got.data());
        CHECK(rc == BSW_E_HIP && strstr(bsw_last_error(A), "dead"), "bsw_submit on the dead context -> %d (%s)", rc, bsw_last_error(A));
        uint64_t nto = 0;
        CHECK(bsw_chain_timeouts(A, &nto) == BSW_E_HIP, "bsw_chain_timeouts on the dead context");
        CHECK(bsw_sync(A) == BSW_E_HIP, "bsw_sync on the dead context");

        bsw_ticket t = 0;
        rc = bsw_submit_t(Bc, &p, w.tasks.data(), 1500, got2.data(), &t);
        CHECK(rc == BSW_OK, "bsw_submit_t -> %d", rc);
        t0 = now_s();
        rc = bsw_wait_ticket(Bc, t);
        CHECK(rc == BSW_E_HIP && strstr(bsw_last_error(Bc), "timeout"), "bsw_wait_ticket behind a stalled stream -> %d (%s)", rc, bsw_last_error(Bc));
        CHECK(now_s() - t0 < 20.0, "the wait took %.1f s", now_s() - t0);
        CHECK(bsw_inflight(Bc) == 0, "submits in flight on the dead context");
        rc = bsw_submit_t(Bc, &p, w.tasks.data(), 1500, got2.data(), &t);
        CHECK(rc == BSW_E_HIP && t == 0 && strstr(bsw_last_error(Bc), "dead"), "a further submit on the dead context -> %d (%s)", rc, bsw_last_error(Bc));

        /* another context of the process */
        rc = bsw_submit(C, &p, w.tasks.data(), 1500, gotb.data());
        if (!rc) rc = bsw_wait(C);
        CHECK(rc == BSW_OK, "the healthy context -> %d (%s)", rc, bsw_last_error(C));
        same_results(gotb.data(), want.data(), 1500, "the healthy context beside two dead ones");
        CHECK(bsw_chain_timeouts(C, &nto) == BSW_OK && nto == 0, "bsw_chain_timeouts on the healthy context: %llu", (unsigned long long)nto);

        hipdbl::release_streams();
        bsw_destroy(A);
        bsw_destroy(Bc);
        bsw_destroy(C);
        fresh(1);                                    /* (a dead context leaves its streams and buffers behind on purpose; drains what was stalled) */
    }
    printf("watchdog: ok\n");
    return 0;
}

static int chain_mode()
{
    fresh(1);
    bsw_params p;
    bsw_default_params(&p);
    {
        /* 250 bp reads under BSW_KERNEL_LANE as a resident batch: lane launches of two 8-bit classes, chained over the slot streams */
        workload w;
        make_workload(w, 3000, 250, 17, false);
        const std::vector<bsw_result> want = expected(p, w.tasks.data(), 3000);
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_LANE, 1, 0, 4, 20000);
        bsw_dev_batch *b = nullptr;
        int rc = bsw_upload(ctx, &p, w.tasks.data(), 3000, &b);
        if (!rc) rc = bsw_run(ctx, b);
        std::vector<bsw_result> got(3000);
        if (!rc) rc = bsw_download(ctx, b, got.data());
        CHECK(rc == BSW_OK, "chain: %d (%s)", rc, bsw_last_error(ctx));
        same_results(got.data(), want.data(), 3000, "a chain whose every wait expires");
        uint64_t nto = 0;
        CHECK(bsw_chain_timeouts(ctx, &nto) == BSW_OK, "bsw_chain_timeouts: %s", bsw_last_error(ctx));
        const uint64_t waits = standin::chain_waits();
        printf("chain: %llu waits queued, %llu expired\n", (unsigned long long)waits, (unsigned long long)nto);
        CHECK(waits > 0, "the batch did not run as a launch chain");
        /* (without the self-test a wait may still expire here: a stand-in raises its flag when its launch is DONE, not when its last
         * workgroup has started, and the oracle may need more than the wait's 20 ms) */
        CHECK(getenv("BSW_CHAIN_SELFTEST") ? nto == waits : nto <= waits, "bsw_chain_timeouts says %llu, %llu waits were queued", (unsigned long long)nto, (unsigned long long)waits);
        bsw_free_batch(ctx, b);
        bsw_destroy(ctx);
    }
    CHECK(hipdbl::live_objects() == 0, "chain: %zu HIP objects left", hipdbl::live_objects());
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "stall") return stall_mode();
    if (mode == "chain") return chain_mode();
    fprintf(stderr, "usage: host_watchdog stall|chain\n");
    return 2;
}
