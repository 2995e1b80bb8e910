/* host_tickets.cpp — the threading contract of the ticket calls (include/bwa_sw_mi355.h, "THREADS"), meant for the TSan build and
 * run under ASan too (TEST INFRASTRUCTURE; tests/test_host_double_cpu.py).
 *   storm     8 threads share one context; each submits, polls with bsw_test, collects with bsw_wait_ticket and checks its own
 *             results, BSW_E_BUSY retried, while a ninth thread keeps calling bsw_wait and bsw_inflight
 *   collide   a thread blocked in bsw_wait_ticket while bsw_wait collects its ticket: BSW_E_INVAL or the ticket's own code
 */
#include <atomic>
#include <chrono>
#include "host_common.h"

static int storm()
{
    fresh(2);
    bsw_params p;
    bsw_default_params(&p);
    {
        const int T = 8, ROUNDS = 6;
        const size_t n = 700;
        std::vector<std::unique_ptr<workload>> w((size_t)T);
        std::vector<std::vector<bsw_result>> want((size_t)T);
        for (int k = 0; k < T; ++k) {
            w[(size_t)k].reset(new workload());
            make_workload(*w[(size_t)k], n, 150, 300 + (uint64_t)k, k % 2 == 0);
            want[(size_t)k] = expected(p, w[(size_t)k]->tasks.data(), n);
        }
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256, 2, 20000);
        std::atomic<int> running{T}, busy{0}, stolen{0}, bad{0};
        std::vector<std::thread> th;
        for (int k = 0; k < T; ++k)
            th.emplace_back([&, k]() {
                std::vector<bsw_result> got(n);
                for (int r = 0; r < ROUNDS; ++r) {
                    memset(got.data(), 0x5a, n * sizeof(bsw_result));
                    bsw_ticket t = 0;
                    int rc;
                    while ((rc = bsw_submit_t(ctx, &p, w[(size_t)k]->tasks.data(), n, got.data(), &t)) == BSW_E_BUSY) { ++busy; std::this_thread::sleep_for(std::chrono::microseconds(200)); }
                    if (rc != BSW_OK || !t) { ++bad; break; }
                    bool collected_elsewhere = false;
                    if ((r + k) % 2 == 0)
                        for (;;) {
                            const int s = bsw_test(ctx, t);
                            if (s == 1) break;
                            if (s < 0) { collected_elsewhere = true; break; }     /* bsw_wait took it: complete */
                            std::this_thread::sleep_for(std::chrono::microseconds(100));
                        }
                    if (!collected_elsewhere) {
                        rc = bsw_wait_ticket(ctx, t);
                        if (rc == BSW_E_INVAL) collected_elsewhere = true;
                        else if (rc != BSW_OK) { ++bad; break; }
                    }
                    if (collected_elsewhere) ++stolen;
                    if (memcmp(got.data(), want[(size_t)k].data(), n * sizeof(bsw_result)) != 0) { ++bad; break; }
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
        bsw_destroy(ctx);
    }
    CHECK(hipdbl::live_objects() == 0, "storm: %zu HIP objects left", hipdbl::live_objects());
    return 0;
}

static int collide()
{
    int invals = 0, owns = 0;
    for (int round = 0; round < 24; ++round) {
        fresh(1);
        bsw_params p;
        bsw_default_params(&p);
        {
            workload w;
            make_workload(w, 300, 150, 40 + (uint64_t)round, false);
            const std::vector<bsw_result> want = expected(p, w.tasks.data(), 300);
            std::vector<bsw_result> got(300);
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2, 20000);
            hipdbl::stall_stream(0);
            hipdbl::stall_stream(1);
            bsw_ticket t = 0;
            CHECK(bsw_submit_t(ctx, &p, w.tasks.data(), 300, got.data(), &t) == BSW_OK, "bsw_submit_t");
            int rc_a = 1, rc_b = 1;
            std::thread a([&]() { rc_a = bsw_wait_ticket(ctx, t); });
            std::thread b([&]() { if (round % 2) std::this_thread::sleep_for(std::chrono::milliseconds(3)); rc_b = bsw_wait(ctx); });
            std::this_thread::sleep_for(std::chrono::milliseconds(20));
            CHECK(bsw_test(ctx, t) == 0, "the submit completed behind stalled streams");
            hipdbl::release_streams();
            a.join();
            b.join();
            CHECK(rc_b == BSW_OK, "bsw_wait -> %d", rc_b);
            CHECK(rc_a == BSW_OK || rc_a == BSW_E_INVAL, "bsw_wait_ticket on a ticket that bsw_wait may have collected -> %d", rc_a);
            if (rc_a == BSW_E_INVAL) ++invals; else ++owns;
            same_results(got.data(), want.data(), 300, "collide");
            CHECK(bsw_inflight(ctx) == 0 && bsw_test(ctx, t) < 0, "the ticket is still known after both waits");
            bsw_destroy(ctx);
        }
        CHECK(hipdbl::live_objects() == 0, "collide: %zu HIP objects left", hipdbl::live_objects());
    }
    printf("collide: bsw_wait_ticket kept its ticket %d times, lost it to bsw_wait %d times\n", owns, invals);
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "storm") return storm();
    if (mode == "collide") return collide();
    fprintf(stderr, "usage: host_tickets storm|collide\n");
    return 2;
}
