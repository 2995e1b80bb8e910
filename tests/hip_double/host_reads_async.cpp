/* host_reads_async.cpp — the asynchronous read-block upload (bsw_reads_upload_start / bsw_reads_test / bsw_reads_wait /
 * bsw_reads_image: bsw_reads_async.hip, the upload jobs of bsw_batch.hip, reads_order in the three submit paths) on the
 * host-memory HIP stand-in, under ASan / UBSan or TSan (TEST INFRASTRUCTURE; tests/test_reads_async_double_cpu.py builds it with
 * its row in tests/_host_double_build.py and runs it).
 *
 *   host_reads_async parity     the image equals bsw_reads_upload's on 1, 2, 3 and 8 devices, one and several pieces per device,
 *                               reads in registered and in pageable memory; the three *_reads_* tickets submitted right behind
 *                               the start with every stream stalled complete only after the release and equal the pointer forms
 *   host_reads_async limits     the third upload and bsw_reads_free while one is in flight answer BSW_E_BUSY; an upload is no
 *                               submit; bsw_destroy with an upload in flight waits for it
 *   host_reads_async watchdog   an upload on a stalled device kills the context; its tickets fail
 *   host_reads_async faults     every HIP / launcher call of a start and of its pieces fails in turn
 *   host_reads_async threads    start / test / wait / submit from nine threads
 *
 * The workloads and the expected values are host_reads' (host_reads_work.h). */
#include <atomic>
#include <chrono>
#include "host_reads_work.h"

namespace standin_rdpack {
uint64_t launches();
uint64_t reads();
void reset();
}

/* blocks and a reference that outlive their contexts on purpose (external linkage: the stores are not optimised away) */
bsw_reads *g_kept_rd[2] = {nullptr, nullptr};
bsw_ref *g_kept_ref = nullptr;
std::vector<bsw_reads *> g_kept;                   /* ... and the blocks of contexts the watchdog killed in the fault sweep */

/* every stream there is or will be (ordinals count up over all contexts of a run: eight contexts of up to eight devices pass 96) */
static void stall_all() { for (int k = 0; k < 16384; ++k) hipdbl::stall_stream(k); }

static bsw_reads *start(bsw_ctx *ctx, block_t &b)
{
    b.seal();
    bsw_reads *rd = nullptr;
    const int rc = bsw_reads_upload_start(ctx, b.ptr.data(), b.len.data(), b.reads.size(), &rd);
    CHECK(rc == BSW_OK && rd, "bsw_reads_upload_start -> %d (%s)", rc, bsw_last_error(ctx));
    return rd;
}

static std::vector<uint64_t> image(bsw_ctx *ctx, const bsw_reads *rd, int k)
{
    uint64_t db = 0;
    CHECK(bsw_reads_info(rd, nullptr, nullptr, &db) == BSW_OK, "bsw_reads_info");
    std::vector<uint64_t> w(db / 8 + 1, 0x5a5a5a5a5a5a5a5aull);
    const int rc = bsw_reads_image(ctx, rd, k, w.data(), db / 8);
    CHECK(rc == BSW_OK, "bsw_reads_image of device %d -> %d (%s)", k, rc, bsw_last_error(ctx));
    CHECK(w.back() == 0x5a5a5a5a5a5a5a5aull, "bsw_reads_image wrote behind the image");
    w.pop_back();
    return w;
}

struct tickets3 {
    std::vector<bsw_result> eo;
    c_out co;
    std::vector<bsw_mresult> mo;
    bsw_ticket t[3] = {0, 0, 0};
    int rc[3] = {0, 0, 0};
    void submit(bsw_ctx *ctx, const bsw_params &p, bsw_ref *ref, bsw_reads *rd, scenario &S)
    {
        eo.assign(S.ew.rt.size() + 1, bsw_result());
        CHECK(bsw_submit_reads_t(ctx, &p, ref, rd, S.ew.rt.data(), S.ew.rt.size(), eo.data(), &t[0]) == BSW_OK, "bsw_submit_reads_t: %s", bsw_last_error(ctx));
        CHECK(submit_rm(ctx, p, ref, rd, S.mt, mo, &t[1]) == BSW_OK, "bsw_matesw_reads_submit_t: %s", bsw_last_error(ctx));
        CHECK(submit_rc(ctx, p, ref, rd, S.ct, co, &t[2]) == BSW_OK, "bsw_cigar_reads_submit_t: %s", bsw_last_error(ctx));
    }
    void wait(bsw_ctx *ctx) { for (int k = 0; k < 3; ++k) rc[k] = bsw_wait_ticket(ctx, t[k]); }
    bool ok() const { return !rc[0] && !rc[1] && !rc[2]; }
    void same(scenario &S, const char *what)
    {
        std::string why;
        CHECK(memcmp(eo.data(), S.want_e.data(), S.ew.rt.size() * sizeof(bsw_result)) == 0, "%s: the extension ticket differs from bsw_submit_ref_t", what);
        CHECK(same_m(mo, S.want.m, S.mt.size()), "%s: the rescue ticket differs from the pointer form", what);
        CHECK(same_c(co, S.want.c, S.ct.size(), &why), "%s: the CIGAR ticket differs from the pointer form: %s", what, why.c_str());
    }
};

/* the block's reads once more, back to back with small gaps in ONE registered arena: the direct path */
struct reg_block {
    block_t blk;
    uint8_t *arena = nullptr;
    void make(const block_t &src)
    {
        size_t total = 64;
        for (auto &r : src.reads) total += r.size() + 3;
        arena = (uint8_t *)bsw_host_alloc(total);
        CHECK(arena, "bsw_host_alloc");
        blk.reads = src.reads;
        blk.ptr.clear(); blk.len.clear();
        size_t off = 5;
        for (size_t i = 0; i < src.reads.size(); ++i) {
            const auto &r = src.reads[i];
            if (!r.empty()) memcpy(arena + off, r.data(), r.size());
            blk.ptr.push_back(r.empty() ? nullptr : arena + off);
            blk.len.push_back((int32_t)r.size());
            off += r.size() + i % 4;
        }
    }
    ~reg_block() { if (arena) bsw_host_free(arena); }
};

static int parity_mode_async()
{
    const bsw_params p = default_params();
    fresh(8);
    size_t cases = 0;
    uint64_t pieces = 0;
    {
        scenario S;
        S.make(300, 700, 91);
        S.blk.reads.insert(S.blk.reads.begin() + 40, std::vector<uint8_t>());      /* zero-length reads in the middle ... */
        for (auto &t : S.ew.rt) if (t.read >= 40) ++t.read;
        for (auto &t : S.mt) if (t.read >= 40) ++t.read;
        for (auto &t : S.ct) if (t.read >= 40) ++t.read;
        S.blk.reads.insert(S.blk.reads.begin(), std::vector<uint8_t>());             /* ... in front ... */
        for (auto &t : S.ew.rt) ++t.read;
        for (auto &t : S.mt) ++t.read;
        for (auto &t : S.ct) ++t.read;
        S.blk.reads.push_back(std::vector<uint8_t>(251));                            /* (every byte value, in a read no task names) */
        for (size_t i = 0; i < 251; ++i) S.blk.reads.back()[i] = (uint8_t)(i + 5);
        S.blk.reads.push_back(std::vector<uint8_t>());                               /* ... and at the end */
        S.blk.seal();
        S.expect(p);
        reg_block RB;
        RB.make(S.blk);
        for (int G : {1, 2, 3, 8}) {
            for (int direct = 0; direct < 2; ++direct) {
                if (G == 1 && !direct) unsetenv("BSW_READS_UP_BYTES"); else setenv("BSW_READS_UP_BYTES", direct ? "9000" : "2500", 1);
                /* (the stand-ins' ledgers are keyed by device addresses: a new context's buffers must not meet the last one's entries) */
                standin::reset();
                standin_reads::reset();
                standin_rdpack::reset();
                bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, G, 256, 2);
                bsw_ref *ref = upload(ctx, S.g);
                block_t &B = direct ? RB.blk : S.blk;
                /* the image */
                bsw_reads *sync = nullptr;
                CHECK(bsw_reads_upload(ctx, B.ptr.data(), B.len.data(), B.reads.size(), &sync) == BSW_OK, "bsw_reads_upload: %s", bsw_last_error(ctx));
                const std::vector<uint64_t> want = image(ctx, sync, 0);
                CHECK(bsw_reads_test(ctx, sync) == 1 && bsw_reads_wait(ctx, sync) == BSW_OK, "a block of bsw_reads_upload is ready");
                CHECK(bsw_reads_free(ctx, sync) == BSW_OK, "bsw_reads_free");
                bsw_reads *rd = nullptr;
                CHECK(bsw_reads_upload_start(ctx, B.ptr.data(), B.len.data(), B.reads.size(), &rd) == BSW_OK && rd, "bsw_reads_upload_start on %d devices: %s", G, bsw_last_error(ctx));
                CHECK(bsw_inflight(ctx) == 0, "an upload counts as a submit");
                CHECK(bsw_reads_wait(ctx, rd) == BSW_OK && bsw_reads_wait(ctx, rd) == BSW_OK && bsw_reads_test(ctx, rd) == 1, "bsw_reads_wait: %s", bsw_last_error(ctx));
                for (int k = 0; k < G; ++k) {
                    const std::vector<uint64_t> got = image(ctx, rd, k);
                    CHECK(got.size() == want.size(), "image sizes");
                    for (size_t i = 0; i < got.size(); ++i)
                        CHECK(got[i] == want[i], "%d devices, %s: word %zu of device %d's copy is %016llx, bsw_reads_upload makes %016llx", G, direct ? "direct" : "gather", i, k,
                              (unsigned long long)got[i], (unsigned long long)want[i]);
                }
                const uint64_t per_dev = standin_rdpack::launches() / (uint64_t)G;
                CHECK(standin_rdpack::launches() == per_dev * (uint64_t)G && per_dev >= ((G == 1 && !direct) ? 1u : 4u), "%llu pack launches on %d devices", (unsigned long long)standin_rdpack::launches(), G);
                pieces += standin_rdpack::launches();
                CHECK(stats_of(ctx).h2d_bytes > 0, "the pieces' bytes are not in bsw_host_stats");
                CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "bsw_reads_free: %s", bsw_last_error(ctx));
                /* ordering: every stream held, the three tickets right behind the start */
                stall_all();
                rd = start(ctx, B);
                tickets3 T;
                T.submit(ctx, p, ref, rd, S);
                CHECK(bsw_inflight(ctx) == 3, "bsw_inflight counts %d with three tickets and an upload", bsw_inflight(ctx));
                std::this_thread::sleep_for(std::chrono::milliseconds(30));
                CHECK(bsw_reads_test(ctx, rd) == 0, "the upload finished on stalled streams");
                for (int k = 0; k < 3; ++k) CHECK(bsw_test(ctx, T.t[k]) == 0, "ticket %d completed although the upload it depends on is held", k);
                CHECK(bsw_reads_free(ctx, rd) == BSW_E_BUSY, "bsw_reads_free with the upload in flight");
                hipdbl::release_streams();
                T.wait(ctx);
                CHECK(T.ok(), "%d devices: tickets -> %d %d %d (%s)", G, T.rc[0], T.rc[1], T.rc[2], bsw_last_error(ctx));
                T.same(S, direct ? "direct" : "gather");
                CHECK(standin_reads::store_launches() >= 3, "no pack launch took its queries from the block");
                CHECK(bsw_reads_wait(ctx, rd) == BSW_OK && bsw_reads_free(ctx, rd) == BSW_OK, "wait + free: %s", bsw_last_error(ctx));
                /* an empty block and one without a base: ready at once */
                bsw_reads *e0 = nullptr;
                const uint8_t *np_[2] = {nullptr, nullptr};
                const int32_t nl[2] = {0, 0};
                CHECK(bsw_reads_upload_start(ctx, nullptr, nullptr, 0, &e0) == BSW_OK && e0 && bsw_reads_test(ctx, e0) == 1, "the empty block");
                CHECK(image(ctx, e0, G - 1) == std::vector<uint64_t>(4, 0ull), "the empty block's image");
                CHECK(bsw_reads_free(ctx, e0) == BSW_OK, "free");
                CHECK(bsw_reads_upload_start(ctx, np_, nl, 2, &e0) == BSW_OK && e0 && bsw_reads_test(ctx, e0) == 1 && bsw_reads_free(ctx, e0) == BSW_OK, "two reads without a base");
                bsw_ref_free(ctx, ref);
                bsw_destroy(ctx);
                CHECK(hipdbl::live_objects() == 1, "%d devices: %zu HIP objects left alive", G, hipdbl::live_objects());     /* (the registered arena) */
                ++cases;
            }
        }
    }
    CHECK(hipdbl::live_objects() == 0, "parity: %zu HIP objects left", hipdbl::live_objects());
    printf("parity: %zu cases, %llu pieces\n", cases, (unsigned long long)pieces);
    return 0;
}

static int limits_mode_async()
{
    const bsw_params p = default_params();
    fresh(2);
    bsw_reads *&kept = g_kept_rd[0];                 /* (a block that outlives its context: reachable, not freed) */
    {
        scenario S;
        S.make(150, 300, 19);
        S.expect(p);
        setenv("BSW_READS_UP_BYTES", "5000", 1);
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256, 2);
        bsw_ref *ref = upload(ctx, S.g);
        stall_all();
        bsw_reads *a = start(ctx, S.blk), *b = start(ctx, S.blk), *c = (bsw_reads *)16;
        std::this_thread::sleep_for(std::chrono::milliseconds(60));      /* (every slot sits in a piece's wait by now: nothing moves) */
        const size_t live = hipdbl::live_objects();
        const bsw_stats s0 = stats_of(ctx);
        CHECK(bsw_reads_upload_start(ctx, S.blk.ptr.data(), S.blk.len.data(), S.blk.reads.size(), &c) == BSW_E_BUSY && !c, "a third upload in flight");
        CHECK(hipdbl::live_objects() == live && stats_of(ctx).h2d_bytes == s0.h2d_bytes, "the refused upload changed something");
        CHECK(bsw_inflight(ctx) == 0 && bsw_wait(ctx) == BSW_OK, "bsw_wait collects an upload");
        CHECK(bsw_reads_test(ctx, a) == 0 && bsw_reads_test(ctx, b) == 0, "uploads finished on stalled streams");
        CHECK(bsw_reads_free(ctx, a) == BSW_E_BUSY && bsw_reads_free(ctx, b) == BSW_E_BUSY, "bsw_reads_free with the upload in flight");
        tickets3 T;                                  /* four tickets fit beside two uploads */
        T.submit(ctx, p, ref, b, S);
        std::vector<bsw_result> e4(S.ew.t.size() + 1);
        bsw_ticket t4 = 0;
        CHECK(bsw_submit_ref_t(ctx, &p, ref, S.ew.t.data(), S.ew.t.size(), e4.data(), &t4) == BSW_OK && bsw_inflight(ctx) == 4, "a fourth ticket beside two uploads");
        hipdbl::release_streams();
        CHECK(bsw_reads_wait(ctx, a) == BSW_OK && bsw_reads_wait(ctx, b) == BSW_OK, "bsw_reads_wait: %s", bsw_last_error(ctx));
        T.wait(ctx);
        CHECK(T.ok() && bsw_wait_ticket(ctx, t4) == BSW_OK, "tickets: %s", bsw_last_error(ctx));
        T.same(S, "limits");
        CHECK(memcmp(e4.data(), S.want_e.data(), S.ew.t.size() * sizeof(bsw_result)) == 0, "the pointer-form ticket beside the uploads differs");
        c = start(ctx, S.blk);                       /* a place is free again */
        CHECK(bsw_reads_wait(ctx, c) == BSW_OK && bsw_reads_free(ctx, c) == BSW_OK && bsw_reads_free(ctx, a) == BSW_OK && bsw_reads_free(ctx, b) == BSW_OK, "free: %s", bsw_last_error(ctx));
        /* bsw_destroy with an upload in flight waits for it */
        bsw_ref_free(ctx, ref);
        stall_all();
        kept = start(ctx, S.blk);
        std::atomic<bool> destroyed{false};
        std::thread rel([&]() {
            std::this_thread::sleep_for(std::chrono::milliseconds(40));
            CHECK(!destroyed.load(), "bsw_destroy returned with the upload held");
            hipdbl::release_streams();
        });
        bsw_destroy(ctx);
        destroyed = true;
        rel.join();
        CHECK(standin_rdpack::launches() > 0, "no piece ran");
    }
    fresh(2);
    printf("limits: ok\n");
    return 0;
}

static int watchdog_mode_async()
{
    const bsw_params p = default_params();
    fresh(1);
    bsw_reads *&kept = g_kept_rd[1];                 /* (what a dead context leaves behind stays reachable) */
    bsw_ref *&kept_ref = g_kept_ref;
    {
        scenario S;
        S.make(100, 200, 29);
        S.expect(p);
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2, 300);
        kept_ref = upload(ctx, S.g);
        stall_all();
        kept = start(ctx, S.blk);
        tickets3 T;
        T.submit(ctx, p, kept_ref, kept, S);
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = bsw_reads_wait(ctx, kept);
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        CHECK(rc == BSW_E_HIP && strstr(bsw_last_error(ctx), "timeout"), "bsw_reads_wait on a stalled device -> %d (%s)", rc, bsw_last_error(ctx));
        CHECK(s < 20.0, "the watchdog took %.1f s", s);
        CHECK(bsw_reads_test(ctx, kept) == BSW_E_HIP && bsw_reads_wait(ctx, kept) == BSW_E_HIP, "the failure is not remembered");
        T.wait(ctx);
        CHECK(T.rc[0] == BSW_E_HIP && T.rc[1] == BSW_E_HIP && T.rc[2] == BSW_E_HIP, "tickets of the dead upload -> %d %d %d", T.rc[0], T.rc[1], T.rc[2]);
        bsw_reads *more = nullptr;
        CHECK(bsw_reads_upload_start(ctx, S.blk.ptr.data(), S.blk.len.data(), S.blk.reads.size(), &more) == BSW_E_HIP && !more && strstr(bsw_last_error(ctx), "dead"), "a start on the dead context");
        hipdbl::release_streams();
        bsw_destroy(ctx);
    }
    fresh(1);
    printf("watchdog: ok\n");
    return 0;
}

static int faults_mode_async()
{
    const bsw_params p = default_params();
    fresh(2);
    uint64_t swept = 0, dead = 0, failed_uploads = 0, refused = 0;
    {
        scenario S;
        S.make(120, 300, 23);
        S.expect(p);
        setenv("BSW_READS_UP_BYTES", "6000", 1);
        for (const char *who : {"launch_reads_pack", "hipMemcpyAsync", "hipMemsetAsync"}) {
            /* one device: the upload's first call of this name fails -> every ticket of the block fails with BSW_E_HIP and a text
             * that says why, NO pack launch reads the block, and a pointer-form ticket beside them is left alone */
            fresh(1);
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 128, 2, 4000);
            bsw_ref *ref = upload(ctx, S.g);
            standin_reads::reset();
            hipdbl::reset_counters();
            hipdbl::fail_named(who, 1);
            bsw_reads *rd = start(ctx, S.blk);
            CHECK(bsw_reads_wait(ctx, rd) == BSW_E_HIP, "%s fails and bsw_reads_wait -> ok", who);
            hipdbl::clear_failures();
            tickets3 T;
            T.submit(ctx, p, ref, rd, S);
            std::vector<bsw_result> e4(S.ew.t.size() + 1);
            bsw_ticket t4 = 0;
            CHECK(bsw_submit_ref_t(ctx, &p, ref, S.ew.t.data(), S.ew.t.size(), e4.data(), &t4) == BSW_OK, "a pointer-form ticket");
            for (int j = 0; j < 3; ++j) {
                T.rc[j] = bsw_wait_ticket(ctx, T.t[j]);
                CHECK(T.rc[j] == BSW_E_HIP && strstr(bsw_last_error(ctx), "upload of the read block failed"), "%s: ticket %d -> %d (%s)", who, j, T.rc[j], bsw_last_error(ctx));
            }
            CHECK(standin_reads::store_launches() == 0, "%s: %llu pack launches read a block whose upload failed", who, (unsigned long long)standin_reads::store_launches());
            CHECK(bsw_wait_ticket(ctx, t4) == BSW_OK && memcmp(e4.data(), S.want_e.data(), S.ew.t.size() * sizeof(bsw_result)) == 0, "%s: the pointer-form ticket beside the failed upload", who);
            CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "bsw_reads_free after a failed upload");
            bsw_ref_free(ctx, ref);
            bsw_destroy(ctx);
            CHECK(hipdbl::live_objects() == 0, "%s: %zu HIP objects left alive", who, hipdbl::live_objects());
        }
        fresh(2);
        uint64_t C = 0;
        for (uint64_t k = 0;; ++k) {
            standin::reset();                         /* (ledgers are keyed by device addresses: nothing of the last context's may be left) */
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 128, 2, 4000);
            bsw_ref *ref = upload(ctx, S.g);
            S.blk.seal();
            standin_reads::reset();
            const size_t live0 = hipdbl::live_objects();
            hipdbl::reset_counters();
            if (k) hipdbl::fail_overall(k);
            bsw_reads *rd = nullptr;
            const int ru = bsw_reads_upload_start(ctx, S.blk.ptr.data(), S.blk.len.data(), S.blk.reads.size(), &rd);
            tickets3 T;
            int rw = BSW_OK;
            if (ru == BSW_OK) {
                T.submit(ctx, p, ref, rd, S);
                rw = bsw_reads_wait(ctx, rd);
                T.wait(ctx);
            } else {
                CHECK(!rd && (ru == BSW_E_HIP || ru == BSW_E_NOMEM), "k=%llu: a failed start answers %d and hands out a block", (unsigned long long)k, ru);
                ++refused;
            }
            const char *f = hipdbl::fired();
            const std::string fname = f ? f : "";
            const uint64_t calls = hipdbl::overall_calls();
            hipdbl::clear_failures();
            if (ru != BSW_OK) CHECK(hipdbl::live_objects() == live0 || fname == "hipFree" || fname == "hipEventDestroy", "k=%llu (%s): a failed start left %zu objects where %zu were", (unsigned long long)k, fname.c_str(), hipdbl::live_objects(), live0);
            if (ru == BSW_OK && rw != BSW_OK) {
                ++failed_uploads;
                CHECK(bsw_reads_test(ctx, rd) == rw, "bsw_reads_test after a failed upload");
                /* the failure hit the upload: a ticket of the block either fails with BSW_E_HIP or — its chunks had all passed the
                 * upload's events when a WAIT of the upload failed — is bit-exact */
                for (int j = 0; j < 3; ++j) CHECK(T.rc[j] == BSW_OK || T.rc[j] == BSW_E_HIP, "k=%llu (%s): ticket %d -> %d", (unsigned long long)k, fname.c_str(), j, T.rc[j]);
                if (fname != "hipEventRecord" && fname != "hipEventQuery" && fname != "hipEventSynchronize") {
                    CHECK(T.rc[0] == BSW_E_HIP && T.rc[1] == BSW_E_HIP && T.rc[2] == BSW_E_HIP, "k=%llu (%s): the upload failed before its work was queued and tickets -> %d %d %d", (unsigned long long)k, fname.c_str(), T.rc[0], T.rc[1], T.rc[2]);
                    /* (a chunk on the OTHER device, whose copy was complete, may have run: the one-device case above counts launches) */
                }
            }
            if (ru == BSW_OK) {
                std::string why;
                if (T.rc[0] == BSW_OK) CHECK(memcmp(T.eo.data(), S.want_e.data(), S.ew.rt.size() * sizeof(bsw_result)) == 0, "k=%llu (%s): the extension ticket succeeds with other results", (unsigned long long)k, fname.c_str());
                if (T.rc[1] == BSW_OK) CHECK(same_m(T.mo, S.want.m, S.mt.size()), "k=%llu (%s): the rescue ticket succeeds with other results", (unsigned long long)k, fname.c_str());
                if (T.rc[2] == BSW_OK) CHECK(same_c(T.co, S.want.c, S.ct.size(), &why), "k=%llu (%s): the CIGAR ticket succeeds with other results: %s", (unsigned long long)k, fname.c_str(), why.c_str());
            }
            if (k == 0) { C = calls; CHECK(ru == BSW_OK && rw == BSW_OK && T.ok(), "the clean scenario fails: %d %d %d %d %d", ru, rw, T.rc[0], T.rc[1], T.rc[2]); }
            else if (f && ru == BSW_OK && rw == BSW_OK && T.ok())
                CHECK(fname == "hipFree" || fname == "hipHostFree" || fname == "hipGetLastError" || fname == "hipSetDevice" || fname == "hipEventDestroy", "k=%llu: %s failed and nobody noticed", (unsigned long long)k, fname.c_str());
            /* other tickets are left alone and the context stays usable, unless the watchdog killed it: a pointer-form ticket and
             * the same upload + tickets, clean */
            bool is_dead = false;
            standin::reset();
            {
                std::vector<bsw_result> e4(S.ew.t.size() + 1);
                const int r2 = bsw_submit_ref_t(ctx, &p, ref, S.ew.t.data(), S.ew.t.size(), e4.data(), nullptr);
                if (r2 == BSW_E_HIP && strstr(bsw_last_error(ctx), "dead")) { is_dead = true; ++dead; if (rd) g_kept.push_back(rd); }
                else {
                    if (rd) CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "k=%llu (%s): bsw_reads_free after a%s upload: %s", (unsigned long long)k, fname.c_str(), rw ? " failed" : "n", bsw_last_error(ctx));
                    CHECK(r2 == BSW_OK && bsw_wait(ctx) == BSW_OK, "k=%llu (%s): a pointer-form ticket afterwards: %s", (unsigned long long)k, fname.c_str(), bsw_last_error(ctx));
                    CHECK(memcmp(e4.data(), S.want_e.data(), S.ew.t.size() * sizeof(bsw_result)) == 0, "k=%llu: the pointer-form ticket differs", (unsigned long long)k);
                    bsw_reads *r3 = start(ctx, S.blk);
                    tickets3 T2;
                    T2.submit(ctx, p, ref, r3, S);
                    T2.wait(ctx);
                    CHECK(T2.ok() && bsw_reads_wait(ctx, r3) == BSW_OK, "k=%llu (%s): the clean rerun: %s", (unsigned long long)k, fname.c_str(), bsw_last_error(ctx));
                    T2.same(S, "the clean rerun");
                    CHECK(bsw_reads_free(ctx, r3) == BSW_OK, "free");
                }
            }
            CHECK(!is_dead || rw != BSW_OK || !T.ok(), "k=%llu: the context is dead and nothing failed", (unsigned long long)k);
            if (!is_dead) bsw_ref_free(ctx, ref);
            bsw_destroy(ctx);
            if (is_dead) fresh(2);
            else CHECK(hipdbl::live_objects() == 0, "k=%llu (%s failed): %zu HIP objects left alive", (unsigned long long)k, fname.c_str(), hipdbl::live_objects());
            if (k && !f) break;
            swept = k;
            CHECK(k < C + 400, "the sweep does not end");
        }
        CHECK(10 * dead < swept + 10, "%llu of %llu injection points killed the context", (unsigned long long)dead, (unsigned long long)swept);
        CHECK(refused >= 3 && failed_uploads >= 5, "%llu refused starts, %llu failed uploads: the sweep missed the upload", (unsigned long long)refused, (unsigned long long)failed_uploads);
        printf("faults: C = %llu, swept %llu, dead %llu, refused %llu, failed uploads %llu\n", (unsigned long long)C, (unsigned long long)swept, (unsigned long long)dead,
               (unsigned long long)refused, (unsigned long long)failed_uploads);
    }
    return 0;
}

static int threads_mode_async()
{
    const bsw_params p = default_params();
    fresh(2);
    {
        scenario S;
        S.make(120, 400, 37);
        S.expect(p);
        setenv("BSW_READS_UP_BYTES", "7000", 1);
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256, 2);
        bsw_ref *ref = upload(ctx, S.g);
        S.blk.seal();
        const size_t ne = S.ew.rt.size();
        std::atomic<int> rounds{0}, busy{0};
        std::vector<std::thread> th;
        for (int w = 0; w < 9; ++w)
            th.emplace_back([&, w]() {
                for (int rep = 0; rep < 3; ++rep) {
                    bsw_reads *rd = nullptr;
                    int rc;
                    while ((rc = bsw_reads_upload_start(ctx, S.blk.ptr.data(), S.blk.len.data(), S.blk.reads.size(), &rd)) == BSW_E_BUSY) { ++busy; std::this_thread::yield(); }
                    CHECK(rc == BSW_OK && rd, "thread %d: start -> %d", w, rc);
                    std::vector<bsw_result> eo(ne + 1);
                    bsw_ticket t = 0;
                    while ((rc = bsw_submit_reads_t(ctx, &p, ref, rd, S.ew.rt.data(), ne, eo.data(), &t)) == BSW_E_BUSY) std::this_thread::yield();
                    CHECK(rc == BSW_OK, "thread %d: submit -> %d", w, rc);
                    const int st = bsw_reads_test(ctx, rd);
                    CHECK(st == 0 || st == 1, "thread %d: bsw_reads_test -> %d", w, st);
                    if ((w + rep) % 2) CHECK(bsw_reads_wait(ctx, rd) == BSW_OK, "thread %d: bsw_reads_wait", w);
                    CHECK(bsw_wait_ticket(ctx, t) == BSW_OK, "thread %d: the ticket", w);
                    CHECK(memcmp(eo.data(), S.want_e.data(), ne * sizeof(bsw_result)) == 0, "thread %d round %d: the extension ticket differs", w, rep);
                    CHECK(bsw_reads_wait(ctx, rd) == BSW_OK && bsw_reads_free(ctx, rd) == BSW_OK, "thread %d: wait + free", w);
                    ++rounds;
                }
            });
        for (auto &t : th) t.join();
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
        printf("threads: ok, %d rounds, %d busy answers\n", rounds.load(), busy.load());
    }
    CHECK(hipdbl::live_objects() == 0, "threads: %zu HIP objects left", hipdbl::live_objects());
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    setenv("BSW_F4_MATESW_WORK", "400000", 1);
    setenv("BSW_F4_CIGAR_WORK", "150000", 1);
    if (mode == "parity") return parity_mode_async();
    if (mode == "limits") return limits_mode_async();
    if (mode == "watchdog") return watchdog_mode_async();
    if (mode == "faults") return faults_mode_async();
    if (mode == "threads") return threads_mode_async();
    fprintf(stderr, "usage: host_reads_async parity | limits | watchdog | faults | threads\n");
    return 2;
}
