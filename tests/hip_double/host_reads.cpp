/* host_reads.cpp — resident read blocks (bsw_reads_upload and the three *_reads_* submits: bsw_reads.hip and the submit paths
 * of bsw_batch.hip / bsw_matesw.hip / bsw_cigar.hip) on the host-memory HIP stand-in, under ASan / UBSan or TSan
 * (TEST INFRASTRUCTURE; tests/test_reads_double_cpu.py builds it with its row in tests/_host_double_build.py and runs it).
 *
 *   host_reads parity    the three submits on 1, 2, 3 and 8 devices: byte for byte the pointer forms' results for the same bytes
 *   host_reads threads   a second thread uploads and frees blocks while tickets are in flight; bsw_reads_free is BUSY until the
 *                        ticket is collected
 *   host_reads faults    every HIP / launcher call of an upload and of one submit of each kind fails in turn
 *   host_reads bytes     H2D bytes per task from bsw_host_stats: equal for 50-base and 250-base reads, and at most the pointer
 *                        form's minus the sequence bytes
 *
 * The CIGAR and rescue workloads are host_f4's (host_f4_work.h), the block and the scenario host_reads_work.h's; a read of the
 * block holds the pointer form's bytes — for CIGAR inside a longer read, at every phase of a word — so the pointer form's result
 * is the expected value.
 */
#include <atomic>
#include <chrono>
#include "host_reads_work.h"

static int parity_mode_reads()
{
    const bsw_params p = default_params();
    fresh(8);
    size_t cases = 0;
    uint64_t chunks_seen = 0;
    {
        scenario S;
        S.make(700, 1500, 91);
        S.expect(p);
        const size_t n = S.ct.size(), ne = S.ew.rt.size();
        for (int G : {1, 2, 3, 8}) {
            standin_reads::reset();
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, G, 256, 2);
            bsw_ref *ref = upload(ctx, S.g);
            bsw_reads *rd = S.blk.upload(ctx);
            uint64_t nr = 0, nb = 0, db = 0;
            CHECK(bsw_reads_info(rd, &nr, &nb, &db) == BSW_OK && nr == S.blk.reads.size() && db >= nb / 2 + 32, "bsw_reads_info: %llu reads, %llu bases, %llu bytes",
                  (unsigned long long)nr, (unsigned long long)nb, (unsigned long long)db);
            std::vector<bsw_result> eo(ne + 1);
            c_out co;
            std::vector<bsw_mresult> mo;
            bsw_ticket te = 0, tc = 0, tm = 0;
            int rc = bsw_submit_reads_t(ctx, &p, ref, rd, S.ew.rt.data(), ne, eo.data(), &te);
            CHECK(rc == BSW_OK && te, "bsw_submit_reads_t on %d devices -> %d (%s)", G, rc, bsw_last_error(ctx));
            rc = submit_rm(ctx, p, ref, rd, S.mt, mo, &tm);
            CHECK(rc == BSW_OK && tm, "bsw_matesw_reads_submit_t on %d devices -> %d (%s)", G, rc, bsw_last_error(ctx));
            rc = submit_rc(ctx, p, ref, rd, S.ct, co, &tc);
            CHECK(rc == BSW_OK && tc, "bsw_cigar_reads_submit_t on %d devices -> %d (%s)", G, rc, bsw_last_error(ctx));
            CHECK(bsw_reads_free(ctx, rd) == BSW_E_BUSY, "bsw_reads_free with three tickets in flight");
            CHECK(bsw_wait_ticket(ctx, tc) == BSW_OK, "the CIGAR ticket: %s", bsw_last_error(ctx));
            CHECK(bsw_reads_free(ctx, rd) == BSW_E_BUSY, "bsw_reads_free with two tickets uncollected");
            CHECK(bsw_wait(ctx) == BSW_OK, "bsw_wait: %s", bsw_last_error(ctx));
            std::string why;
            CHECK(same_c(co, S.want.c, n, &why), "%d devices: the CIGAR submit over resident reads differs from the pointer form: %s", G, why.c_str());
            CHECK(same_m(mo, S.want.m, n), "%d devices: the rescue submit over resident reads differs from the pointer form", G);
            CHECK(memcmp(eo.data(), S.want_e.data(), ne * sizeof(bsw_result)) == 0, "%d devices: the extension submit over resident reads differs from bsw_submit_ref_t", G);
            CHECK(standin_reads::store_launches() >= 3, "%llu pack launches took their queries from the block", (unsigned long long)standin_reads::store_launches());
            const bsw_stats s = stats_of(ctx);
            CHECK(s.chunks >= 3 * 8, "%llu chunks for three submits: not enough to reach every one of 8 devices", (unsigned long long)s.chunks);
            chunks_seen += s.chunks;
            /* the checks, in the caller's thread, and no ticket; the block stays free of users */
            {
                bsw_ticket tb = 7;
                std::vector<bsw_rd_task> be(S.ew.rt.begin(), S.ew.rt.begin() + 20);
                be[11].read = (uint32_t)S.blk.reads.size();
                CHECK(bsw_submit_reads_t(ctx, &p, ref, rd, be.data(), 20, eo.data(), &tb) == BSW_E_INVAL && tb == 0, "extension: read index n_reads");
                be[11] = S.ew.rt[11]; be[5].seed.qbeg = S.blk.len[be[5].read];
                CHECK(bsw_submit_reads_t(ctx, &p, ref, rd, be.data(), 20, eo.data(), &tb) == BSW_E_INVAL, "extension: a seed beyond its read");
                std::vector<bsw_rd_mtask> bm(S.mt.begin(), S.mt.begin() + 20);
                bm[3].read = 0xffffffffu;
                CHECK(submit_rm(ctx, p, ref, rd, bm, mo, &tb) == BSW_E_INVAL && tb == 0, "rescue: read index 2^32 - 1");
                bm[3] = S.mt[3]; bm[4].is_rev = 2;
                CHECK(submit_rm(ctx, p, ref, rd, bm, mo, &tb) == BSW_E_INVAL, "rescue: the pointer form's check");
                std::vector<bsw_rd_ctask> bc(S.ct.begin(), S.ct.begin() + 20);
                bc[2].read = (uint32_t)S.blk.reads.size();
                CHECK(submit_rc(ctx, p, ref, rd, bc, co, &tb) == BSW_E_INVAL && tb == 0, "CIGAR: read index n_reads");
                bc[2] = S.ct[2]; bc[6].qb = -1;
                CHECK(submit_rc(ctx, p, ref, rd, bc, co, &tb) == BSW_E_INVAL, "CIGAR: qb < 0");
                bc[6] = S.ct[6]; bc[6].qe = bc[6].qb - 1;
                CHECK(submit_rc(ctx, p, ref, rd, bc, co, &tb) == BSW_E_INVAL, "CIGAR: qe < qb");
                bc[6] = S.ct[6]; bc[6].qe = S.blk.len[bc[6].read] + 1;
                CHECK(submit_rc(ctx, p, ref, rd, bc, co, &tb) == BSW_E_INVAL, "CIGAR: qe beyond the read");
                bc[6] = S.ct[6]; bc[7].max_tries = 4;
                CHECK(submit_rc(ctx, p, ref, rd, bc, co, &tb) == BSW_E_INVAL, "CIGAR: the pointer form's check");
                CHECK(bsw_inflight(ctx) == 0, "a refused submit made a ticket");
            }
            CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "bsw_reads_free after the tickets were collected: %s", bsw_last_error(ctx));
            {   /* upload's own checks */
                bsw_reads *bad = (bsw_reads *)16;
                const uint8_t *ptrs[2] = {S.blk.ptr[0], nullptr};
                int32_t lens[2] = {S.blk.len[0], 5};
                CHECK(bsw_reads_upload(ctx, ptrs, lens, 2, &bad) == BSW_E_INVAL && !bad, "a NULL read of non-zero length");
                lens[1] = -1;
                CHECK(bsw_reads_upload(ctx, ptrs, lens, 2, &bad) == BSW_E_INVAL, "a negative length");
                lens[1] = 65536; ptrs[1] = ptrs[0];
                CHECK(bsw_reads_upload(ctx, ptrs, lens, 2, &bad) == BSW_E_LIMIT, "a read of 65 536 bases");
                CHECK(bsw_reads_upload(ctx, nullptr, nullptr, 0, &bad) == BSW_OK && bad && bsw_reads_free(ctx, bad) == BSW_OK, "an empty block");
            }
            bsw_ref_free(ctx, ref);
            bsw_destroy(ctx);
            CHECK(hipdbl::live_objects() == 0, "%d devices: %zu HIP objects left alive", G, hipdbl::live_objects());
            ++cases;
        }
        {   /* a block of another context */
            bsw_ctx *a = make_ctx(BSW_KERNEL_AUTO, 1, 256), *b = make_ctx(BSW_KERNEL_AUTO, 1, 256);
            bsw_ref *ref = upload(b, S.g);
            bsw_reads *rd = S.blk.upload(a);
            std::vector<bsw_result> eo(21);
            c_out co;
            std::vector<bsw_mresult> mo;
            CHECK(bsw_submit_reads_t(b, &p, ref, rd, S.ew.rt.data(), 20, eo.data(), nullptr) == BSW_E_INVAL, "extension with a foreign block");
            CHECK(submit_rm(b, p, ref, rd, S.mt, mo, nullptr) == BSW_E_INVAL && submit_rc(b, p, ref, rd, S.ct, co, nullptr) == BSW_E_INVAL, "rescue / CIGAR with a foreign block");
            CHECK(bsw_reads_free(b, rd) == BSW_E_INVAL && bsw_reads_free(a, rd) == BSW_OK, "bsw_reads_free by the wrong context");
            bsw_ref_free(b, ref);
            bsw_destroy(a);
            bsw_destroy(b);
        }
    }
    printf("parity: %zu cases, %llu chunks\n", cases, (unsigned long long)chunks_seen);
    return 0;
}

/* ---- threads: upload and free from a second thread while tickets are in flight ---- */
static int threads_mode()
{
    const bsw_params p = default_params();
    fresh(2);
    {
        scenario S;
        S.make(400, 900, 17);
        S.expect(p);
        const size_t n = S.ct.size(), ne = S.ew.rt.size();
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 256, 2);
        bsw_ref *ref = upload(ctx, S.g);
        bsw_reads *rd = S.blk.upload(ctx);
        std::atomic<bool> stop{false};
        std::atomic<int> rounds{0};
        std::thread other([&]() {                     /* "block k + 1": uploaded, used by nobody, freed */
            while (!stop) {
                bsw_reads *nx = nullptr;
                CHECK(bsw_reads_upload(ctx, S.blk.ptr.data(), S.blk.len.data(), S.blk.reads.size(), &nx) == BSW_OK && nx, "upload on the second thread: %s", bsw_last_error(ctx));
                CHECK(bsw_reads_free(ctx, nx) == BSW_OK, "free on the second thread");
                ++rounds;
            }
        });
        for (int rep = 0; rep < 3; ++rep) {
            std::vector<bsw_result> eo(ne + 1);
            c_out co;
            std::vector<bsw_mresult> mo;
            bsw_ticket t[3] = {0, 0, 0};
            CHECK(bsw_submit_reads_t(ctx, &p, ref, rd, S.ew.rt.data(), ne, eo.data(), &t[0]) == BSW_OK, "extension: %s", bsw_last_error(ctx));
            CHECK(submit_rm(ctx, p, ref, rd, S.mt, mo, &t[1]) == BSW_OK, "rescue: %s", bsw_last_error(ctx));
            CHECK(submit_rc(ctx, p, ref, rd, S.ct, co, &t[2]) == BSW_OK, "CIGAR: %s", bsw_last_error(ctx));
            for (int k = 0; k < 3; ++k) {
                CHECK(bsw_reads_free(ctx, rd) == BSW_E_BUSY, "bsw_reads_free with %d tickets uncollected", 3 - k);
                CHECK(bsw_wait_ticket(ctx, t[k]) == BSW_OK, "ticket %d: %s", k, bsw_last_error(ctx));
            }
            std::string why;
            CHECK(same_c(co, S.want.c, n, &why) && same_m(mo, S.want.m, n) && memcmp(eo.data(), S.want_e.data(), ne * sizeof(bsw_result)) == 0, "round %d differs: %s", rep, why.c_str());
        }
        while (rounds < 2) std::this_thread::yield();
        stop = true;
        other.join();
        CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "bsw_reads_free: %s", bsw_last_error(ctx));
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
        printf("threads: ok, %d uploads beside the tickets\n", rounds.load());
    }
    CHECK(hipdbl::live_objects() == 0, "threads: %zu HIP objects left", hipdbl::live_objects());
    return 0;
}

/* ---- faults: every call of an upload and of one submit of each kind fails in turn ---- */
static int faults_mode_reads()
{
    const bsw_params p = default_params();
    fresh(2);
    uint64_t swept = 0, dead = 0;
    {
        scenario S;
        S.make(150, 400, 23);
        S.expect(p);
        const size_t n = S.ct.size(), ne = S.ew.rt.size();
        uint64_t C = 0;
        for (uint64_t k = 0;; ++k) {
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 2, 128, 2, 4000);
            bsw_ref *ref = upload(ctx, S.g);
            S.blk.seal();
            hipdbl::reset_counters();
            if (k) hipdbl::fail_overall(k);
            bsw_reads *rd = nullptr;
            const int ru = bsw_reads_upload(ctx, S.blk.ptr.data(), S.blk.len.data(), S.blk.reads.size(), &rd);
            int rc[3] = {0, 0, 0};
            std::vector<bsw_result> eo(ne + 1);
            c_out co;
            std::vector<bsw_mresult> mo;
            if (ru == BSW_OK) {
                bsw_ticket t[3] = {0, 0, 0};
                CHECK(bsw_submit_reads_t(ctx, &p, ref, rd, S.ew.rt.data(), ne, eo.data(), &t[0]) == BSW_OK && submit_rm(ctx, p, ref, rd, S.mt, mo, &t[1]) == BSW_OK &&
                      submit_rc(ctx, p, ref, rd, S.ct, co, &t[2]) == BSW_OK, "k=%llu: a submit is refused (%s)", (unsigned long long)k, bsw_last_error(ctx));
                for (int j = 0; j < 3; ++j) rc[j] = bsw_wait_ticket(ctx, t[j]);
            } else
                CHECK(!rd && ru == BSW_E_HIP, "k=%llu: a failed upload answers %d and hands out a block", (unsigned long long)k, ru);
            const char *f = hipdbl::fired();
            const std::string fname = f ? f : "";
            const uint64_t calls = hipdbl::overall_calls();
            hipdbl::clear_failures();
            std::string why;
            if (ru == BSW_OK) {
                if (rc[0] == BSW_OK) CHECK(memcmp(eo.data(), S.want_e.data(), ne * sizeof(bsw_result)) == 0, "k=%llu (%s): the extension ticket succeeds with other results", (unsigned long long)k, fname.c_str());
                if (rc[1] == BSW_OK) CHECK(same_m(mo, S.want.m, n), "k=%llu (%s): the rescue ticket succeeds with other results", (unsigned long long)k, fname.c_str());
                if (rc[2] == BSW_OK) CHECK(same_c(co, S.want.c, n, &why), "k=%llu (%s): the CIGAR ticket succeeds with other results: %s", (unsigned long long)k, fname.c_str(), why.c_str());
            }
            if (k == 0) { C = calls; CHECK(ru == BSW_OK && !rc[0] && !rc[1] && !rc[2], "the clean scenario fails: %d %d %d %d", ru, rc[0], rc[1], rc[2]); }
            else if (f && !(ru != BSW_OK || rc[0] || rc[1] || rc[2]))      /* (a release, or the restore of the caller's device: ignored by design) */
                CHECK(fname == "hipFree" || fname == "hipHostFree" || fname == "hipGetLastError" || fname == "hipSetDevice", "k=%llu: %s failed and nobody noticed", (unsigned long long)k, fname.c_str());
            /* the context stays usable — unless the failure made a wait run into the watchdog, which kills it by design: the same
             * three submits, clean */
            bool is_dead = false;
            standin::reset();                         /* (nothing is in flight: a launch round the failed chunk left open must not meet the rerun's) */
            if (ru != BSW_OK) {
                S.blk.seal();
                const int r2 = bsw_reads_upload(ctx, S.blk.ptr.data(), S.blk.len.data(), S.blk.reads.size(), &rd);
                CHECK(r2 == BSW_OK, "k=%llu (%s failed): a further upload -> %d (%s)", (unsigned long long)k, fname.c_str(), r2, bsw_last_error(ctx));
            }
            {
                bsw_ticket t[3];
                const int r2 = bsw_submit_reads_t(ctx, &p, ref, rd, S.ew.rt.data(), ne, eo.data(), &t[0]);
                if (r2 == BSW_E_HIP && strstr(bsw_last_error(ctx), "dead")) { is_dead = true; ++dead; }
                else {
                    CHECK(r2 == BSW_OK && submit_rm(ctx, p, ref, rd, S.mt, mo, &t[1]) == BSW_OK && submit_rc(ctx, p, ref, rd, S.ct, co, &t[2]) == BSW_OK && bsw_wait(ctx) == BSW_OK,
                          "k=%llu (%s): the context is not usable afterwards: %s", (unsigned long long)k, fname.c_str(), bsw_last_error(ctx));
                    CHECK(memcmp(eo.data(), S.want_e.data(), ne * sizeof(bsw_result)) == 0 && same_m(mo, S.want.m, n) && same_c(co, S.want.c, n, &why), "k=%llu: the clean rerun differs", (unsigned long long)k);
                }
            }
            CHECK(!is_dead || rc[0] || rc[1] || rc[2], "k=%llu: the context is dead and no ticket failed", (unsigned long long)k);
            if (!is_dead) CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "k=%llu: bsw_reads_free: %s", (unsigned long long)k, bsw_last_error(ctx));
            if (!is_dead) bsw_ref_free(ctx, ref);
            bsw_destroy(ctx);
            if (is_dead) fresh(2);                    /* (a dead context abandons its device memory with the device: DESIGN.md) */
            else CHECK(hipdbl::live_objects() == 0, "k=%llu (%s failed): %zu HIP objects left alive", (unsigned long long)k, fname.c_str(), hipdbl::live_objects());
            if (k && !f) break;                       /* this run made fewer than k calls: the sweep is over */
            swept = k;
            CHECK(k < C + 400, "the sweep does not end");
        }
        CHECK(10 * dead < swept + 10, "%llu of %llu injection points killed the context", (unsigned long long)dead, (unsigned long long)swept);
        printf("faults: C = %llu, swept %llu, dead %llu\n", (unsigned long long)C, (unsigned long long)swept, (unsigned long long)dead);
    }
    return 0;
}

/* ---- bytes: what crosses the link per task ---- */
static int bytes_mode()
{
    const bsw_params p = default_params();
    fresh(1);
    double per[2][3];
    const int LEN[2] = {50, 250};
    for (int v = 0; v < 2; ++v) {
        /* n tasks per kind over reads of LEN[v] bases: mates of that length, whole reads as CIGAR slices, one seed per read */
        genome1_t g;
        g.make(150001, 3);
        rng_t r(100 + (uint64_t)v);
        const size_t n = 1000;
        block_t blk;
        ework ew;
        make_ext(ew, blk, g, r, n, LEN[v]);
        std::vector<bsw_rd_mtask> mt(n);
        std::vector<bsw_rd_ctask> ct(n);
        std::vector<bsw_mtask> pm(n);
        std::vector<bsw_ctask> pc(n);
        uint64_t seq_bytes = 0;
        for (size_t i = 0; i < n; ++i) {
            const bsw_rd_task &e = ew.rt[i];
            const int64_t x = e.rmax0 + 30;
            memset(&mt[i], 0, sizeof(mt[i])); memset(&ct[i], 0, sizeof(ct[i])); memset(&pm[i], 0, sizeof(pm[i])); memset(&pc[i], 0, sizeof(pc[i]));
            mt[i].read = e.read; mt[i].is_rev = 0; mt[i].rb = x - 20; mt[i].re = x + LEN[v] + 20; mt[i].xtra = KSW_XSUBO | KSW_XSTART | 19; mt[i].min_score = 19;
            ct[i].read = e.read; ct[i].qb = 0; ct[i].qe = LEN[v]; ct[i].w = 20; ct[i].rb = x; ct[i].re = x + LEN[v]; ct[i].min_score = INT_MIN; ct[i].max_tries = 1;
            pm[i].mate = blk.ptr[e.read]; pm[i].l_ms = LEN[v]; pm[i].rb = mt[i].rb; pm[i].re = mt[i].re; pm[i].xtra = mt[i].xtra; pm[i].min_score = 19;
            pc[i].query = blk.ptr[e.read]; pc[i].l_query = LEN[v]; pc[i].w = 20; pc[i].rb = ct[i].rb; pc[i].re = ct[i].re; pc[i].min_score = INT_MIN; pc[i].max_tries = 1;
            seq_bytes += (uint64_t)LEN[v];
        }
        standin_reads::set_max_query_len(LEN[v]);
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2);
        bsw_ref *ref = upload(ctx, g);
        bsw_reads *rd = blk.upload(ctx);
        std::vector<bsw_result> eo(n + 1);
        std::vector<bsw_mresult> mo(n + 1), mo2(n + 1);
        c_out co, co2;
        co.init(n); co2.init(n);
        uint64_t h[7];
        h[0] = stats_of(ctx).h2d_bytes;
        CHECK(bsw_submit_reads_t(ctx, &p, ref, rd, ew.rt.data(), n, eo.data(), nullptr) == BSW_OK && bsw_wait(ctx) == BSW_OK, "extension: %s", bsw_last_error(ctx));
        h[1] = stats_of(ctx).h2d_bytes;
        CHECK(bsw_matesw_reads_submit_t(ctx, &p, ref, rd, mt.data(), n, mo.data(), nullptr) == BSW_OK && bsw_wait(ctx) == BSW_OK, "rescue: %s", bsw_last_error(ctx));
        h[2] = stats_of(ctx).h2d_bytes;
        CHECK(bsw_cigar_reads_submit_t(ctx, &p, ref, rd, ct.data(), n, MAXC, co.cig.data(), MAXMD, co.md.data(), co.res.data(), nullptr) == BSW_OK && bsw_wait(ctx) == BSW_OK, "CIGAR: %s", bsw_last_error(ctx));
        h[3] = stats_of(ctx).h2d_bytes;
        CHECK(bsw_matesw_ref_submit_t(ctx, &p, ref, pm.data(), n, mo2.data(), nullptr) == BSW_OK && bsw_wait(ctx) == BSW_OK, "rescue, pointer form: %s", bsw_last_error(ctx));
        h[4] = stats_of(ctx).h2d_bytes;
        CHECK(bsw_cigar_ref_submit_t(ctx, &p, ref, pc.data(), n, MAXC, co2.cig.data(), MAXMD, co2.md.data(), co2.res.data(), nullptr) == BSW_OK && bsw_wait(ctx) == BSW_OK, "CIGAR, pointer form: %s", bsw_last_error(ctx));
        h[5] = stats_of(ctx).h2d_bytes;
        std::string why;
        CHECK(same_m(mo, mo2, n) && same_c(co, co2, n, &why), "%d-base reads: the two forms differ: %s", LEN[v], why.c_str());
        for (int k = 0; k < 3; ++k) per[v][k] = (double)(h[k + 1] - h[k]) / (double)n;
        /* pageable sequences: the pointer forms send the records AND the bases */
        CHECK(h[2] - h[1] <= (h[4] - h[3]) - seq_bytes, "rescue over %d-base reads: %llu bytes, the pointer form %llu of which %llu are mates", LEN[v],
              (unsigned long long)(h[2] - h[1]), (unsigned long long)(h[4] - h[3]), (unsigned long long)seq_bytes);
        CHECK(h[3] - h[2] <= (h[5] - h[4]) - seq_bytes, "CIGAR over %d-base reads: %llu bytes, the pointer form %llu of which %llu are reads", LEN[v],
              (unsigned long long)(h[3] - h[2]), (unsigned long long)(h[5] - h[4]), (unsigned long long)seq_bytes);
        printf("bytes: %d-base reads: extension %.1f, rescue %.1f, CIGAR %.1f H2D bytes per task (pointer forms: rescue %.1f, CIGAR %.1f)\n", LEN[v], per[v][0], per[v][1], per[v][2],
               (double)(h[4] - h[3]) / (double)n, (double)(h[5] - h[4]) / (double)n);
        CHECK(bsw_reads_free(ctx, rd) == BSW_OK, "bsw_reads_free");
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
    }
    for (int k = 0; k < 3; ++k)
        CHECK(per[0][k] == per[1][k], "kind %d: %.2f H2D bytes per task with 50-base reads, %.2f with 250-base reads: a term grows with the sequences", k, per[0][k], per[1][k]);
    CHECK(hipdbl::live_objects() == 0, "bytes: %zu HIP objects left", hipdbl::live_objects());
    printf("bytes: ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    setenv("BSW_F4_MATESW_WORK", "400000", 1);       /* (chunks a test-sized submit is cut into several of, as host_f4_stream does) */
    setenv("BSW_F4_CIGAR_WORK", "150000", 1);
    if (mode == "parity") return parity_mode_reads();
    if (mode == "threads") return threads_mode();
    if (mode == "faults") return faults_mode_reads();
    if (mode == "bytes") return bytes_mode();
    fprintf(stderr, "usage: host_reads parity | threads | faults | bytes\n");
    return 2;
}
