/* host_align_long.cpp — the hosts of ksw_align2's long-query route (bsw_set_align_long: bsw_f4.hip, bsw_matesw.hip, bsw_align_long.hip)
 * on the host-memory HIP stand-in, as a stand-alone program per sanitizer (TEST INFRASTRUCTURE; built by
 * its row in tests/_host_double_build.py, run by tests/test_align_long_double_cpu.py).
 *
 *   host_align_long gate      mode 0 refuses a query of more than 1 024 bases, modes 1 and 2 accept it, 8 192 bases are refused always;
 *                             which stand-in ran which task
 *   host_align_long split     a batch that crosses the b[] bound of the sub-batch loop, long tasks in every sub-batch
 *   host_align_long flip      a ticket of one-task chunks submitted under mode 1 (2) behind stalled streams, the switch set to 0 before
 *                             any chunk is processed
 *   host_align_long faults    every HIP call of a batch with long tasks fails in turn; the context stays usable
 *   host_align_long sequence  a batch without long tasks makes, call for call, the HIP calls it makes with the switch off
 *
 * Expected values: oracle/ksw_align_ref.c on the caller's bytes. */
#include "host_common.h"

#include <algorithm>
#include <chrono>

extern "C" void ksw_align2_ref(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat,
                               int o_del, int e_del, int o_ins, int e_ins, int xtra, int32_t *out, uint64_t *cells);
namespace standin_alnl {
uint64_t launches(int cls);
uint64_t launches();
uint64_t tasks();
uint64_t long_tasks();
void reset();
}  // namespace standin_alnl

/* this program's own generator (a 64-bit LCG's high bits): its stream defines the workloads, which the splitmix rng_t of
 * host_common.h would change */
struct lcg_t {
    uint64_t s;
    explicit lcg_t(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    int below(int n) { return n > 0 ? (int)(next() % (uint32_t)n) : 0; }
};

struct awork {
    std::vector<std::vector<uint8_t>> q, tg;
    std::vector<bsw_atask> t;
    void add(lcg_t &r, int ql, int piece, int flank, int xtra)
    {
        std::vector<uint8_t> qq((size_t)ql), tt;
        for (uint8_t &c : qq) c = (uint8_t)r.below(4);
        for (int k = 0; k < flank; ++k) tt.push_back((uint8_t)r.below(4));
        const int a = r.below(ql - std::min(piece, ql) + 1);
        for (int k = 0; k < std::min(piece, ql); ++k) tt.push_back(r.below(25) == 0 ? (uint8_t)r.below(4) : qq[(size_t)(a + k)]);
        for (int k = 0; k < flank; ++k) tt.push_back((uint8_t)r.below(4));
        q.push_back(qq); tg.push_back(tt);
        xt.push_back(xtra);
    }
    std::vector<int> xt;
    void finish()
    {
        t.clear();
        for (size_t i = 0; i < q.size(); ++i) {
            bsw_atask a;
            memset(&a, 0, sizeof(a));
            a.query = q[i].data(); a.target = tg[i].data(); a.qlen = (int)q[i].size(); a.tlen = (int)tg[i].size(); a.xtra = xt[i];
            t.push_back(a);
        }
    }
};

static void want_of(const bsw_params &p, const bsw_atask &t, int32_t *want)
{
    ksw_align2_ref(t.qlen, t.query, t.tlen, t.target, 5, p.mat, p.o_del, p.e_del, p.o_ins, p.e_ins, t.xtra, want, nullptr);
}

static void same_as_oracle(const bsw_params &p, const std::vector<bsw_atask> &t, const std::vector<bsw_kswr> &res, size_t n, const char *what)
{
    for (size_t i = 0; i < n; ++i) {
        int32_t want[7];
        want_of(p, t[i], want);
        CHECK(memcmp(&res[i], want, sizeof(want)) == 0, "%s: task %zu (%d bases): score %d te %d qe %d tb %d qb %d, the oracle's %d %d %d %d %d", what, i, t[i].qlen,
              res[i].score, res[i].te, res[i].qe, res[i].tb, res[i].qb, want[0], want[1], want[2], want[5], want[6]);
    }
}

static const int XF = KSW_XSUBO | KSW_XSTART | 19;

static void mixed(awork &w, lcg_t &r, bool with_long)
{
    const int lens[] = {150, 1024, 1025, 1500, 3000, 8191};
    for (int rep = 0; rep < 2; ++rep)
        for (int ql : lens) {
            if (ql > BSW_ALIGN_MAX_QLEN && !with_long) continue;
            w.add(r, ql, 300, 40, XF);
            w.add(r, ql, 120, 40, XF | KSW_XBYTE);
        }
    w.finish();
}

/* ---- a tiny genome for the rescue calls ---- */
struct lcg_genome_t {
    int64_t l_pac = 0;
    std::vector<uint8_t> bases, pac;
    void make(int64_t n, uint64_t seed)
    {
        lcg_t r(seed);
        l_pac = n;
        bases.resize((size_t)n);
        pac.assign((size_t)(n / 4 + 1), 0);
        for (int64_t i = 0; i < n; ++i) {
            bases[(size_t)i] = (uint8_t)r.below(4);
            pac[(size_t)(i >> 2)] |= (uint8_t)(bases[(size_t)i] << ((~i & 3) << 1));
        }
    }
    std::vector<uint8_t> get(int64_t rb, int64_t re) const          /* bns_get_seq, a window on one strand */
    {
        std::vector<uint8_t> o;
        for (int64_t k = rb; k < re; ++k) o.push_back(k < l_pac ? bases[(size_t)k] : (uint8_t)(3 - bases[(size_t)(2 * l_pac - 1 - k)]));
        return o;
    }
};

struct mwork {
    std::vector<std::vector<uint8_t>> mate;
    std::vector<bsw_mtask> t;
    void add(const lcg_genome_t &g, lcg_t &r, int l_ms, int is_rev, int strand, int xtra)
    {
        const int wl = l_ms + 300;
        const int64_t rb = (strand ? g.l_pac : 0) + r.below((int)(g.l_pac - wl));
        std::vector<uint8_t> w = g.get(rb, rb + wl), m((size_t)l_ms);
        const int a = r.below(200);
        for (int k = 0; k < l_ms; ++k) m[(size_t)k] = r.below(30) == 0 ? (uint8_t)r.below(4) : w[(size_t)(a + k) % w.size()];
        if (is_rev) { std::reverse(m.begin(), m.end()); for (uint8_t &c : m) c = (uint8_t)(3 - c); }
        mate.push_back(m);
        bsw_mtask x;
        memset(&x, 0, sizeof(x));
        x.l_ms = l_ms; x.is_rev = is_rev; x.rb = rb; x.re = rb + wl; x.xtra = xtra; x.min_score = 19;
        t.push_back(x);
    }
    void finish() { for (size_t i = 0; i < t.size(); ++i) t[i].mate = mate[i].data(); }
};

static void same_rescue(const bsw_params &p, const lcg_genome_t &g, const mwork &w, const std::vector<bsw_mresult> &res, const char *what)
{
    for (size_t i = 0; i < w.t.size(); ++i) {
        const bsw_mtask &t = w.t[i];
        std::vector<uint8_t> q = w.mate[i], tg = g.get(t.rb, t.re);
        if (t.is_rev) { std::reverse(q.begin(), q.end()); for (uint8_t &c : q) c = c < 4 ? (uint8_t)(3 - c) : (uint8_t)4; }
        int32_t want[7];
        ksw_align2_ref(t.l_ms, q.data(), (int)tg.size(), tg.data(), 5, p.mat, p.o_del, p.e_del, p.o_ins, p.e_ins, t.xtra, want, nullptr);
        CHECK(memcmp(&res[i].aln, want, sizeof(want)) == 0, "%s: mate %zu (%d bases, is_rev %d): score %d te %d qb %d, the oracle's %d %d %d", what, i, t.l_ms, t.is_rev,
              res[i].aln.score, res[i].aln.te, res[i].aln.qb, want[0], want[1], want[6]);
        CHECK(res[i].status == ((want[0] >= t.min_score && want[6] >= 0) ? 0 : 2), "%s: mate %zu: status %d", what, i, res[i].status);
    }
}

static uint64_t stats_sum()
{
    uint64_t st[32], s = 0;
    const int n = bsw_align_long_stats(st, 32);
    CHECK(n == 12, "bsw_align_long_stats -> %d classes", n);
    for (int c = 0; c < n; ++c) s += st[c];
    return s;
}

static int gate_mode()
{
    const bsw_params p = default_params();
    fresh(1);
    standin_alnl::reset();
    CHECK(bsw_align_long() == 0, "the switch starts at %d", bsw_align_long());
    {
        lcg_t r(5);
        awork all, shortw;
        mixed(all, r, true);
        mixed(shortw, r, false);
        const size_t n = all.t.size(), ns = shortw.t.size();
        size_t n_long = 0;
        for (const bsw_atask &t : all.t) n_long += t.qlen > BSW_ALIGN_MAX_QLEN;
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2);
        std::vector<bsw_kswr> res(n);
        const uint64_t s0 = stats_sum();
        CHECK(bsw_align_batch(ctx, &p, all.t.data(), n, res.data()) == BSW_E_LIMIT, "mode 0 took a query of more than 1 024 bases");
        CHECK(bsw_align_batch(ctx, &p, shortw.t.data(), ns, res.data()) == BSW_OK, "mode 0, short tasks: %s", bsw_last_error(ctx));
        same_as_oracle(p, shortw.t, res, ns, "mode 0");
        CHECK(standin_alnl::launches() == 0 && hipdbl::calls("launch_align_long") == 0 && stats_sum() == s0, "mode 0 reached the long launcher");
        bsw_set_align_long(1);
        uint64_t la = hipdbl::calls("launch_align");
        CHECK(bsw_align_batch(ctx, &p, all.t.data(), n, res.data()) == BSW_OK, "mode 1: %s", bsw_last_error(ctx));
        same_as_oracle(p, all.t, res, n, "mode 1");
        CHECK(standin_alnl::tasks() == n_long && standin_alnl::long_tasks() == n_long, "mode 1: %llu tasks on the long launcher, %zu are long",
              (unsigned long long)standin_alnl::tasks(), n_long);
        CHECK(hipdbl::calls("launch_align") > la, "mode 1: the short tasks did not take launch_align");
        CHECK(stats_sum() - s0 == standin_alnl::launches() && standin_alnl::launches() >= 4, "bsw_align_long_stats counts %llu launches, the stand-in %llu",
              (unsigned long long)(stats_sum() - s0), (unsigned long long)standin_alnl::launches());
        for (int mode = 1; mode <= 2; ++mode) {                 /* beyond BSW_ALIGN_LONG_MAX_QLEN: refused under every mode */
            bsw_set_align_long(mode);
            std::vector<uint8_t> q(8192, 1), tg(50, 1);
            bsw_atask big;
            memset(&big, 0, sizeof(big));
            big.query = q.data(); big.target = tg.data(); big.qlen = 8192; big.tlen = 50; big.xtra = XF;
            CHECK(bsw_align_batch(ctx, &p, &big, 1, res.data()) == BSW_E_LIMIT, "mode %d took 8 192 bases", mode);
            big.qlen = 8191;
            CHECK(bsw_align_batch(ctx, &p, &big, 1, res.data()) == BSW_OK, "mode %d refused 8 191 bases: %s", mode, bsw_last_error(ctx));
        }
        bsw_set_align_long(2);
        la = hipdbl::calls("launch_align");
        const uint64_t t0 = standin_alnl::tasks();
        CHECK(bsw_align_batch(ctx, &p, all.t.data(), n, res.data()) == BSW_OK, "mode 2: %s", bsw_last_error(ctx));
        same_as_oracle(p, all.t, res, n, "mode 2");
        CHECK(hipdbl::calls("launch_align") == la && standin_alnl::tasks() - t0 == n, "mode 2: a task took launch_align");
        bsw_set_align_long(0);
        /* the drop-in calls through the process-wide context */
        const bsw_atask &L = all.t[4];
        CHECK(L.qlen == 1025, "task 4 has %d bases", L.qlen);
        kswr_t k = ksw_align2(L.qlen, (uint8_t *)L.query, L.tlen, (uint8_t *)L.target, 5, p.mat, 6, 1, 6, 1, L.xtra, nullptr);
        CHECK(k.score == -1, "ksw_align2 under mode 0 took 1 025 bases");
        bsw_set_align_long(1);
        int32_t want[7];
        want_of(p, L, want);
        k = ksw_align2(L.qlen, (uint8_t *)L.query, L.tlen, (uint8_t *)L.target, 5, p.mat, 6, 1, 6, 1, L.xtra, nullptr);
        CHECK(memcmp(&k, want, sizeof(want)) == 0, "ksw_align2 under mode 1: score %d, the oracle's %d", k.score, want[0]);
        k = ksw_align(L.qlen, (uint8_t *)L.query, L.tlen, (uint8_t *)L.target, 5, p.mat, 6, 1, L.xtra, nullptr);
        CHECK(memcmp(&k, want, sizeof(want)) == 0, "ksw_align under mode 1: score %d, the oracle's %d", k.score, want[0]);
        bsw_set_align_long(0);
        /* mate rescue, the batch call */
        lcg_genome_t g;
        g.make(40001, 3);
        bsw_ref *ref = nullptr;
        CHECK(bsw_ref_upload(ctx, g.pac.data(), g.l_pac, &ref) == BSW_OK, "bsw_ref_upload: %s", bsw_last_error(ctx));
        mwork mw;
        for (int l_ms : {150, 1025, 1500, 3000})
            for (int k2 = 0; k2 < 4; ++k2) mw.add(g, r, l_ms, k2 & 1, k2 >> 1, XF | ((k2 & 1) ? KSW_XBYTE : 0));
        mw.finish();
        std::vector<bsw_mresult> mres(mw.t.size());
        CHECK(bsw_matesw_ref_batch(ctx, &p, ref, mw.t.data(), mw.t.size(), mres.data()) == BSW_E_LIMIT, "mode 0 took a mate of more than 1 024 bases");
        bsw_set_align_long(1);
        CHECK(bsw_matesw_ref_batch(ctx, &p, ref, mw.t.data(), mw.t.size(), mres.data()) == BSW_OK, "mode 1 rescue: %s", bsw_last_error(ctx));
        bsw_set_align_long(0);
        same_rescue(p, g, mw, mres, "mode 1 rescue");
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
    }
    printf("gate: ok, %llu launches of the long stand-in\n", (unsigned long long)standin_alnl::launches());
    return 0;
}

static int split_mode()
{
    const bsw_params p = default_params();
    fresh(1);
    standin_alnl::reset();
    uint64_t sub = 0;
    {
        lcg_t r(7);
        awork w;
        /* 12 distinct tasks: nine tiny queries against 65 535-base targets with a b[] slice each, three long queries */
        for (int i = 0; i < 12; ++i) {
            if (i % 4 == 1) { w.add(r, i == 1 ? 1025 : i == 5 ? 2000 : 3000, 100, 10, XF | (i == 1 ? KSW_XBYTE : 0)); continue; }
            const int ql = 1 + (i * 3) % 8;
            std::vector<uint8_t> q((size_t)ql), tg((size_t)(65535 - (i % 2) * 7));
            for (uint8_t &c : q) c = (uint8_t)r.below(4);
            for (uint8_t &c : tg) c = (uint8_t)r.below(4);
            for (int c = 0; c < 6; ++c) std::copy(q.begin(), q.end(), tg.begin() + r.below((int)tg.size() - ql + 1));
            w.q.push_back(q); w.tg.push_back(tg);
            w.xt.push_back(KSW_XSUBO | KSW_XSTART | ((i & 1) ? KSW_XBYTE : 0) | (ql > 4 ? 4 : 1));
        }
        w.finish();
        const size_t D = w.t.size(), n = 5700;              /* 9 of 12 tasks add 65 535 entries: 2^28 is crossed near task 5 460 */
        for (size_t k = D; k < n; ++k) w.t.push_back(w.t[k % D]);
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2, 600000);
        std::vector<bsw_kswr> res(n);
        bsw_set_align_long(1);
        const uint64_t p0 = hipdbl::calls("launch_pack");
        const int rc = bsw_align_batch(ctx, &p, w.t.data(), n, res.data());
        bsw_set_align_long(0);
        CHECK(rc == BSW_OK, "split: bsw_align_batch -> %d (%s)", rc, bsw_last_error(ctx));
        sub = hipdbl::calls("launch_pack") - p0;
        same_as_oracle(p, w.t, res, D, "split");
        for (size_t k = D; k < n; ++k) CHECK(memcmp(&res[k], &res[k % D], sizeof(bsw_kswr)) == 0, "split: result %zu differs from result %zu of the same task", k, k % D);
        CHECK(sub >= 2, "split: %llu sub-batches", (unsigned long long)sub);
        CHECK(standin_alnl::launches() == 3 * sub && standin_alnl::long_tasks() == n / 4, "split: %llu launches of the long stand-in in %llu sub-batches, %llu long tasks of %zu",
              (unsigned long long)standin_alnl::launches(), (unsigned long long)sub, (unsigned long long)standin_alnl::long_tasks(), n / 4);
        bsw_destroy(ctx);
    }
    CHECK(hipdbl::live_objects() == 0, "split: %zu HIP objects left alive", hipdbl::live_objects());
    printf("split: ok, %llu sub-batches\n", (unsigned long long)sub);
    return 0;
}

static int flip_mode()
{
    const bsw_params p = default_params();
    lcg_genome_t g;
    g.make(40001, 3);
    uint64_t chunks = 0;
    for (int mode = 1; mode <= 2; ++mode) {
        fresh(1);
        standin_alnl::reset();
        lcg_t r(11 + (uint64_t)mode);
        mwork mw;
        for (int k = 0; k < 12; ++k) mw.add(g, r, mode == 1 ? (k % 3 == 0 ? 1025 : k % 3 == 1 ? 1500 : 3000) : 100 + 17 * k, k & 1, (k >> 1) & 1, XF | ((k & 4) ? KSW_XBYTE : 0));
        mw.finish();
        const size_t n = mw.t.size();
        bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2, 60000);
        bsw_ref *ref = nullptr;
        CHECK(bsw_ref_upload(ctx, g.pac.data(), g.l_pac, &ref) == BSW_OK, "bsw_ref_upload: %s", bsw_last_error(ctx));
        for (int k = 0; k < 64; ++k) hipdbl::stall_stream(k);        /* every stream: a slot gets as far as its first chunk's queue */
        std::vector<bsw_mresult> res(n);
        bsw_ticket t = 0;
        bsw_set_align_long(mode);
        const uint64_t la = hipdbl::calls("launch_align");
        CHECK(bsw_matesw_ref_submit_t(ctx, &p, ref, mw.t.data(), n, res.data(), &t) == BSW_OK, "flip: submit under mode %d: %s", mode, bsw_last_error(ctx));
        bsw_set_align_long(0);                                        /* ten of the twelve one-task chunks have not been looked at yet */
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
        CHECK(bsw_test(ctx, t) == 0, "flip: the ticket completed behind stalled streams");
        hipdbl::release_streams();
        CHECK(bsw_wait_ticket(ctx, t) == BSW_OK, "flip: the ticket of mode %d, collected under mode 0: %s", mode, bsw_last_error(ctx));
        same_rescue(p, g, mw, res, "flip");
        CHECK(standin_alnl::tasks() == n && hipdbl::calls("launch_align") == la, "flip: mode %d, %llu of %zu tasks on the long stand-in", mode,
              (unsigned long long)standin_alnl::tasks(), n);
        CHECK(standin_alnl::launches() == n, "flip: %llu launches for %zu one-task chunks", (unsigned long long)standin_alnl::launches(), n);
        chunks += standin_alnl::launches();
        if (mode == 1) {                                              /* what enters now is refused again */
            bsw_ticket t2 = 0;
            CHECK(bsw_matesw_ref_submit_t(ctx, &p, ref, mw.t.data(), n, res.data(), &t2) == BSW_E_LIMIT, "flip: mode 0 took the long mates");
        }
        bsw_ref_free(ctx, ref);
        bsw_destroy(ctx);
        CHECK(hipdbl::live_objects() == 0, "flip: %zu HIP objects left alive", hipdbl::live_objects());
    }
    printf("flip: ok, %llu chunks\n", (unsigned long long)chunks);
    return 0;
}

static int faults_mode()
{
    const bsw_params p = default_params();
    uint64_t long_failed = 0;
    sweep_t s;
    s.releases = {"hipFree", "hipHostFree", "hipGetLastError"};
    s.tickets = false;
    s.exact = true;
    for (int reg = 0; reg < 2; ++reg) {                        /* both memory kinds: the gather and the direct branch */
        std::vector<bsw_kswr> clean;
        fault_sweep(s, 1, [&](sweep_t &s) {
            const unsigned long long k = s.k;
            lcg_t r(31);
            awork w;
            mixed(w, r, true);
            const size_t n = w.t.size();
            uint8_t *arena = nullptr;
            if (reg) {                                     /* one registered arena holds every sequence */
                size_t tot = 64;
                for (const bsw_atask &t : w.t) tot += (size_t)t.qlen + (size_t)t.tlen + 2;
                arena = (uint8_t *)bsw_host_alloc(tot);
                CHECK(arena, "bsw_host_alloc");
                size_t at = 0;
                for (bsw_atask &t : w.t) {
                    memcpy(arena + at, t.query, (size_t)t.qlen); t.query = arena + at; at += (size_t)t.qlen + 1;
                    memcpy(arena + at, t.target, (size_t)t.tlen); t.target = arena + at; at += (size_t)t.tlen + 1;
                }
            }
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2, 3000);
            bsw_set_align_long(1);
            std::vector<bsw_kswr> first(n), again(n);
            memset(first.data(), 0, n * sizeof(bsw_kswr));
            s.arm();
            const int rc = bsw_align_batch(ctx, &p, w.t.data(), n, first.data());
            s.judge({{rc, rc ? bsw_last_error(ctx) : ""}});
            if (k == 0) {
                CHECK(hipdbl::calls("launch_align_long") >= 4, "the batch of the fault sweep makes %llu long launches", (unsigned long long)hipdbl::calls("launch_align_long"));
                same_as_oracle(p, w.t, first, n, "faults, clean");
                clean = first;
            } else if (rc == BSW_OK)                           /* no failure happened, or that of a release */
                CHECK(memcmp(first.data(), clean.data(), n * sizeof(bsw_kswr)) == 0, "k=%llu: %s failed, the call reported success and its results differ", k, s.fname.c_str());
            else
                long_failed += s.fname == "launch_align_long";
            const int rc2 = bsw_align_batch(ctx, &p, w.t.data(), n, again.data());      /* the same call on the same context */
            CHECK(rc2 == BSW_OK, "k=%llu (%s failed): the same call repeated -> %d (%s)", k, s.fname.c_str(), rc2, bsw_last_error(ctx));
            CHECK(memcmp(again.data(), clean.data(), n * sizeof(bsw_kswr)) == 0, "k=%llu (%s failed): the same call repeated is not bit-exact", k, s.fname.c_str());
            bsw_set_align_long(0);
            bsw_destroy(ctx);
            if (arena) bsw_host_free(arena);
        });
    }
    printf("faults: C = %llu, visited %llu, failed %llu, ignored %llu, long launches failed %llu\n", (unsigned long long)s.Csum, (unsigned long long)s.visited,
           (unsigned long long)s.failed, (unsigned long long)s.ignored, (unsigned long long)long_failed);
    s.done();
    return 0;
}

/* the names of the HIP calls of one batch, in order: call k is the one a failure planned for the k-th call overall fires in */
static std::vector<std::string> call_names(int mode, uint64_t *total)
{
    const bsw_params p = default_params();
    std::vector<std::string> names;
    for (uint64_t k = 0;; ++k) {
        fresh(1);
        bool made = true;
        {
            lcg_t r(41);
            awork w;
            mixed(w, r, false);
            const size_t n = w.t.size();
            bsw_ctx *ctx = make_ctx(BSW_KERNEL_AUTO, 1, 256, 2, 3000);
            bsw_set_align_long(mode);
            std::vector<bsw_kswr> res(n);
            hipdbl::reset_counters();
            if (k) hipdbl::fail_overall(k);
            const int rc = bsw_align_batch(ctx, &p, w.t.data(), n, res.data());
            const char *f = hipdbl::fired();
            hipdbl::clear_failures();
            bsw_set_align_long(0);
            if (k == 0) {
                CHECK(rc == BSW_OK, "sequence: the clean call under mode %d -> %d (%s)", mode, rc, bsw_last_error(ctx));
                CHECK(hipdbl::calls("launch_align_long") == 0, "sequence: a batch without long tasks reached the long launcher under mode %d", mode);
                same_as_oracle(p, w.t, res, n, "sequence");
                *total = hipdbl::overall_calls();
            } else if (!f) made = false;
            else names.push_back(f);
            bsw_destroy(ctx);
        }
        if (!made) break;
    }
    return names;
}

static int sequence_mode()
{
    uint64_t c0 = 0, c1 = 0;
    const std::vector<std::string> off = call_names(0, &c0), on = call_names(1, &c1);
    CHECK(c0 == c1 && off.size() == c0 && on.size() == c1, "sequence: %llu calls with the switch off, %llu with it on (%zu / %zu visited)", (unsigned long long)c0,
          (unsigned long long)c1, off.size(), on.size());
    for (size_t k = 0; k < off.size(); ++k) CHECK(off[k] == on[k], "sequence: call %zu is %s with the switch off and %s with it on", k + 1, off[k].c_str(), on[k].c_str());
    CHECK(std::count(off.begin(), off.end(), std::string("launch_align")) >= 4, "sequence: the batch launches fewer than four classes");
    printf("sequence: ok, %llu calls\n", (unsigned long long)c0);
    return 0;
}

int main(int argc, char **argv)
{
    setenv("BSW_F4_MATESW_WORK", "1", 1);                      /* flip: a rescue chunk holds one task */
    unsetenv("BSW_ALIGN_LONG");
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "gate") return gate_mode();
    if (mode == "split") return split_mode();
    if (mode == "flip") return flip_mode();
    if (mode == "faults") return faults_mode();
    if (mode == "sequence") return sequence_mode();
    fprintf(stderr, "usage: host_align_long gate | split | flip | faults | sequence\n");
    return 2;
}
