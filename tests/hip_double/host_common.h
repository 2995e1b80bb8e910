/* host_common.h — what the host-double test programs share: workloads, expected results from the oracle, checks, the random
 * stream, uploads, and the driver of the single-failure sweeps.
 * TEST INFRASTRUCTURE (tests/test_host_double_cpu.py builds and runs the programs). */
#ifndef BSW_HOST_COMMON_H
#define BSW_HOST_COMMON_H

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "bwa_sw_mi355.h"
#include "../../oracle/ksw_extend_ref.h"
#include "hip_double.h"
#include "launchers.h"

extern "C" void rtl_ref_pair_batch(const bsw_params *p, const bsw_task *tasks, size_t n, bsw_result *out);
extern "C" void rtl_ref_ext_batch(const bsw_params *p, const bsw_ext_task *tasks, size_t n, bsw_ext *out);

#define CHECK(cond, ...)                                                         \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                                        \
            fputc('\n', stderr);                                                 \
            fflush(stderr);                                                      \
            abort();                                                             \
        }                                                                        \
    } while (0)

struct workload {
    std::vector<bsw_task> tasks;
    uint8_t *arena = nullptr;                        /* malloc, or bsw_host_alloc when registered */
    size_t arena_len = 0;
    bool registered = false;
    ~workload() { if (registered) bsw_host_free(arena); else free(arena); }
    workload() = default;
    workload(const workload &) = delete;
    workload &operator=(const workload &) = delete;
};

/* bsw_synth reads of 150 or 250 bases with Ns and junk flanks, two-sided (seed anywhere) unless one_sided; tag = index */
inline void make_workload(workload &w, size_t n, int read_len, uint64_t seed, bool registered, bool one_sided = false, double n_rate = 0.004)
{
    bsw_synth_spec sp;
    memset(&sp, 0, sizeof(sp));
    sp.seed = seed; sp.read_len = read_len; sp.seed_len_min = 19; sp.seed_len_max = read_len == 250 ? 60 : 40;
    sp.seed_at_start = one_sided ? 1 : 0;
    sp.sub_rate = 0.03; sp.indel_rate = 0.008; sp.n_rate = n_rate; sp.junk_frac = 0.1;
    sp.a = 1; sp.w = 100; sp.o = 6; sp.e = 1;
    w.arena_len = bsw_synth_arena_bound(&sp, n) + 64;
    w.registered = registered;
    w.arena = (uint8_t *)(registered ? bsw_host_alloc(w.arena_len) : malloc(w.arena_len));
    CHECK(w.arena, "arena of %zu bytes", w.arena_len);
    memset(w.arena, 0, w.arena_len);
    w.tasks.resize(n ? n : 1);
    CHECK(bsw_synth_generate(&sp, n, w.tasks.data(), w.arena, w.arena_len) >= 0, "bsw_synth_generate");
    w.tasks.resize(n);
    for (size_t i = 0; i < n; ++i) w.tasks[i].tag = (uint32_t)i;
}

/* the oracle's pair batch on 8 threads (BSW_VARIANT_RTL: tests/ksw_extend_rtl_ref.c) */
inline std::vector<bsw_result> expected(const bsw_params &p, const bsw_task *tasks, size_t n)
{
    std::vector<bsw_result> out(n);
    if (!n) return out;
    if (p.variant == BSW_VARIANT_RTL) {
        const int T = 8;
        std::vector<std::thread> th;
        for (int k = 0; k < T; ++k)
            th.emplace_back([&, k]() { const size_t lo = n * (size_t)k / T, hi = n * (size_t)(k + 1) / T; rtl_ref_pair_batch(&p, tasks + lo, hi - lo, out.data() + lo); });
        for (auto &t : th) t.join();
    } else
        bsw_pair_batch_ref(&p, tasks, n, out.data(), 8);
    return out;
}

inline void same_results(const bsw_result *got, const bsw_result *want, size_t n, const char *what)
{
    for (size_t i = 0; i < n; ++i)
        if (memcmp(&got[i], &want[i], sizeof(bsw_result)) != 0)
            CHECK(false, "%s: record %zu of %zu differs from the oracle (tag %u / %u, score %d / %d, truesc %d / %d, left cells %u / %u)", what, i, n,
                  got[i].tag, want[i].tag, got[i].score, want[i].score, got[i].truesc, want[i].truesc, got[i].left.cells, want[i].left.cells);
}

inline bsw_ctx *make_ctx(int kernel, int n_dev, size_t chunk_tasks, int streams = 2, int timeout_ms = 20000, const int *devices = nullptr)
{
    bsw_config c;
    bsw_default_config(&c);
    c.kernel = kernel; c.streams = streams; c.pack_threads = 4; c.chunk_tasks = chunk_tasks; c.timeout_ms = timeout_ms;
    c.n_devices = n_dev;
    for (int k = 0; k < n_dev; ++k) c.devices[k] = devices ? devices[k] : k;
    bsw_ctx *ctx = nullptr;
    const int rc = bsw_create(&c, &ctx);
    CHECK(rc == BSW_OK && ctx, "bsw_create -> %d", rc);
    return ctx;
}

inline void fresh(int n_devices)
{
    hipdbl::reset(n_devices);
    standin::reset();
}

/* splitmix64: the random stream of every workload but host_align_long's and host_reads_enc's (their own 32-bit generators) */
struct rng_t {
    uint64_t s;
    explicit rng_t(uint64_t seed) : s(seed * 0x9e3779b97f4a7c15ull + 1) {}
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    int in(int lo, int hi) { return lo + below(hi - lo + 1); }           /* inclusive */
    double unit() { return (double)(next() >> 11) / 9007199254740992.0; }
};

inline bsw_params default_params()
{
    bsw_params p;
    bsw_default_params(&p);
    return p;
}
/* a genome of any layout that has pac and l_pac */
template <class G>
bsw_ref *upload(bsw_ctx *ctx, const G &g)
{
    bsw_ref *ref = nullptr;
    CHECK(bsw_ref_upload(ctx, g.pac.data(), g.l_pac, &ref) == BSW_OK && ref, "bsw_ref_upload: %s", bsw_last_error(ctx));
    return ref;
}
/* a workload of any kind that has its reads as ptr[] and len[] */
template <class W>
bsw_reads *upload_reads(bsw_ctx *ctx, const W &w)
{
    bsw_reads *rd = nullptr;
    CHECK(bsw_reads_upload(ctx, w.ptr.data(), w.len.data(), w.ptr.size(), &rd) == BSW_OK && rd, "bsw_reads_upload: %s", bsw_last_error(ctx));
    return rd;
}
inline bsw_stats stats_of(bsw_ctx *ctx)
{
    bsw_stats s;
    memset(&s, 0, sizeof(s));
    CHECK(bsw_host_stats(ctx, &s, sizeof(s)) == BSW_OK, "bsw_host_stats");
    return s;
}

/* ---- the single-failure sweep.  Run 0 of a scenario is clean and counts the HIP and launcher calls of its window (C); run k lets
 * call k of the window fail, k = 1, 2, ... until a run ends without having made call k: call C + 1 is never made.  A scenario
 * builds its context, opens the window with arm(), makes the calls under test, closes it with judge() — handing over what each
 * call answered — and then checks results, reruns and tears down.  The rules judge() holds every run to: exactly one call under
 * test fails per injected failure, with a text of its own and BSW_E_HIP, or BSW_E_NOMEM after a failed allocation (a ticket may
 * answer either then, a synchronous call must answer BSW_E_NOMEM); all of them may succeed only when the failed call is one of
 * `releases`, whose code the library ignores by design.  fault_sweep() adds the balance of HIP objects around every run.  The
 * program prints its own summary from the tallies, then calls done(). ---- */
struct sweep_t {
    std::vector<std::string> releases;
    bool tickets = true;                 /* the calls under test are tickets or jobs of the pipeline, not synchronous batch calls */
    bool exact = false;                  /* the window makes the same calls in every run: the sweep ends at k = C + 1 and visits all C;
                                            otherwise threads decide how many calls a run makes, and it must end past 9/10 of C */
    uint64_t min_visited = 0, min_failed = 0;
    uint64_t k = 0, C = 0, Csum = 0, visited = 0, failed = 0, ignored = 0;       /* C: of this sweep; the others add up over sweeps */
    std::string fname;                   /* the call that failed in this run; empty: none */
    bool over = false;

    void arm()
    {
        hipdbl::reset_counters();
        if (k) hipdbl::fail_overall(k);
    }
    struct answer { int rc; std::string text; };
    void judge(const std::vector<answer> &calls)
    {
        const char *f = hipdbl::fired();
        fname = f ? f : "";
        const uint64_t made = hipdbl::overall_calls();
        hipdbl::clear_failures();
        int nfail = 0;
        for (const answer &a : calls) nfail += a.rc != 0;
        const unsigned long long kk = k;
        if (k == 0) {
            C = made;
            Csum += C;
            for (const answer &a : calls) CHECK(a.rc == 0, "the clean scenario -> %d (%s)", a.rc, a.text.c_str());
        } else if (!f) {
            if (exact) CHECK(k == C + 1 && made == C, "call %llu of the scenario was never made: this run made %llu calls, the clean one %llu", kk, (unsigned long long)made, (unsigned long long)C);
            else CHECK(k > made && 10 * k > 9 * C, "call %llu of the scenario was never made (this run made %llu, the clean one %llu)", kk, (unsigned long long)made, (unsigned long long)C);
            CHECK(nfail == 0, "k=%llu: no failure happened and a call failed", kk);
            over = true;
        } else {
            ++visited;
            if (nfail) {
                ++failed;
                CHECK(nfail == 1, "k=%llu: %s failed once and %d calls failed", kk, fname.c_str(), nfail);
                const bool alloc = fname == "hipMalloc" || fname == "hipHostMalloc";
                for (size_t j = 0; j < calls.size(); ++j)
                    if (calls[j].rc) {
                        CHECK(tickets ? calls[j].rc == BSW_E_HIP || (alloc && calls[j].rc == BSW_E_NOMEM) : calls[j].rc == (alloc ? BSW_E_NOMEM : BSW_E_HIP), "k=%llu: %s failed and call %zu answered %d (%s)", kk, fname.c_str(), j, calls[j].rc, calls[j].text.c_str());
                        CHECK(!calls[j].text.empty() && (!tickets || calls[j].text.compare(0, 7, "aborted") != 0), "k=%llu: %s failed, call %zu reports '%s'", kk, fname.c_str(), j, calls[j].text.c_str());
                    }
            } else {
                ++ignored;
                bool known = false;
                for (const std::string &r : releases) known = known || r == fname;
                CHECK(known, "k=%llu: %s failed and every call reported success", kk, fname.c_str());
            }
        }
    }
    void done() const
    {
        CHECK(visited >= min_visited && failed >= min_failed && (!exact || visited == Csum), "the sweep visited %llu of %llu calls, %llu failed", (unsigned long long)visited,
              (unsigned long long)Csum, (unsigned long long)failed);
    }
};

/* runs scenario(s) for k = 0, 1, ... on n_devices fresh devices until judge() has seen the run that no longer makes call k; the
 * tallies add up over several sweeps with one sweep_t */
template <class F>
void fault_sweep(sweep_t &s, int n_devices, F scenario)
{
    s.over = false;
    for (s.k = 0; !s.over; ++s.k) {
        fresh(n_devices);
        const size_t live0 = hipdbl::live_objects();
        scenario(s);
        CHECK(hipdbl::live_objects() == live0, "k=%llu (%s failed): %zu HIP objects left alive after the scenario", (unsigned long long)s.k, s.fname.c_str(), hipdbl::live_objects() - live0);
    }
}

#endif
