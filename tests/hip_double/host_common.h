/* host_common.h — what the host-double test programs share: workloads, expected results from the oracle, checks.
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

#endif
