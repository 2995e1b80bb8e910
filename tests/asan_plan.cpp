// Sanitizer run of the batch plan (validation, chunk layout, class counts, plan replay): the host-side .hip files compiled host-only
// with -fsanitize=address,undefined and linked against the host-memory HIP stand-in and the CPU stand-ins of the kernel launchers
// (tests/hip_double/: the class tables live there, one copy for every test program).
//   asan_plan        the small plans
//   asan_plan big    more than 100 000 two-sided 250 bp seeds under BSW_KERNEL_AUTO with order[] sized EXACTLY as the header documents
//                    (BSW_LANE_FUSE / BSW_NSPLIT are read once per process: the caller sets them, one run per switch set)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "bwa_sw_mi355.h"

// the capacity of order[] that include/bwa_sw_mi355.h documents for bsw_plan_batch
static size_t documented_capacity(size_t n) { return bsw_plan_order_capacity(n); }

static int big()
{
    bsw_params p; bsw_default_params(&p);
    bsw_synth_spec sp; memset(&sp, 0, sizeof(sp));
    sp.seed = 9; sp.read_len = 250; sp.seed_len_min = 19; sp.seed_len_max = 60; sp.sub_rate = 0.03; sp.indel_rate = 0.01;
    sp.n_rate = 0.0001; sp.junk_frac = 0.1; sp.a = 1; sp.w = 100; sp.o = 6; sp.e = 1;
    size_t worst = 0, worst_n = 0;
    for (size_t n : {size_t(100001), size_t(120000), size_t(200000)}) {
        std::vector<uint8_t> arena(bsw_synth_arena_bound(&sp, n));
        std::vector<bsw_task> tasks(n);
        if (bsw_synth_generate(&sp, n, tasks.data(), arena.data(), arena.size()) < 0) return 1;
        uint32_t *order = (uint32_t *)malloc(documented_capacity(n) * sizeof(uint32_t));      // (exactly: ASan guards the word behind it)
        std::vector<uint32_t> seg(BSW_PLAN_SEGS + 1);
        if (bsw_plan_batch(&p, tasks.data(), n, BSW_KERNEL_AUTO, 1, order, seg.data()) < 0) return 2;
        if (seg[BSW_PLAN_SEGS] > documented_capacity(n)) return 3;
        if (seg[BSW_PLAN_SEGS] * n > worst * (worst_n ? worst_n : 1) || !worst) { worst = seg[BSW_PLAN_SEGS]; worst_n = n; }
        printf("asan_plan big: n %zu, order_len %u, 4n+16 = %zu, documented %zu\n", n, seg[BSW_PLAN_SEGS], 4 * n + 16, documented_capacity(n));
        free(order);
    }
    puts("asan_plan big ok");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "big")) return big();
    bsw_params p; bsw_default_params(&p);
    bsw_synth_spec sp; memset(&sp, 0, sizeof(sp));
    sp.seed = 3; sp.read_len = 250; sp.seed_len_min = 19; sp.seed_len_max = 80; sp.sub_rate = 0.03; sp.indel_rate = 0.01;
    sp.n_rate = 0.003; sp.junk_frac = 0.1; sp.a = 1; sp.w = 100; sp.o = 6; sp.e = 1;
    for (size_t n : {size_t(0), size_t(1), size_t(63), size_t(5000), size_t(20000)}) {
        std::vector<uint8_t> arena(bsw_synth_arena_bound(&sp, n));
        std::vector<bsw_task> tasks(n ? n : 1);
        if (bsw_synth_generate(&sp, n, tasks.data(), arena.data(), arena.size()) < 0) return 1;
        for (int kernel = 0; kernel < 3; ++kernel)
            for (int threads : {1, 5}) {
                std::vector<uint32_t> order(documented_capacity(n)), seg(BSW_PLAN_SEGS + 1);
                if (bsw_plan_batch(&p, tasks.data(), n, kernel, threads, order.data(), seg.data()) < 0) return 2;
                if (seg[BSW_PLAN_SEGS] > documented_capacity(n)) return 3;
            }
    }
    uint8_t b[77]; uint64_t w[5];
    for (int i = 0; i < 77; ++i) b[i] = (uint8_t)(i * 37);
    for (int len = 0; len <= 77; ++len) bsw_pack_bases(b, len, w);
    puts("asan_plan ok");
    return 0;
}
