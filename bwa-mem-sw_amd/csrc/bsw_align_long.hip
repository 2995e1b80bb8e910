/*
 * bsw_align_long.hip — the switch of ksw_align2's long-query route (bsw_set_align_long, BSW_ALIGN_LONG), its launch counters,
 * and the one place that names the launcher of bsw_align_long_kernel.hip (part of the host side of libbwasw_mi355.so; shared
 * types: bsw_internal.h).
 *
 * The hosts of the local alignment (bsw_f4.hip, bsw_matesw.hip) never refer to launch_align_long: they hold a pointer to the
 * table below, which this unit registers when the library is loaded.  A program that links those two units without this one (the
 * host-double test programs of before the route) sees a NULL table and behaves as mode 0.
 */
#include "bsw_internal.h"

#define ALIGN_LONG_MAX_CLASSES 32

static std::atomic<int> &align_long_switch()
{
    static std::atomic<int> mode([] {
        const char *e = getenv("BSW_ALIGN_LONG");
        return (e && (e[0] == '1' || e[0] == '2') && e[1] == 0) ? e[0] - '0' : 0;
    }());
    return mode;
}
static std::atomic<uint64_t> g_align_long_launches[ALIGN_LONG_MAX_CLASSES];

static int al_mode() { return align_long_switch().load(std::memory_order_relaxed); }
static int al_class_count() { return std::min(bsw::align_long_class_count(), ALIGN_LONG_MAX_CLASSES); }
static int al_class_of(int qlen, int byte_mode)
{
    const int c = bsw::align_long_class_of(qlen, byte_mode);
    return c < al_class_count() ? c : -1;
}
static hipError_t al_launch(int cls, const bsw_dparams &P, const uint64_t *seq, const bsw_adtask *tasks, const uint32_t *order, uint32_t n,
                            unsigned long long *blist, bsw_kswr *out, hipStream_t s)
{
    if (cls < 0 || cls >= al_class_count()) return hipErrorInvalidValue;
    const hipError_t e = bsw::launch_align_long(cls, P, seq, tasks, order, n, blist, out, s);
    if (e == hipSuccess && n) g_align_long_launches[cls].fetch_add(1, std::memory_order_relaxed);
    return e;
}

static const align_long_ops g_ops = {al_mode, al_class_count, al_class_of, al_launch};
static const struct align_long_registrar {
    align_long_registrar() { align_long_register(&g_ops); }
} g_registrar;

extern "C" void bsw_set_align_long(int mode) { align_long_switch().store(mode == 1 || mode == 2 ? mode : 0, std::memory_order_relaxed); }
extern "C" int bsw_align_long(void) { return al_mode(); }
extern "C" int bsw_align_long_stats(uint64_t *launches, int cap)
{
    const int n = al_class_count();
    for (int c = 0; c < n && c < cap && launches; ++c) launches[c] = g_align_long_launches[c].load(std::memory_order_relaxed);
    return n;
}
