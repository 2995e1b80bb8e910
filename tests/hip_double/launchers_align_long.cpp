/* launchers_align_long.cpp — bsw::launch_align_long and its class functions for the host-double program of ksw_align2's
 * long-query route (TEST INFRASTRUCTURE; built by its row in tests/_host_double_build.py, never part of the library).
 *
 * The class table is restated from the header's contract (bsw_align_long_stats: 8-bit mode slen bounds 16 .. 512, then 16-bit mode
 * 32 .. 1 024, slen = ceil(qlen / lanes)).  The stand-in computes every listed task with oracle/ksw_align_ref.c from the staged
 * words and dies when a task is listed for a class other than its own.  (The stand-in of launch_align in launchers.cpp already
 * dies when a task of more than 1 024 bases reaches it: no class of bsw_align_kernel is that task's.) */
#include "../../bwa-mem-sw_amd/csrc/bsw_internal.h"
#include "../../oracle/ksw_extend_ref.h"
#include "hip_double.h"

#include <algorithm>
#include <atomic>
#include <vector>

extern "C" void ksw_align2_ref(int qlen, const uint8_t *query, int tlen, const uint8_t *target, int m, const int8_t *mat,
                               int o_del, int e_del, int o_ins, int e_ins, int xtra, int32_t *out, uint64_t *cells);

static std::atomic<uint64_t> g_launches[12], g_tasks{0}, g_long_tasks{0};

namespace standin_alnl {
uint64_t launches(int cls) { return g_launches[cls]; }
uint64_t launches()
{
    uint64_t s = 0;
    for (int c = 0; c < 12; ++c) s += g_launches[c];
    return s;
}
uint64_t tasks() { return g_tasks; }
uint64_t long_tasks() { return g_long_tasks; }           /* tasks of more than BSW_ALIGN_MAX_QLEN bases */
void reset()
{
    for (int c = 0; c < 12; ++c) g_launches[c] = 0;
    g_tasks = 0; g_long_tasks = 0;
}
}  // namespace standin_alnl

namespace bsw {

static const int kByte[] = {16, 32, 64, 128, 256, 512}, kWord[] = {32, 64, 128, 256, 512, 1024};
int align_long_class_count() { return 12; }
int align_long_class_of(int qlen, int byte_mode)
{
    if (qlen > BSW_ALIGN_LONG_MAX_QLEN) return -1;
    const int lanes = byte_mode ? 16 : 8, slen = (qlen + lanes - 1) / lanes;
    for (int k = 0; k < 6; ++k)
        if (slen <= (byte_mode ? kByte[k] : kWord[k])) return (byte_mode ? 0 : 6) + k;
    return -1;
}

hipError_t launch_align_long(int cls, const bsw_dparams &P_, const uint64_t *seq, const bsw_adtask *tasks, const uint32_t *order, uint32_t n,
                             unsigned long long *blist, bsw_kswr *out, hipStream_t s)
{
    const hipError_t g = hipdbl::gate("launch_align_long");
    if (g != hipSuccess) return g;
    if (cls < 0 || cls >= align_long_class_count()) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const bsw_dparams P = P_;
    const int dev = hipdbl::device_of_stream(s);
    hipdbl::enqueue(s, [=]() {
        if (hipdbl::device_of_ptr(order, 4 * (size_t)n) != dev) hipdbl::die("stand-in launch_align_long: the order segment of class %d does not live on device %d", cls, dev);
        std::vector<uint8_t> q, t;
        for (uint32_t slot = 0; slot < n; ++slot) {
            const uint32_t idx = order[slot];
            const bsw_adtask &T = tasks[idx];
            const int want = align_long_class_of(T.qlen, (T.xtra & KSW_XBYTE) != 0);
            if (want != cls) hipdbl::die("stand-in launch_align_long: task %u (%d query bases, xtra 0x%x) belongs to class %d and is listed for class %d", idx, T.qlen, (unsigned)T.xtra, want, cls);
            const uint64_t blen = (T.xtra & KSW_XSUBO) ? (uint64_t)T.tlen : 0;
            if (blen) { blist[T.b_off] = 0; blist[T.b_off + blen - 1] = 0; }      /* (ASan: the slice lies inside the scratch) */
            q.resize((size_t)T.qlen); t.resize((size_t)T.tlen);
            for (int k = 0; k < T.qlen; ++k) q[(size_t)k] = (uint8_t)((seq[T.q_off + (uint32_t)(k >> 4)] >> ((k & 15) * 4)) & 15);
            for (int k = 0; k < T.tlen; ++k) t[(size_t)k] = (uint8_t)((seq[T.t_off + (uint32_t)(k >> 4)] >> ((k & 15) * 4)) & 15);
            if (T.pad & BSW_AD_QRC) {
                std::reverse(q.begin(), q.end());
                for (uint8_t &c : q) c = c < 4 ? (uint8_t)(3 - c) : (uint8_t)4;
            }
            int32_t r[7];
            ksw_align2_ref(T.qlen, q.data(), T.tlen, t.data(), 5, P.mat, P.o_del, P.e_del, P.o_ins, P.e_ins, T.xtra, r, nullptr);
            memcpy(&out[idx], r, sizeof(bsw_kswr));
            if (T.qlen > BSW_ALIGN_MAX_QLEN) g_long_tasks += 1;
        }
        g_launches[cls] += 1;
        g_tasks += n;
    });
    return hipSuccess;
}

}  // namespace bsw
