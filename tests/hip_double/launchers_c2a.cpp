/* launchers_c2a.cpp — the CPU stand-in of the chain2aln replay launcher for the host-double program of bsw_c2a_device.hip (TEST
 * INFRASTRUCTURE; built by the row tests/test_c2a_device_cpu.py adds to tests/_host_double_build.py, never part of the library).
 * It is the companion library's place: a constructor registers a launcher with the main library's unit.  The launcher runs
 * bsw_c2a_core.h — the header the kernel is compiled from — with the CPU policy, on the stream's worker. */
#include "hip_double.h"
#include "../../bwa-mem-sw_amd/csrc/bsw_c2a_core.h"

#include <atomic>

static std::atomic<uint64_t> g_launches{0}, g_reads{0};
namespace standin_c2a {
uint64_t launches() { return g_launches; }
uint64_t reads() { return g_reads; }
}  // namespace standin_c2a

static int c2a_standin_launch(const c2a_dev_args *a_, void *stream)
{
    const hipError_t g = hipdbl::gate("launch_c2a_replay");
    if (g != hipSuccess) return (int)g;
    const c2a_dev_args a = *a_;
    hipdbl::enqueue((hipStream_t)stream, [a]() {
        c2a_cpu_launch(&a);
        g_launches += 1;
        g_reads += a.n_reads;
    });
    return (int)hipSuccess;
}

static const c2a_dev_ops g_ops = {c2a_standin_launch};
__attribute__((constructor)) static void c2a_standin_register() { (void)bsw_c2a_device_register(&g_ops); }
