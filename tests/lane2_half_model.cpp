// CPU model of bsw_lane2_kernel with the KERNEL's choice of block bodies (TEST INFRASTRUCTURE): tests/lane2_model.cpp as it
// is, compiled with BSW_L2_KERNEL_DISPATCH — no column-by-column first block, the column-by-column last block only in the
// top blocks of the class — so that the half-block skips of lane2::block8h run wherever the GPU kernel runs them, and with
// a counter of what the rows of a run reached (tests/test_lane2_half_blocks_cpu.py asserts its shapes reach every case).
// g++ -O2 -std=c++17 -shared -fPIC -I include -o lane2_half_model.so tests/lane2_half_model.cpp
#include <cstring>

// [0..8) rows by jlo & 7, [8..16) rows by jhi & 7, [16] skip-low in a dense block, [17] skip-low in an edge block,
// [18] skip-high, [19] skip-low and skip-high in one BLOCK (each counted once per lane of the wave)
static unsigned long long half_stats[20];
static inline void lane2_half_stat(int jl, int jh, bool low_dense, bool low_edge, bool high, bool both)
{
    ++half_stats[jl]; ++half_stats[8 + jh];
    half_stats[16] += low_dense; half_stats[17] += low_edge; half_stats[18] += high;
    half_stats[19] += both;
}
#define BSW_L2_KERNEL_DISPATCH 1
#define BSW_L2_SKIP_STATS(jl, jh, ld, le, he, both) lane2_half_stat(jl, jh, ld, le, he, both)

#include "lane2_model.cpp"

extern "C" void lane2_half_stats(unsigned long long *out, int reset)
{
    if (out) memcpy(out, half_stats, sizeof(half_stats));
    if (reset) memset(half_stats, 0, sizeof(half_stats));
}
