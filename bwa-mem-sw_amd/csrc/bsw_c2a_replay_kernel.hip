/*
 * bsw_c2a_replay_kernel.hip — mem_chain2aln's seed loop on the GPU (gfx950): the whole of the companion library libbwasw_c2a.so.
 * The loop itself is bsw_c2a_core.h; here are its device policy, the three kernels of a launch, the launcher, and the constructor
 * that hands the launcher to libbwasw_mi355.so (bsw_c2a_device_register) when this library is loaded.
 *
 *   bsw_c2a_replay_kernel   one 16-lane DPP row per read, four reads per wavefront.  The row's lanes stripe over the read's regions
 *                           for the explains vote and over the chain's seeds for the un-skip vote, the next-key maximum and the
 *                           seedcov sum.  The per-seed state is one bit per owned seed in a register (seed i belongs to lane
 *                           i % 16, bit i / 16: BSW_C2A_DEV_MAX_CHAIN = 16 x 32), so nothing but regions and flags touches memory.
 *                           Every loop is bounded by the chain's n_seeds or the read's region count: there is no wait.
 *   bsw_c2a_scan_kernel     exclusive prefix sums of the per-read counts, one workgroup (the order comes from here, not from atomics)
 *   bsw_c2a_move_kernel     a row per read moves its regions to their compact place, 16 bytes per lane and step
 *
 * The rows of a wavefront run different trip counts; all cross-lane traffic stays inside a row, whose lanes are always active
 * together (the loop structure outside the strided loops is row-uniform).  Plain C++ and vector stores only.
 */
#include <hip/hip_runtime.h>

#include "bsw_c2a_core.h"

namespace bsw {

/* the value of the lane N places to the right in the 16-lane DPP row (row_ror: the rotation stays inside the row) */
template <int N>
__device__ __forceinline__ uint32_t c2a_row_ror(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x120 + N, 0xf, 0xf, false);
}

/* Votes by ballot, reductions by DPP row rotations of 8, 4, 2 and 1 lanes: after the four steps every lane of the row holds the
 * reduction over all sixteen (maximum and wrap-around sum are commutative and associative, so the order does not matter). */
struct c2a_row_policy {
    enum { W = 16 };
    uint32_t ln, shift, ext;
    __device__ uint32_t lane() const { return ln; }
    __device__ bool any(bool b) const { return ((__ballot(b) >> shift) & 0xffffull) != 0; }
    template <int N>
    __device__ static uint64_t max_step(uint64_t v)
    {
        const uint64_t o = (uint64_t)c2a_row_ror<N>((uint32_t)(v >> 32)) << 32 | c2a_row_ror<N>((uint32_t)v);
        return o > v ? o : v;
    }
    __device__ uint64_t max_u64(uint64_t v) const { return max_step<1>(max_step<2>(max_step<4>(max_step<8>(v)))); }
    __device__ uint32_t sum_u32(uint32_t v) const
    {
        v += c2a_row_ror<8>(v);
        v += c2a_row_ror<4>(v);
        v += c2a_row_ror<2>(v);
        v += c2a_row_ror<1>(v);
        return v;
    }
    __device__ void clear() { ext = 0; }
    __device__ void set(uint32_t i) { ext |= 1u << (i >> 4); }
    __device__ bool get(uint32_t i) const { return (ext >> (i >> 4)) & 1u; }
};

#define C2A_BLOCK 256

__global__ __launch_bounds__(C2A_BLOCK) void bsw_c2a_replay_kernel(const c2a_dread *reads, uint32_t n_reads, const c2a_dchain *chains, const bsw_cseed *seeds,
                                                                   uint32_t seed_base, const char *results, uint32_t stride, c2a_dpar par, bsw_creg *stage,
                                                                   uint32_t *counts, uint8_t *flags)
{
    const uint32_t tid = blockIdx.x * C2A_BLOCK + threadIdx.x, row = tid >> 4;
    if (row >= n_reads) return;
    c2a_row_policy pol;
    pol.ln = tid & 15u; pol.shift = threadIdx.x & 48u; pol.ext = 0;
    const c2a_dread rd = reads[row];
    uint32_t cnt = 0;
    if (rd.host) {
        for (uint32_t i = pol.ln; i < rd.n_seeds; i += 16) flags[rd.seed0 + i] = 0;
    } else {
        cnt = c2a_replay_read(pol, par, chains + rd.chain0, rd.n_chains, seeds, seed_base, results, stride, stage + rd.seed0, flags);
    }
    if (pol.ln == 0) counts[row] = cnt;
}

#define C2A_SCAN_THREADS 1024
__global__ __launch_bounds__(C2A_SCAN_THREADS) void bsw_c2a_scan_kernel(const uint32_t *counts, uint32_t n, uint32_t *offs)
{
    __shared__ uint32_t part[C2A_SCAN_THREADS];
    const uint32_t t = threadIdx.x, per = (n + C2A_SCAN_THREADS - 1) / C2A_SCAN_THREADS;
    const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += counts[i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < C2A_SCAN_THREADS; d <<= 1) {          /* inclusive scan of the partial sums */
        const uint32_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t at = part[t] - sum;
    for (uint32_t i = lo; i < hi; ++i) { offs[i] = at; at += counts[i]; }
    if (t == C2A_SCAN_THREADS - 1) offs[n] = part[t];
}

__global__ __launch_bounds__(C2A_BLOCK) void bsw_c2a_move_kernel(const c2a_dread *reads, uint32_t n_reads, const bsw_creg *stage, const uint32_t *counts,
                                                                 const uint32_t *offs, bsw_creg *out)
{
    const uint32_t tid = blockIdx.x * C2A_BLOCK + threadIdx.x, row = tid >> 4, ln = tid & 15u;
    if (row >= n_reads) return;
    const uint4 *src = (const uint4 *)(stage + reads[row].seed0);
    uint4 *dst = (uint4 *)(out + offs[row]);
    const uint32_t words = counts[row] * (uint32_t)(sizeof(bsw_creg) / sizeof(uint4));
    for (uint32_t k = ln; k < words; k += 16) dst[k] = src[k];
}

static int c2a_launch(const c2a_dev_args *a, void *stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (!a || !a->n_reads) return (int)hipSuccess;
    const uint32_t rows_per_block = C2A_BLOCK / 16, grid = (a->n_reads + rows_per_block - 1) / rows_per_block;
    hipLaunchKernelGGL(bsw_c2a_replay_kernel, dim3(grid), dim3(C2A_BLOCK), 0, s, a->reads, a->n_reads, a->chains, a->seeds, a->seed_base,
                       (const char *)a->results, a->stride, a->par, a->stage, a->counts, a->flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(bsw_c2a_scan_kernel, dim3(1), dim3(C2A_SCAN_THREADS), 0, s, (const uint32_t *)a->counts, a->n_reads, a->offs);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    hipLaunchKernelGGL(bsw_c2a_move_kernel, dim3(grid), dim3(C2A_BLOCK), 0, s, a->reads, a->n_reads, (const bsw_creg *)a->stage, (const uint32_t *)a->counts,
                       (const uint32_t *)a->offs, a->out);
    return (int)hipGetLastError();
}

}  // namespace bsw

static const c2a_dev_ops g_c2a_ops = {bsw::c2a_launch};
__attribute__((constructor)) static void c2a_register_launcher() { (void)bsw_c2a_device_register(&g_c2a_ops); }
