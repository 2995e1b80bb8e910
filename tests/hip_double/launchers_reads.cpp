/* launchers_reads.cpp — bsw::launch_pack for the host-double programs that use resident read blocks (TEST INFRASTRUCTURE; built
 * by its row in tests/_host_double_build.py, never part of the library).
 *
 * launchers.cpp stays as it is: this builder compiles it a second time with -Dlaunch_pack=launch_pack_bytes, so its byte stand-in
 * (and the ledger of pack launches it keeps for the alignment stand-ins) is reachable under that name, and this file provides
 * launch_pack itself.  A launch without BSW_PACK_STORE goes straight through.  A launch WITH it is restated from the contract of
 * bsw_reads_fetch.h by a nibble loop over the store — base i of the left query at position s - i (when BSW_PACK_REV_LEFT is set)
 * or s + i, of the right query at s + i — into byte sequences in the order the kernels want them, which the byte stand-in then
 * packs.  The store is "device" memory of the double: ASan is the witness that no position leaves the allocation, and the copy
 * handed to a chunk must live on the chunk's device.
 */
#include "../../bwa-mem-sw_amd/csrc/bsw_internal.h"
#include "hip_double.h"
#include "launchers_reads.h"

#include <atomic>
#include <memory>

namespace bsw {
hipError_t launch_pack_bytes(const uint8_t *raw, const bsw_dtask *tasks, const bsw_rawoff *roff, uint32_t bias, uint32_t n, int rev_left,
                             const uint8_t *pac, int64_t l_pac, const bsw_refx *refx, uint64_t *seq, uint8_t *nflag, hipStream_t s);
}

static std::atomic<int> g_max_len{8192};
static std::atomic<uint64_t> g_store_launches{0}, g_store_bases{0};

namespace standin_reads {
void set_max_query_len(int n) { g_max_len = n; }
uint64_t store_launches() { return g_store_launches; }
uint64_t store_bases() { return g_store_bases; }
void reset() { g_store_launches = 0; g_store_bases = 0; }
}  // namespace standin_reads

namespace bsw {

hipError_t launch_pack(const uint8_t *raw, const bsw_dtask *tasks, const bsw_rawoff *roff, uint32_t bias, uint32_t n, int rev_left,
                       const uint8_t *pac, int64_t l_pac, const bsw_refx *refx, uint64_t *seq, uint8_t *nflag, hipStream_t s)
{
    if (!(rev_left & BSW_PACK_STORE)) return launch_pack_bytes(raw, tasks, roff, bias, n, rev_left & BSW_PACK_REV_LEFT, pac, l_pac, refx, seq, nflag, s);
    if (!pac) hipdbl::die("stand-in launch_pack: a store launch without the resident reference");
    if (bias) hipdbl::die("stand-in launch_pack: a store launch with a raw bias");
    const int dev = hipdbl::device_of_stream(s), cap = g_max_len;
    const uint64_t *store = (const uint64_t *)raw;
    /* the byte sequences the byte stand-in packs: two queries of at most `cap` bases per task (the test program says how long its
     * queries get), kept alive behind both launches by a third, empty one */
    auto bytes = std::make_shared<std::vector<uint8_t>>((size_t)n * 2 * (size_t)cap + 64);
    auto ro = std::make_shared<std::vector<bsw_rawoff>>(n ? n : 1);
    const bool back = (rev_left & BSW_PACK_REV_LEFT) != 0;
    hipdbl::enqueue(s, [=]() {
        if (n && hipdbl::device_of_ptr(store, 8) != dev)
            hipdbl::die("stand-in launch_pack: the read block copy handed to a chunk of device %d does not live there", dev);
        const auto base_at = [&](int64_t p) -> uint8_t {
            if (p < 0) hipdbl::die("stand-in launch_pack: position %lld in front of the store", (long long)p);
            return (uint8_t)((store[p >> 4] >> (4 * (p & 15))) & 15u);
        };
        size_t at = 32;
        uint64_t nb = 0;
        for (uint32_t ti = 0; ti < n; ++ti) {
            const bsw_dtask &T = tasks[ti];
            const bsw_rawoff &R = roff[ti];
            bsw_rawoff &O = (*ro)[ti];
            O = bsw_rawoff{0, 0, 0, 0};
            if (T.lqlen > cap || T.rqlen > cap) hipdbl::die("stand-in launch_pack: a query of %d / %d bases, the program announced %d", T.lqlen, T.rqlen, cap);
            if (T.lqlen) {
                O.lq = (uint32_t)at;
                for (int i = 0; i < T.lqlen; ++i) (*bytes)[at++] = base_at(back ? (int64_t)R.lq - i : (int64_t)R.lq + i);
            }
            if (T.rqlen) {
                O.rq = (uint32_t)at;
                for (int i = 0; i < T.rqlen; ++i) (*bytes)[at++] = base_at((int64_t)R.rq + i);
            }
            nb += (uint64_t)T.lqlen + (uint64_t)T.rqlen;
        }
        g_store_launches += 1;
        g_store_bases += nb;
    });
    const hipError_t e = launch_pack_bytes(bytes->data(), tasks, ro->data(), 0u, n, 0, pac, l_pac, refx, seq, nflag, s);
    hipdbl::enqueue(s, [bytes, ro]() {});
    return e;
}

}  // namespace bsw
