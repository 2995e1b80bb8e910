/* launchers_reads_pack.cpp — bsw::launch_reads_pack for the host-double program of the asynchronous read-block upload (TEST
 * INFRASTRUCTURE; built by its row in tests/_host_double_build.py, never part of the library).
 *
 * The kernel's word function (csrc/bsw_reads_pack.h) is restated from its contract by a nibble loop: base j of a read is the byte
 * raw[raw_off + j], stored as min(byte, 4) in nibble j & 15 of word woff + (j >> 4); the nibbles behind the last base are zero; a
 * read of length 0 writes nothing.  The raw buffer and the store are "device" memory of the double: ASan is the witness that no
 * offset leaves an allocation, and the stand-in dies when either does not live on the stream's device. */
#include "../../bwa-mem-sw_amd/csrc/bsw_internal.h"
#include "../../bwa-mem-sw_amd/csrc/bsw_reads_pack.h"
#include "hip_double.h"

#include <atomic>

static std::atomic<uint64_t> g_launches{0}, g_reads{0};

namespace standin_rdpack {
uint64_t launches() { return g_launches; }
uint64_t reads() { return g_reads; }
void reset() { g_launches = 0; g_reads = 0; }
}  // namespace standin_rdpack

namespace bsw {

hipError_t launch_reads_pack(const uint8_t *raw, const bsw_rdpack_rec *rec, uint32_t n, uint64_t *store, hipStream_t s)
{
    const hipError_t g = hipdbl::gate("launch_reads_pack");
    if (g != hipSuccess) return g;
    const int dev = hipdbl::device_of_stream(s);
    hipdbl::enqueue(s, [=]() {
        if (n && (hipdbl::device_of_ptr(raw, 1) != dev || hipdbl::device_of_ptr(rec, sizeof(*rec)) != dev))
            hipdbl::die("stand-in launch_reads_pack: the raw bytes or the records of a piece of device %d do not live there", dev);
        for (uint32_t i = 0; i < n; ++i) {
            const bsw_rdpack_rec R = rec[i];
            if (R.len < 0) hipdbl::die("stand-in launch_reads_pack: record %u has length %d", i, R.len);
            if (R.len && hipdbl::device_of_ptr(store + R.woff, 8 * (size_t)((R.len + 15) >> 4)) != dev)
                hipdbl::die("stand-in launch_reads_pack: the words of read %u leave the copy of device %d", i, dev);
            for (int j = 0; j < R.len; ++j) {
                const uint8_t b = raw[(size_t)R.raw_off + (size_t)j];
                uint64_t &w = store[(size_t)R.woff + (size_t)(j >> 4)];
                if (!(j & 15)) w = 0;
                w |= (uint64_t)(b > 4 ? 4 : b) << (4 * (j & 15));
            }
        }
        g_launches += 1;
        g_reads += n;
    });
    return hipSuccess;
}

}  // namespace bsw
