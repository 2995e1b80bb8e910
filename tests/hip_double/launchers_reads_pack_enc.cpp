/* launchers_reads_pack_enc.cpp — bsw::launch_reads_pack for the host-double program of the upload encodings (TEST INFRASTRUCTURE;
 * built by its row in tests/_host_double_build.py in place of launchers_reads_pack.cpp, never part of the library).
 *
 * The kernel's word function (csrc/bsw_reads_pack.h) is restated from its contract per base, honouring the record's `enc`:
 *   BSW_READS_CODES   base j is the byte raw[raw_off + j], stored as min(byte, 4)
 *   BSW_READS_ASCII   base j is the letter raw[raw_off + j]: A a 0, C c 1, G g 2, T t 3, every other byte 4
 *   BSW_READS_PACKED  base j is nibble j & 15 of the uint64 at raw[raw_off + 8 (j >> 4)], raw_off a multiple of 8, stored as
 *                     min(nibble, 4)
 * in nibble j & 15 of word woff + (j >> 4); the nibbles behind the last base are zero; a read of length 0 writes nothing.  Records of
 * different encodings may stand in one launch.  The raw buffer and the store are "device" memory of the double: ASan is the
 * witness that no offset leaves an allocation — the raw bytes a read needs are asked for exactly — and the stand-in dies when
 * either does not live on the stream's device, on an encoding it does not know, and on a packed read off its boundary. */
#include "../../bwa-mem-sw_amd/csrc/bsw_internal.h"
#include "../../bwa-mem-sw_amd/csrc/bsw_reads_pack.h"
#include "hip_double.h"

#include <atomic>
#include <cstring>

static std::atomic<uint64_t> g_launches{0}, g_reads{0}, g_by_enc[3];

namespace standin_rdpack {
uint64_t launches() { return g_launches; }
uint64_t reads() { return g_reads; }
uint64_t reads_of(int enc) { return g_by_enc[enc]; }
void reset() { g_launches = 0; g_reads = 0; for (auto &c : g_by_enc) c = 0; }
}  // namespace standin_rdpack

static unsigned letter_code(uint8_t b)
{
    switch (b) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}

namespace bsw {

hipError_t launch_reads_pack(const uint8_t *raw, const bsw_rdpack_rec *rec, uint32_t n, uint64_t *store, hipStream_t s)
{
    const hipError_t g = hipdbl::gate("launch_reads_pack");
    if (g != hipSuccess) return g;
    const int dev = hipdbl::device_of_stream(s);
    hipdbl::enqueue(s, [=]() {
        if (n && (hipdbl::device_of_ptr(raw, 1) != dev || hipdbl::device_of_ptr(rec, n * sizeof(*rec)) != dev))
            hipdbl::die("stand-in launch_reads_pack: the raw bytes or the records of a piece of device %d do not live there", dev);
        for (uint32_t i = 0; i < n; ++i) {
            const bsw_rdpack_rec R = rec[i];
            if (R.len < 0) hipdbl::die("stand-in launch_reads_pack: record %u has length %d", i, R.len);
            if (R.enc > 2u) hipdbl::die("stand-in launch_reads_pack: record %u has encoding %u", i, R.enc);
            const size_t nw = (size_t)((R.len + 15) >> 4);
            const size_t rawb = R.enc == BSW_READS_PACKED ? 8 * nw : (size_t)R.len;
            if (!R.len) { g_by_enc[R.enc] += 1; continue; }
            if (R.enc == BSW_READS_PACKED && (R.raw_off & 7u)) hipdbl::die("stand-in launch_reads_pack: the words of read %u start at byte %u of the raw buffer", i, R.raw_off);
            if (hipdbl::device_of_ptr(raw + R.raw_off, rawb) != dev) hipdbl::die("stand-in launch_reads_pack: the raw bytes of read %u leave the buffer of device %d", i, dev);
            if (hipdbl::device_of_ptr(store + R.woff, 8 * nw) != dev) hipdbl::die("stand-in launch_reads_pack: the words of read %u leave the copy of device %d", i, dev);
            for (int j = 0; j < R.len; ++j) {
                unsigned c;
                if (R.enc == BSW_READS_PACKED) {
                    uint64_t in;
                    memcpy(&in, raw + (size_t)R.raw_off + 8 * (size_t)(j >> 4), 8);
                    c = (unsigned)(in >> (4 * (j & 15))) & 15u;
                    if (c > 4) c = 4;
                } else {
                    const uint8_t b = raw[(size_t)R.raw_off + (size_t)j];
                    c = R.enc == BSW_READS_ASCII ? letter_code(b) : (b > 4 ? 4u : b);
                }
                uint64_t &w = store[(size_t)R.woff + (size_t)(j >> 4)];
                if (!(j & 15)) w = 0;
                w |= (uint64_t)c << (4 * (j & 15));
            }
            g_by_enc[R.enc] += 1;
        }
        g_launches += 1;
        g_reads += n;
    });
    return hipSuccess;
}

}  // namespace bsw
