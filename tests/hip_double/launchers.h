/* launchers.h — what the test programs can ask the CPU stand-ins of the kernel launchers (launchers.cpp; TEST INFRASTRUCTURE). */
#ifndef BSW_STANDIN_LAUNCHERS_H
#define BSW_STANDIN_LAUNCHERS_H

#include <cstdint>
#include <vector>

namespace standin {
void reset();                                        /* forget ledgers and statistics (call next to hipdbl::reset) */
std::vector<uint32_t> device_tags(int dev);          /* tags of the seeds whose results were computed on that device, in any order */
uint64_t chunks_checked();                           /* result copies whose chunk ledger was checked */
uint64_t bins_beyond_4n16();                         /* launch_bin calls whose N list ended behind order[4*n+16) */
uint64_t max_order_end();                            /* the largest nlist_off + nlist_cap seen */
uint64_t chain_waits();                              /* launch_wait_count calls */
}  // namespace standin

#endif
