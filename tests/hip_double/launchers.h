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
uint64_t f4_rounds();                                /* launch rounds of the global / align stand-ins whose ledger was checked */
uint64_t f4_tasks();                                 /* tasks those stand-ins computed */
/* the stand-ins' restatement of the align and global class tables (host_parity tables prints them) */
int align_class_count();
int align_class_of(int qlen, int byte_mode);
int global_class_count();
int global_class_cols(int cls);
int global_long_class_count();
int global_long_ring(int cls);                       /* records of the LDS ring of class cls */
}  // namespace standin

#endif
