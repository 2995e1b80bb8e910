/* launchers_reads.h — what the resident-read test program can ask its launch_pack stand-in (launchers_reads.cpp; TEST INFRASTRUCTURE). */
#ifndef BSW_STANDIN_LAUNCHERS_READS_H
#define BSW_STANDIN_LAUNCHERS_READS_H

#include <cstdint>

namespace standin_reads {
void set_max_query_len(int n);                       /* the longest query side the program's store launches pack (sizes the stand-in's scratch) */
uint64_t store_launches();                           /* pack launches that took their queries from a read block */
uint64_t store_bases();                              /* query bases those launches fetched */
void reset();
}  // namespace standin_reads

#endif
