/* bsw_sdp_pass.h — what bsw_sdp.c and bsw_rescue.c share inside the library (plain C; not installed). */
#ifndef BSW_SDP_PASS_H
#define BSW_SDP_PASS_H
#include "../../include/bwa_sw_mi355.h"

#ifdef __cplusplus
extern "C" {
#endif
/* bsw_sdp.c: mem_sort_dedup_patch on ONE read's regions with patch = 0, in place: the sort by re, the redundancy kills, the sort
 * by (score, rb, qb) and the removal of duplicates, both sorts stable on the order a[] has on entry.  src is carried along;
 * src_tmp is n values of scratch.  Returns the number of regions left. */
__attribute__((visibility("hidden"))) size_t bsw_sdp_pass0(float mask_level_redun, int32_t max_chain_gap, bsw_sreg *a, size_t n, uint32_t *src_tmp);
/* bsw_rescue.c: the counts so far and the regions collect would write now, for bsw_rescue_job_stats and finish's out_cap */
__attribute__((visibility("hidden"))) int bsw_rescue_peek(const bsw_rescue_eng *eng, bsw_rescue_stats *stats, size_t *n_out);
#ifdef __cplusplus
}
#endif
#endif
