/* nj_tree.h -- host/pllhip_nj.c for pll_distance_dev.hip: the join list of pllhip_distmat_nj_joins -> a tree */
#ifndef PLLHIP_NJ_TREE_H
#define PLLHIP_NJ_TREE_H

#include "pll.h"

#ifdef __cplusplus
extern "C" {
#endif

/* slots / lengths: tips - 3 rounds of two entries, then three; labels may be NULL; NULL on failure (pll_errno) */
pll_utree_t * pllhip_nj_build_tree(unsigned int tips, const unsigned int * slots, const double * lengths,
                                   const char * const * labels);

#ifdef __cplusplus
}
#endif

#endif
