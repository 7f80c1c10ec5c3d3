/* treeset_plan.h -- what the host makes of one tree for the tree set (host/pllhip_treeset.c), and what the device
 * reads (pll_treeset_dev.hip, kernels_treeset.hpp).  Contract: INTEGRATION.md, "Split support and tree distances";
 * design: DESIGN.md section 16.
 *
 * A tree of T tips is rooted at the tip of id 0.  Below that tip's neighbour hang the other T - 1 tips; visited depth
 * first they form `order`, and the tips below every inner node are one interval of it.
 *
 *   split plan        order[T - 1], and lo/hi[T - 3]: the T - 3 inner edges as intervals [lo, hi) of order.  None holds
 *                     tip 0, so the normalised split is always the complement of the interval's tips.
 *   transfer program  2T - 3 steps in postorder: "push tip t" and "combine the two top entries; this node has s tips".
 *                     The child that needs the deeper stack comes first, so the stack never holds more than
 *                     1 + floor(log2(T)) entries (<= PLLHIP_TS_MAX_STACK for T <= 65535).
 */
#ifndef PLLHIP_TREESET_PLAN_H_INCLUDED
#define PLLHIP_TREESET_PLAN_H_INCLUDED

#include <stdint.h>

#include "pll.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PLLHIP_TS_MAX_TIPS  65535u
#define PLLHIP_TS_MAX_STACK 17u
#define PLLHIP_TS_PUSH      0u
#define PLLHIP_TS_COMBINE   1u

typedef struct pllhip_ts_step
{
  uint32_t kind;   /* PLLHIP_TS_PUSH | PLLHIP_TS_COMBINE */
  uint32_t arg;    /* push: the tip's id; combine: the number of tips below the node */
} pllhip_ts_step_t;

typedef struct pllhip_ts_labels pllhip_ts_labels_t;

#ifdef __HIPCC__
#define PLLHIP_TS_BOTH __host__ __device__
#else
#define PLLHIP_TS_BOTH
#endif

/* the key of a tip: a split's hash is the sum of the keys of the tips whose bit is set */
PLLHIP_TS_BOTH static inline uint64_t pllhip_ts_key(uint32_t tip)
{
  uint64_t k = ((uint64_t)tip + 1u) * 0x9e3779b97f4a7c15ULL;
  k ^= k >> 33; k *= 0xff51afd7ed558ccdULL; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ULL; k ^= k >> 33;
  return k;
}

static inline unsigned int pllhip_ts_words(unsigned int tip_count) { return (tip_count + 31u) / 32u; }

/* label -> id table; NULL and pll_errno = PLL_ERROR_PARAM_INVALID for a NULL or duplicate label */
pllhip_ts_labels_t * pllhip_ts_labels_create(unsigned int tip_count, const char * const * labels);
void pllhip_ts_labels_destroy(pllhip_ts_labels_t * table);
/* -1: unknown */
long pllhip_ts_labels_find(const pllhip_ts_labels_t * table, const char * label);
/* the label of tip `id`; NULL: no such tip */
const char * pllhip_ts_labels_get(const pllhip_ts_labels_t * table, unsigned int id);

/* order [T - 1], lo, hi, edge [T - 3] (edge may be NULL: the record of every inner edge in the caller's tree, on the
 * side away from tip 0), program [2T - 3].  *max_stack: the deepest stack the program reaches.  The tree is only read.
 * PLL_FAILURE with pll_errno PLL_ERROR_PARAM_INVALID (tip ids, labels), PLL_ERROR_TREE_INVALID (not binary, not T
 * tips, broken links, stack bound) or PLL_ERROR_MEM_ALLOC. */
int pllhip_ts_flatten(const pll_utree_t * tree, unsigned int tip_count, const pllhip_ts_labels_t * labels,
                      uint32_t * order, uint32_t * lo, uint32_t * hi, pll_unode_t ** edge,
                      pllhip_ts_step_t * program, unsigned int * max_stack);

/* the T - 3 normalised splits of a plan, in plan order: words [(T - 3) * ceil(T / 32)], hash [T - 3] (may be NULL) */
void pllhip_ts_plan_splits(unsigned int tip_count, const uint32_t * order, const uint32_t * lo, const uint32_t * hi,
                           uint32_t * words, uint64_t * hash);
/* perm [count]: the indices of the splits ascending by words compared as unsigned, word 0 first */
void pllhip_ts_sort_splits(unsigned int tip_count, unsigned int count, const uint32_t * words, uint32_t * perm);

/* ---- consensus (host/pllhip_consensus.c; device: kernels_treeset.hpp, k_cs_*) ---- */

/* The integer thresholds of a consensus over B trees.  A split held by c trees is in outright when c >= *need_major
 * and is a candidate at all when c >= *need_minor (<= *need_major).  threshold 1.0: need_major = B.  A cut
 * max(threshold, 0.5) of exactly 0.5: the smallest c with 2c > B.  Any other cut: the smallest c for which the one
 * correctly rounded quotient (double)c / (double)B is greater than the cut.  need_minor = need_major for a threshold
 * >= 0.5, 1 for 0.0, and else the smallest c with (double)c / (double)B > threshold.
 * PLL_FAILURE with PLL_ERROR_PARAM_INVALID for B = 0 or a threshold outside [0, 1] (NaN included). */
int pllhip_ts_consensus_needs(unsigned int tree_count, double threshold, unsigned int * need_major,
                              unsigned int * need_minor);

/* The unrooted, possibly multifurcating tree of `count` (0 .. T - 3) pairwise compatible, distinct, non-trivial splits
 * in normal form (bit 0 of word 0 set, unused high bits clear): words [count][ceil(T / 32)], support [count] or NULL.
 * Tips carry node_index = clv_index = tip id and the table's label (labels may be NULL: no labels).  The inner node on
 * the side of a split's edge away from tip 0 carries the split's support as its label, in the shortest decimal form
 * that reads back as the same double; every record of that node points to the one string, as pll_utree_clone
 * leaves it, so pll_utree_destroy(tree, NULL) frees everything.  vroot is tip 0's neighbour; count = 0 gives the star.
 * NULL with PLL_ERROR_PARAM_INVALID (a split that is not in normal form, trivial, given twice, or incompatible with
 * another) or PLL_ERROR_MEM_ALLOC. */
pll_utree_t * pllhip_ts_tree_from_splits(unsigned int tip_count, const pllhip_ts_labels_t * labels, unsigned int count,
                                         const uint32_t * words, const double * support);

#ifdef __cplusplus
}
#endif

#endif
