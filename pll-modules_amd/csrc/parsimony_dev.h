/*
 * parsimony_dev.h -- device side of the parsimony engine (pll_parsimony_dev.hip), called by the host code of
 * csrc/host/pll_parsimony.c.  Internal to the library; plain C.
 *
 * One object per partition: the packed state sets of its tips and of up to tips - 2 inner nodes (node ids:
 * tips 0 .. tips-1 = tip indices, inner nodes tips .. 2 tips - 3), the set above every inner node, and the
 * pattern weights as bit planes -- on the partition's device, or per shard on the shards' devices.  It holds no
 * reference to the partition once created.
 */
#ifndef PLLHIP_PARSIMONY_DEV_H_INCLUDED
#define PLLHIP_PARSIMONY_DEV_H_INCLUDED

#include "pll.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pllhip_pars_dev_s pllhip_pars_dev_t;

/* packs the tips of `partition` (any tip representation the engine holds) on its device(s); NULL + pll_errno */
pllhip_pars_dev_t * pllhip_pars_dev_create(const pll_partition_t * partition);
void pllhip_pars_dev_destroy(pllhip_pars_dev_t * dev);

/* Queues one walk (kernels_parsimony.hpp, k_pars_walk): `ops` = ndown triples then npre quadruples.  cand: node id
   of the candidate set (< 0: none, npre must be 0).  count_score: add the down ops' cost to the score.  Returns
   PLL_FAILURE + pll_errno on a HIP error. */
int pllhip_pars_dev_launch(pllhip_pars_dev_t * dev, const int * ops, unsigned int ndown, unsigned int npre,
                           int cand, int count_score);
/* Waits for the last walk and ADDS its per-edge costs (npre values) and its score to the accumulators (either
   may be NULL). */
int pllhip_pars_dev_collect(pllhip_pars_dev_t * dev, unsigned long long * edge_acc, unsigned long long * score_acc);

/* SPR rounds (k_pars_spr).  hint: the batch that fills the chip for this object's site count.  reserve: scratch for
   up to `want` pruned subtrees per launch (at least 1) plus schedule and cost buffers for them; returns
   the batch the object now holds (<= want), 0 + pll_errno on failure.  launch: `ops` (nops ints) then `nmem`
   member records {first op, ndown, npre, candidate node, first output}, nout counts in all.  collect: waits and
   ADDS the nout counts to acc. */
unsigned pllhip_pars_dev_spr_hint(const pllhip_pars_dev_t * dev);
unsigned pllhip_pars_dev_spr_reserve(pllhip_pars_dev_t * dev, unsigned want);
int pllhip_pars_dev_spr_launch(pllhip_pars_dev_t * dev, const int * ops, size_t nops, const int * members,
                               unsigned nmem, unsigned nout);
int pllhip_pars_dev_spr_collect(pllhip_pars_dev_t * dev, unsigned long long * acc);

/* operand encoding of the SPR schedule (kernels_parsimony.hpp) */
#define PLLHIP_PARS_SRC_D 0
#define PLLHIP_PARS_SRC_U 1
#define PLLHIP_PARS_SRC_X 2

#ifdef __cplusplus
}
#endif

#endif
